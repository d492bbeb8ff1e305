// shade_dev.hip -- lit render buffers: three unshared VertexNormalColor per triangle of the current fragments, each with the normal of
// its face, on the device: what Poly::RenderPolyhedronNormal (Inc/Poly.h:50-61, Src/Poly.cpp:619-679) hands a renderer, where k_faces
// writes Poly::RenderPolyhedron's zero normals.
//
// Definition (include/surtr_hip.h carries it in full): the faces are the loops Poly::ExtractFaces yields, in its order; the normal of a
// loop is its Newell sum from its smallest vertex, in double, normalised; a triangle belongs to the lowest-numbered face that owns a
// half-edge leaving each of its corners.  This walker is built for Mesh-sized loops (a cap of a 100 000-vertex piece has about 100 000
// corners): no lane walks a loop, everything is pointer jumping or a tree, O(H log L) per fragment.
//
//   k_sh_faces    one workgroup per fragment, a thread per half-edge in strides.  (1) the successor of every half-edge -- its origin by
//                 bisection of the ring offsets, its place in the target's ring by a scan of that ring -- and whether the successor is a
//                 permutation (integer counts); (2) the leader (smallest id) of every loop by pointer jumping; (3) the distance of every
//                 half-edge to its loop's end by pointer jumping on the loop cut at its leader, hence its rank and the loop's length; a
//                 scan over the leaders numbers the faces and lays the loops out one after the other; (4) every half-edge puts its term
//                 of the Newell sum at (loop base + rank) and the loops are summed as balanced trees in place: in round d entry i with
//                 i mod 2d == 0 takes entry i + d.  Jumps go from one buffer to another, the tree's readers and writers of a round are
//                 disjoint: the same bits whatever the order the threads run in.  Two tiers: the ten words per half-edge lie in LDS for
//                 fragments of up to SURTR_SHADE_LH (2048) half-edges, in a slice of global scratch above (a second launch of a few workgroups).
//   k_sh_scan     one workgroup: totals, the capacity check, the header and the records
//   k_sh_emit     a lane per triangle: the common face of its corners (the smallest ring against the other two), the normal of that
//                 face or of the triangle itself, three 36-byte vertices
// The context keeps nothing: one temporary allocation per call, ordered on the context's stream, and no host synchronisation in the
// _dev form.  The kernels only read the arena.
#include <cmath>
#include <cstring>

#include "surtr_ctx.h"

static_assert(sizeof(surtr_shaded) == 16, "surtr_shaded is 16 bytes");

// Half-edges of a fragment whose scratch lies in LDS, 40 bytes each.  4096 do not fit a CU's 160 KB at all; 2048 are 82 KB, one
// workgroup (four waves) per CU; 1024 are 42 KB, three per CU.  Measured on a configs[3] event: the fragments
// between the two limits are few but large, and left to the handful of workgroups of the global tier they are the call's tail --
// 2048 is the faster limit there, and no slower on a click's few small fragments.
#ifndef SURTR_SHADE_LH
#define SURTR_SHADE_LH 2048u
#endif
#define SH_WG SURTR_WG
#define SH_WORDS 10u                 // scratch words per half-edge: four of topology, six that are jump buffers first and the sums then
#define SH_WHOLE 0x80000000u         // (work records only) the fragment takes the fallback as a whole

namespace {

struct ShWork
{
    uint32_t nmax, hcap, lds_limit, HG;      // fragments / packed half-edges there is room for; tier limit; half-edges of a global slice
    uint32_t* hdr;            // [0] fragments [1] the caller's buffers hold everything: k_sh_emit runs
    surtr_shaded* rec;        // per fragment: faces and status as k_sh_faces found them
    uint32_t* hlead;          // per Mesh half-edge, in the packed order of the download (o_mh + e): the leader of its loop
    uint32_t* hfno;           // at the leaders: the face number
    float* fnorm;             // at the leaders: the normal
    uint32_t* slices;         // global tier: SH_WORDS * HG words per workgroup
};

// One fragment's Mesh: ring(v) = nbr[loff[v] - mh_off .. + llen[v]); half-edge id = position in nbr.
struct ShFrag { const float* pos; const uint32_t* loff; const uint32_t* llen; const int32_t* nbr; uint32_t n, H, mh_off; };

__device__ __forceinline__ ShFrag sh_frag(const FragRec& fr, const Arena& A)
{
    return ShFrag{A.pos + 3 * (size_t)fr.mv_off, A.loff + fr.mv_off, A.llen + fr.mv_off, A.nbr + fr.mh_off, fr.mv_n, fr.mh_n, fr.mh_off};
}
// The vertex whose ring holds half-edge e: the last one whose ring starts at or before e.
__device__ __forceinline__ uint32_t sh_org(const ShFrag& F, uint32_t e)
{
    uint32_t lo = 0, hi = F.n;
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (F.loff[mid] - F.mh_off <= e) lo = mid; else hi = mid; }
    return lo;
}
struct ShD3 { double x, y, z; };
__device__ __forceinline__ ShD3 sh_pos(const ShFrag& F, uint32_t v)
{
    return ShD3{(double)F.pos[3 * (size_t)v], (double)F.pos[3 * (size_t)v + 1], (double)F.pos[3 * (size_t)v + 2]};
}
__device__ __forceinline__ ShD3 sh_cross(const ShD3& a, const ShD3& b) { return ShD3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// n = N / sqrt(N.N) rounded to float; zero when N.N is zero or not finite
__device__ __forceinline__ void sh_normalise(const ShD3& N, float out[3])
{
    const double nn = (N.x * N.x + N.y * N.y) + N.z * N.z;
    out[0] = 0.f; out[1] = 0.f; out[2] = 0.f;
    if (!(nn > 0.0) || !(nn <= 1.7976931348623157e308)) return;
    const double len = sqrt(nn);
    out[0] = (float)(N.x / len); out[1] = (float)(N.y / len); out[2] = (float)(N.z / len);
}

// Steps 1 to 4 on one fragment.  U: SH_WORDS * H words, 8-byte aligned, LDS or global.
__device__ __forceinline__ void sh_fragment(const ShFrag& F, uint32_t* U, uint32_t o_mh, const ShWork& W, surtr_shaded* rec)
{
    __shared__ uint32_t sc[2][SH_WG + 1];
    __shared__ uint32_t s_kmax;
    const uint32_t tid = threadIdx.x, G = group_size(), H = F.H;
    uint32_t* nxt = U; uint32_t* a1 = U + H; uint32_t* a2 = U + 2 * (size_t)H; uint32_t* a3 = U + 3 * (size_t)H;
    uint32_t* r0 = U + 4 * (size_t)H; uint32_t* r1 = U + 5 * (size_t)H;
    double* T = (double*)(U + 4 * (size_t)H);      // 3 H doubles over r0, r1 and the four arrays behind them

    // (1) successor; a1 counts how many half-edges name each one as theirs
    int bad = 0;
    for (uint32_t e = tid; e < H; e += G) a1[e] = 0;
    for (uint32_t v = tid; v < F.n; v += G) { const uint32_t r = F.loff[v] - F.mh_off; if (r > H || F.llen[v] > H - r) bad = 1; }
    bad = __syncthreads_or(bad);
    if (!bad)
    {
        for (uint32_t e = tid; e < H; e += G)
        {
            nxt[e] = e;
            const uint32_t a = sh_org(F, e), ra = F.loff[a] - F.mh_off;
            if (!(ra <= e && e - ra < F.llen[a])) { bad = 1; continue; }      // the rings are not packed in vertex order
            const uint32_t b = (uint32_t)F.nbr[e];
            if (b >= F.n) { bad = 1; continue; }                              // the entry names no vertex
            const uint32_t rb = F.loff[b] - F.mh_off, lb = F.llen[b];
            uint32_t k = 0;
            while (k < lb && (uint32_t)F.nbr[rb + k] != a) ++k;
            if (k == lb) { bad = 1; continue; }                               // the link lacks its way back
            const uint32_t nx = rb + (k == 0u ? lb - 1u : k - 1u);
            nxt[e] = nx;
            atomicAdd(&a1[nx], 1u);
        }
        __syncthreads();
        for (uint32_t e = tid; e < H; e += G) if (a1[e] != 1u) bad = 1;       // a ring lists a neighbour twice
        bad = __syncthreads_or(bad);
    }
    if (bad)
    {
        if (tid == 0u) { rec->n_faces = 0; rec->status = SH_WHOLE; }
        return;
    }

    // (2) leaders: a1 / a2 the smallest id seen, a3 / r0 the jump, from one buffer into the other
    for (uint32_t e = tid; e < H; e += G) { a1[e] = e; a3[e] = nxt[e]; }
    __syncthreads();
    uint32_t* Lc = a1; uint32_t* Ln = a2; uint32_t* Jc = a3; uint32_t* Jn = r0;
    for (uint32_t span = 1; span < H; span <<= 1)
    {
        for (uint32_t e = tid; e < H; e += G) { const uint32_t j = Jc[e], x = Lc[e], y = Lc[j]; Ln[e] = x < y ? x : y; Jn[e] = Jc[j]; }
        __syncthreads();
        uint32_t* t = Lc; Lc = Ln; Ln = t; t = Jc; Jc = Jn; Jn = t;
    }
    if (Lc != a1)
    {
        for (uint32_t e = tid; e < H; e += G) a1[e] = Lc[e];
        __syncthreads();
    }
    const uint32_t* lead = a1;

    // (3) distance to the loop's end (the half-edge whose successor is the leader): a2 / a3 the distance, r0 / r1 the jump
    for (uint32_t e = tid; e < H; e += G) { const uint32_t nx = nxt[e]; const bool last = lead[nx] == nx; a2[e] = last ? 0u : 1u; r0[e] = last ? e : nx; }
    __syncthreads();
    uint32_t* Dc = a2; uint32_t* Dn = a3; Jc = r0; Jn = r1;
    for (uint32_t span = 1; span < H; span <<= 1)
    {
        for (uint32_t e = tid; e < H; e += G) { const uint32_t j = Jc[e]; Dn[e] = Dc[e] + Dc[j]; Jn[e] = Jc[j]; }
        __syncthreads();
        uint32_t* t = Dc; Dc = Dn; Dn = t; t = Jc; Jc = Jn; Jn = t;
    }
    if (Dc != a2)
    {
        for (uint32_t e = tid; e < H; e += G) a2[e] = Dc[e];
        __syncthreads();
    }
    const uint32_t* dist = a2;
    // face numbers and loop bases: exclusive sums over the leaders in id order (a chunk per thread, thread 0 adds the chunks up).
    // From here nxt[leader] = the loop's base and a3[leader] = its length.
    const uint32_t chunk = (H + G - 1u) / G;
    const uint32_t e0 = tid * chunk < H ? tid * chunk : H, e1 = e0 + chunk < H ? e0 + chunk : H;
    uint32_t cf = 0, ck = 0, kmax = 0;
    for (uint32_t e = e0; e < e1; ++e) if (lead[e] == e) { ++cf; ck += dist[e] + 1u; }
    sc[0][tid] = cf; sc[1][tid] = ck;
    if (tid == 0u) s_kmax = 0;
    __syncthreads();
    if (tid == 0u)
        for (int q = 0; q < 2; ++q)
        {
            uint32_t run = 0;
            for (uint32_t t = 0; t < G; ++t) { const uint32_t x = sc[q][t]; sc[q][t] = run; run += x; }
            sc[q][SH_WG] = run;
        }
    __syncthreads();
    cf = sc[0][tid]; ck = sc[1][tid];
    const uint32_t n_faces = sc[0][SH_WG];
    for (uint32_t e = e0; e < e1; ++e)
        if (lead[e] == e)
        {
            const uint32_t k = dist[e] + 1u;
            W.hfno[o_mh + e] = cf; nxt[e] = ck; a3[e] = k;
            ++cf; ck += k; kmax = k > kmax ? k : kmax;
        }
    if (kmax) atomicMax(&s_kmax, kmax);
    __syncthreads();
    kmax = s_kmax;

    // (4) the terms in loop order, then the trees
    for (uint32_t e = tid; e < H; e += G)
    {
        const uint32_t l = lead[e], k = a3[l], i = k - 1u - dist[e];
        double* t = T + 3 * (size_t)(nxt[l] + i);
        ShD3 c{0.0, 0.0, 0.0};
        if (i >= 1u && i + 2u <= k)
        {
            const ShD3 q0 = sh_pos(F, sh_org(F, l)), qa = sh_pos(F, sh_org(F, e)), qb = sh_pos(F, (uint32_t)F.nbr[e]);
            c = sh_cross(ShD3{qa.x - q0.x, qa.y - q0.y, qa.z - q0.z}, ShD3{qb.x - q0.x, qb.y - q0.y, qb.z - q0.z});
        }
        t[0] = c.x; t[1] = c.y; t[2] = c.z;
    }
    __syncthreads();
    for (uint32_t d = 1; d < kmax; d <<= 1)
    {
        for (uint32_t e = tid; e < H; e += G)
        {
            const uint32_t l = lead[e], k = a3[l], i = k - 1u - dist[e];
            if ((i & (2u * d - 1u)) != 0u || i + d >= k) continue;
            double* t = T + 3 * (size_t)(nxt[l] + i);
            const double* u = t + 3 * (size_t)d;
            t[0] = t[0] + u[0]; t[1] = t[1] + u[1]; t[2] = t[2] + u[2];
        }
        __syncthreads();
    }
    for (uint32_t e = tid; e < H; e += G)
    {
        W.hlead[o_mh + e] = lead[e];
        if (lead[e] != e) continue;
        const double* t = T + 3 * (size_t)nxt[e];
        float n[3] = {0.f, 0.f, 0.f};
        if (a3[e] >= 3u) sh_normalise(ShD3{t[0], t[1], t[2]}, n);
        float* o = W.fnorm + 3 * (size_t)(o_mh + e);
        o[0] = n[0]; o[1] = n[1]; o[2] = n[2];
    }
    if (tid == 0u) { rec->n_faces = n_faces; rec->status = 0; }
}

// tier 0: the fragments of up to lds_limit half-edges, scratch in LDS; tier 1: the others, scratch in this workgroup's global slice.
__global__ __launch_bounds__(SH_WG) void k_sh_faces(const FragRec* __restrict__ frags, const surtr_counts* __restrict__ counts, Arena A, ShWork W, uint32_t tier)
{
    __shared__ unsigned long long s_u[(size_t)SH_WORDS * SURTR_SHADE_LH / 2u];
    if (counts->status != 0u) return;
    uint32_t n = counts->n_frag;
    if (n > W.nmax) n = W.nmax;
    for (uint32_t f = blockIdx.x; f < n; f += gridDim.x)
    {
        const FragRec fr = frags[f];
        const bool in_lds = fr.mh_n <= W.lds_limit;
        if (in_lds != (tier == 0u)) continue;
        // nothing to walk, no room in the call's tables, or more half-edges than a global slice holds: per-triangle normals
        if (fr.mh_n == 0u || fr.mv_n == 0u || fr.o_mh > W.hcap || fr.mh_n > W.hcap - fr.o_mh || (!in_lds && fr.mh_n > W.HG))
        {
            if (threadIdx.x == 0u) { W.rec[f].n_faces = 0; W.rec[f].status = SH_WHOLE; }
            continue;
        }
        uint32_t* U = in_lds ? (uint32_t*)s_u : W.slices + (size_t)blockIdx.x * SH_WORDS * W.HG;
        sh_fragment(sh_frag(fr, A), U, fr.o_mh, W, &W.rec[f]);
        __syncthreads();
    }
}

// records_bytes >= 16 (checked on the host): the header is always written; the records only when everything fits.
__global__ __launch_bounds__(SH_WG) void k_sh_scan(const FragRec* __restrict__ frags, const surtr_counts* __restrict__ counts, ShWork W,
                                                   surtr_shaded* __restrict__ out, size_t records_bytes, size_t vnc_cap, uint32_t with_tri, size_t tri_cap)
{
    __shared__ uint32_t sc[2][SH_WG + 1];
    const uint32_t failed = counts->status;
    const uint32_t all = failed ? 0u : counts->n_frag;
    const uint32_t n = all < W.nmax ? all : W.nmax;
    const uint32_t G = group_size(), seg = (n + G - 1u) / G;
    const uint32_t f0 = threadIdx.x * seg < n ? threadIdx.x * seg : n, f1 = f0 + seg < n ? f0 + seg : n;
    uint32_t nf = 0, nv = 0;
    for (uint32_t f = f0; f < f1; ++f) { nf += W.rec[f].n_faces; nv += frags[f].idx_n; }
    sc[0][threadIdx.x] = nf; sc[1][threadIdx.x] = nv;
    __syncthreads();
    if (threadIdx.x == 0u)
        for (int q = 0; q < 2; ++q)
        {
            uint32_t run = 0;
            for (uint32_t t = 0; t < G; ++t) run += sc[q][t];
            sc[q][SH_WG] = run;
        }
    __syncthreads();
    const uint32_t tf = sc[0][SH_WG], tv = sc[1][SH_WG];
    const bool fits = !failed && all <= W.nmax && ((size_t)n + 1u) * sizeof(surtr_shaded) <= records_bytes && tv <= vnc_cap && (!with_tri || tv / 3u <= tri_cap);
    if (fits)
        for (uint32_t f = f0; f < f1; ++f)
        {
            const surtr_shaded r = W.rec[f];
            out[1u + f] = surtr_shaded{frags[f].o_idx, frags[f].idx_n, r.n_faces, (r.status & SH_WHOLE) ? (uint32_t)SURTR_SHADE_PER_TRIANGLE : 0u};
        }
    if (threadIdx.x == 0u)
    {
        out[0] = surtr_shaded{all, tv, tf, failed ? failed : (fits ? (uint32_t)SURTR_OK : (uint32_t)SURTR_E_CAPACITY)};
        W.hdr[0] = n; W.hdr[1] = fits ? 1u : 0u;
    }
}

__device__ __forceinline__ bool sh_ring_has(const uint32_t* hl, uint32_t len, uint32_t x)
{
    for (uint32_t s = 0; s < len; ++s) if (hl[s] == x) return true;
    return false;
}

__global__ __launch_bounds__(SH_WG) void k_sh_emit(const FragRec* __restrict__ frags, Arena A, ShWork W, surtr_shaded* __restrict__ out, float* __restrict__ vnc,
                                                   size_t vnc_cap, uint32_t* __restrict__ tri_face, size_t tri_cap, float cr, float cg, float cb)
{
    if (!W.hdr[1]) return;      // a buffer of the caller's is too small: nothing but the header is written
    const uint32_t n = W.hdr[0];
    for (uint32_t f = blockIdx.x; f < n; f += gridDim.x)
    {
        const FragRec fr = frags[f];
        const uint32_t nt = fr.idx_n / 3u;
        if (nt == 0u) continue;
        const ShFrag F = sh_frag(fr, A);
        const bool whole = (W.rec[f].status & SH_WHOLE) != 0u;
        const uint32_t* hl = W.hlead + fr.o_mh;
        bool fell = false;
        for (uint32_t t = threadIdx.x; t < nt; t += group_size())
        {
            uint32_t v[3];
            bool ok = true;
            for (int c = 0; c < 3; ++c) { v[c] = A.idx[fr.idx_off + 3u * t + c]; if (v[c] >= F.n) { v[c] = 0u; ok = false; } }
            uint32_t best = 0xFFFFFFFFu;
            if (!whole && ok)
            {
                // the corner with the shortest ring first: its faces against the rings of the other two
                uint32_t r[3], len[3];
                for (int c = 0; c < 3; ++c) { r[c] = F.loff[v[c]] - F.mh_off; len[c] = F.llen[v[c]]; }
                int s0 = 0;
                if (len[1] < len[s0]) s0 = 1;
                if (len[2] < len[s0]) s0 = 2;
                const int s1 = (s0 + 1) % 3, s2 = (s0 + 2) % 3;
                for (uint32_t s = 0; s < len[s0]; ++s)
                {
                    const uint32_t x = hl[r[s0] + s];
                    if (x < best && sh_ring_has(hl + r[s1], len[s1], x) && sh_ring_has(hl + r[s2], len[s2], x)) best = x;
                }
            }
            const ShD3 pa = sh_pos(F, v[0]), pb = sh_pos(F, v[1]), pc = sh_pos(F, v[2]);
            float nrm[3];
            uint32_t fno = SURTR_SHADE_NO_FACE;
            if (best != 0xFFFFFFFFu)
            {
                fno = W.hfno[fr.o_mh + best];
                const float* q = W.fnorm + 3 * (size_t)(fr.o_mh + best);
                nrm[0] = q[0]; nrm[1] = q[1]; nrm[2] = q[2];
            }
            else
            {
                sh_normalise(sh_cross(ShD3{pb.x - pa.x, pb.y - pa.y, pb.z - pa.z}, ShD3{pc.x - pa.x, pc.y - pa.y, pc.z - pa.z}), nrm);
                fell = true;
            }
            const size_t j0 = (size_t)fr.o_idx + 3u * (size_t)t;
            if (j0 + 3u <= vnc_cap)
                for (int c = 0; c < 3; ++c)
                {
                    float* o = vnc + 9 * (j0 + c);
                    const float* p = F.pos + 3 * (size_t)v[c];
                    o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = nrm[0]; o[4] = nrm[1]; o[5] = nrm[2]; o[6] = cr; o[7] = cg; o[8] = cb;
                }
            if (tri_face && j0 / 3u < tri_cap) tri_face[j0 / 3u] = fno;
        }
        if (fell && !whole) atomicOr(&out[1u + f].status, (uint32_t)SURTR_SHADE_PER_TRIANGLE);
    }
}

// The call's scratch: one allocation ordered on the stream (the emulation runs everything in program order).
hipError_t sh_alloc(void** p, size_t bytes, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    return hipMallocAsync(p, bytes, st);
#else
    (void)st;
    return hipMalloc(p, bytes);
#endif
}
void sh_free(void* p, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    (void)hipFreeAsync(p, st);
#else
    (void)st;
    (void)hipFree(p);
#endif
}

int sh_launch(surtr_ctx* ctx, uint32_t nmax, uint32_t hcap, const float color[3], void* dev_records, size_t records_bytes, float* dev_vnc, size_t vnc_cap,
              uint32_t* dev_tri_face, size_t tri_cap)
{
    hipStream_t st = ctx->stream;
    ShWork W;
    memset(&W, 0, sizeof(W));
    W.nmax = nmax; W.hcap = hcap;
    W.lds_limit = ctx->shade_lds_limit ? std::min(ctx->shade_lds_limit, (uint32_t)SURTR_SHADE_LH) : (uint32_t)SURTR_SHADE_LH;
    // the global tier: slices for a fragment as large as k_faces has room for, as many as a quarter of a gigabyte holds (1 .. 32)
    W.HG = std::max(std::max(ctx->fs.HF, ctx->fs_big.HF), W.lds_limit + 1u);
    const size_t slice = (size_t)SH_WORDS * W.HG * 4;
    const uint32_t n_slices = (uint32_t)std::min<size_t>(std::min<size_t>(32, std::max(nmax, 1u)), std::max<size_t>(1, ((size_t)256 << 20) / slice));
    auto up = [](size_t b) { return (b + 255) & ~(size_t)255; };
    const size_t o_rec = 256, o_lead = o_rec + up((size_t)std::max(nmax, 1u) * sizeof(surtr_shaded)), o_fno = o_lead + up((size_t)hcap * 4),
                 o_norm = o_fno + up((size_t)hcap * 4), o_sl = o_norm + up((size_t)hcap * 12), bytes = o_sl + slice * n_slices;
    char* base = nullptr;
    HIPCHK(sh_alloc((void**)&base, bytes, st));
    W.hdr = (uint32_t*)base; W.rec = (surtr_shaded*)(base + o_rec); W.hlead = (uint32_t*)(base + o_lead); W.hfno = (uint32_t*)(base + o_fno);
    W.fnorm = (float*)(base + o_norm); W.slices = (uint32_t*)(base + o_sl);
    hipError_t e = hipMemsetAsync(W.hdr, 0, 16, st);
    if (e == hipSuccess)
    {
        const uint32_t grid = std::max(1u, std::min(nmax, 4096u));
        const float cr = color ? color[0] : 0.25f, cg = color ? color[1] : 0.25f, cb = color ? color[2] : 0.25f;
        hipLaunchKernelGGL(k_sh_faces, dim3(grid), dim3(SH_WG), 0, st, (const FragRec*)ctx->d_frags, (const surtr_counts*)ctx->d_counts, ctx->arena, W, 0u);
        hipLaunchKernelGGL(k_sh_faces, dim3(n_slices), dim3(SH_WG), 0, st, (const FragRec*)ctx->d_frags, (const surtr_counts*)ctx->d_counts, ctx->arena, W, 1u);
        hipLaunchKernelGGL(k_sh_scan, dim3(1), dim3(SH_WG), 0, st, (const FragRec*)ctx->d_frags, (const surtr_counts*)ctx->d_counts, W, (surtr_shaded*)dev_records,
                           records_bytes, vnc_cap, dev_tri_face ? 1u : 0u, tri_cap);
        hipLaunchKernelGGL(k_sh_emit, dim3(grid), dim3(SH_WG), 0, st, (const FragRec*)ctx->d_frags, ctx->arena, W, (surtr_shaded*)dev_records, dev_vnc, vnc_cap,
                           dev_tri_face, tri_cap, cr, cg, cb);
        e = hipGetLastError();
    }
    sh_free(base, st);
    if (e != hipSuccess) { ctx->err = std::string("shaded: ") + hipGetErrorString(e); return SURTR_E_HIP; }
    return SURTR_OK;
}

// SURTR_E_STATE unless there are current fragments of an event that did not fail, triangulated
int sh_state(const surtr_ctx* ctx)
{
    if (!ctx->have_event) return SURTR_E_STATE;
    if (ctx->last_current && ctx->last.status) return SURTR_E_STATE;
    if (!(ctx->last_flags & SURTR_EVT_RENDER)) return SURTR_E_STATE;
    return SURTR_OK;
}

} // namespace

extern "C" int surtr_set_shade_tier(surtr_ctx* ctx, uint32_t half_edges)
{
    if (!ctx) return SURTR_E_INVALID;
    ctx->shade_lds_limit = half_edges;
    return SURTR_OK;
}

extern "C" int surtr_event_shaded_dev(surtr_ctx* ctx, const float color[3], void* dev_records, size_t records_bytes, float* dev_vnc, size_t vnc_cap,
                                      uint32_t* dev_tri_face, size_t tri_cap)
{
    if (!ctx || !dev_records || (dev_vnc == nullptr) != (vnc_cap == 0) || (dev_tri_face == nullptr) != (tri_cap == 0)) return SURTR_E_INVALID;
    const int rs = sh_state(ctx);
    if (rs) return rs;
    if (records_bytes < sizeof(surtr_shaded)) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    if (ctx->last_current)
    {
        // the host holds this event's counts: buffers too small are refused here
        const surtr_counts& c = ctx->last;
        if (((size_t)c.n_frag + 1u) * sizeof(surtr_shaded) > records_bytes || c.n_idx > vnc_cap || (dev_tri_face && c.n_idx / 3u > tri_cap)) return SURTR_E_CAPACITY;
        if (c.n_frag == 0)
        {
            HIPCHK(hipMemsetAsync(dev_records, 0, sizeof(surtr_shaded), ctx->stream));
            return SURTR_OK;
        }
        return sh_launch(ctx, c.n_frag, c.mesh_nbrs, color, dev_records, records_bytes, dev_vnc, vnc_cap, dev_tri_face, tri_cap);
    }
    // without a synchronisation: the capacities of the fragment table and the arena bound the work; the kernels read the counts on the device
    return sh_launch(ctx, ctx->cap_frags, ctx->arena.capH, color, dev_records, records_bytes, dev_vnc, vnc_cap, dev_tri_face, tri_cap);
}

extern "C" int surtr_event_shaded(surtr_ctx* ctx, const float color[3], uint32_t* n, surtr_shaded* records, uint32_t* n_vertices, float* vnc, uint32_t* tri_face,
                                  uint32_t* n_faces)
{
    if (!ctx || !n || !n_vertices) return SURTR_E_INVALID;
    const bool fill = records && vnc;
    if (!fill && (records || vnc || tri_face)) return SURTR_E_INVALID;
    if (!ctx->have_event) return SURTR_E_STATE;
    surtr_counts c;
    const int rc0 = surtr_event_counts(ctx, &c);
    if (rc0 == SURTR_OK && c.status) return SURTR_E_STATE;
    if (rc0 && ctx->last_current && ctx->last.status) return SURTR_E_STATE;      // (the counts came back: the event itself had failed)
    if (rc0) return rc0;
    const int rs = sh_state(ctx);
    if (rs) return rs;
    const bool small = fill && (*n < c.n_frag || *n_vertices < c.n_idx);
    if (small) { *n = c.n_frag; *n_vertices = c.n_idx; return SURTR_E_CAPACITY; }
    const size_t vcap = std::max<size_t>(c.n_idx, 1u), tcap = std::max<size_t>(c.n_idx / 3u, 1u);
    DevBuf<surtr_shaded> d_rec; DevBuf<float> d_vnc; DevBuf<uint32_t> d_tri;
    int rc = d_rec.grow(ctx, (size_t)c.n_frag + 1u);
    if (rc == SURTR_OK) rc = d_vnc.grow(ctx, 9 * vcap);
    if (rc == SURTR_OK && tri_face) rc = d_tri.grow(ctx, tcap);
    if (rc == SURTR_OK) rc = surtr_event_shaded_dev(ctx, color, d_rec.p, ((size_t)c.n_frag + 1u) * sizeof(surtr_shaded), d_vnc.p, vcap, d_tri.p, d_tri.p ? tcap : 0);
    if (rc) return rc;
    surtr_shaded h;
    HIPCHK(hipMemcpyAsync(&h, d_rec.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (h.status) return (int)h.status;
    *n = h.first_vertex; *n_vertices = h.n_vertices;
    if (n_faces) *n_faces = h.n_faces;
    if (!fill) return SURTR_OK;
    if (h.first_vertex) HIPCHK(hipMemcpyAsync(records, d_rec.p + 1, (size_t)h.first_vertex * sizeof(surtr_shaded), hipMemcpyDeviceToHost, ctx->stream));
    if (h.n_vertices) HIPCHK(hipMemcpyAsync(vnc, d_vnc.p, (size_t)h.n_vertices * 36, hipMemcpyDeviceToHost, ctx->stream));
    if (tri_face && h.n_vertices) HIPCHK(hipMemcpyAsync(tri_face, d_tri.p, (size_t)(h.n_vertices / 3u) * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SURTR_OK;
}
