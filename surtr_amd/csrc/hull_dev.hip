// hull_dev.hip -- collision hulls: the face loops and face planes of every Convex of the last event, or of every resident piece, on the
// device: what Compound::PieceExtractedConvex (SetExtract, Src/Surtr.cpp:2151-2155) holds for CookingConvexManual (:2555-2614), as the
// arrays PxConvexMeshDesc::polygons / indices take (PxHullPolygon records, 16-bit solid-local indices).
//
// Definition (include/surtr_hip.h carries it in full): the faces are the loops Poly::ExtractFaces yields, in its order -- by (start
// vertex, ring slot), each from its smallest vertex.  The plane of a loop is its Newell normal, summed in double in loop order, with
// the offset at mid-range of the loop's own vertices; convexity and planarity are read in double from the FLOAT plane as written.
//
//   k_hl_count    one wave per solid, a lane per vertex in tiles of SURTR_LANES: every half-edge decides with ONE walk whether it leads
//                 its loop (the walk stops at the first smaller vertex; a leader's walk closes and gives the loop's length) -> faces,
//                 entries, longest loop, status and box of the solid.  FEW and LARGE are decided from the counts, before any walk.
//   k_hl_scan     one workgroup: exclusive sums of what will be written, the totals, the capacity check, the header and the records
//   k_hl_emit     as k_hl_count; a __shfl_up scan with a running base across the tiles places the loops in (vertex, slot) order, then
//                 every leader walks its loop once more, serially, to write it and to sum the plane
//   k_hl_errors   a lane per vertex against the planes (every lane reads the same plane: a broadcast load), a lane per loop entry for
//                 the planarity; maxima reduced by shuffles
// A leader test costs O(loop) and every half-edge of the loop makes one: O(loop^2) per face in the worst numbering.  That is fine for
// Convex solids (faces of a few vertices); it is not the way to walk a Mesh.  The kernel boundary between k_hl_emit and k_hl_errors is
// the fence: no lane reads from global memory what another lane stored in the same kernel.  Maxima are order-independent and nothing
// is accumulated with atomics: the same bits whatever the stream, the in-flight hint or the other work.  The context keeps nothing:
// one temporary allocation per call, ordered on the context's stream, and no host synchronisation in the _dev forms.
#include <cmath>
#include <cstring>

#include "surtr_ctx.h"

static_assert(sizeof(surtr_hull_polygon) == 20, "surtr_hull_polygon has PxHullPolygon's layout: 20 bytes");
static_assert(sizeof(surtr_hull) == 48, "surtr_hull is 48 bytes");

#define HL_WG SURTR_WG          // threads of the scan's workgroup (256; one in the emulation)
#define HL_WITHHOLD (SURTR_HULL_FEW | SURTR_HULL_OPEN | SURTR_HULL_IRREGULAR | SURTR_HULL_LARGE)

namespace {

// Where the solids are: the resident Convex set (CSR, loff[v + 1] - loff[v]) or the arena (FragRec offsets, absolute loff + llen).
struct HlSrc
{
    uint32_t frags_on;
    const FragRec* frags; Arena A; const surtr_counts* counts;
    const float* pos; const uint32_t* loff; const int32_t* nbr; const uint32_t* vo; uint32_t n_res;
};
struct HlSolid { const float* pos; const uint32_t* loff; const uint32_t* llen; const int32_t* nbr; uint32_t nv; };

// Scratch of one call (one allocation, carved on the host).
struct HlWork
{
    uint32_t nmax;
    uint32_t* hdr;          // [0] solids [1] the caller's buffers hold everything: emit and errors run
    surtr_hull* rec;        // per solid: what k_hl_count found, then the offsets of k_hl_scan
};

__device__ __forceinline__ uint32_t hl_count(const HlSrc& s) { return s.frags_on ? s.counts->n_frag : s.n_res; }

__device__ HlSolid hl_solid(const HlSrc& s, uint32_t f)
{
    if (!s.frags_on)
    {
        const uint32_t a = s.vo[f];
        return HlSolid{s.pos + 3 * (size_t)a, s.loff + a, nullptr, s.nbr, s.vo[f + 1] - a};
    }
    const FragRec& fr = s.frags[f];
    return HlSolid{s.A.pos + 3 * (size_t)fr.cv_off, s.A.loff + fr.cv_off, s.A.llen + fr.cv_off, s.A.nbr, fr.cv_n};
}
__device__ __forceinline__ uint32_t hl_len(const HlSolid& S, uint32_t v) { return S.llen ? S.llen[v] : S.loff[v + 1] - S.loff[v]; }
__device__ __forceinline__ bool hl_finite(float x) { return fabsf(x) <= 3.4028235e38f; }

// Half-edge (u -> w) -> the vertex after w on its face: the ring entry of w listed just before u (FaceLoop, Src/Poly.cpp:34-41).
// u missing from w's ring (the loop cannot close) sets bad.
__device__ __forceinline__ uint32_t hl_next(const HlSolid& S, uint32_t u, uint32_t w, bool& bad)
{
    const int32_t* r = S.nbr + S.loff[w];
    const uint32_t n = hl_len(S, w);
    if (n == 0u) { bad = true; return 0xFFFFFFFFu; }
    uint32_t k = 0;
    while (k < n && (uint32_t)r[k] != u) ++k;
    if (k == n) bad = true;
    return (uint32_t)r[(k == 0u || k == n) ? n - 1u : k - 1u];
}
// A ring that lists a neighbour twice: the later slot starts no face of its own (ExtractFaces keys by the first slot).
__device__ __forceinline__ bool hl_repeat(const int32_t* r, uint32_t s)
{
    for (uint32_t q = 0; q < s; ++q) if (r[q] == r[s]) return true;
    return false;
}

// Does half-edge (v -> w) lead its loop?  One walk of at most H half-edges: it ends at the first vertex smaller than v (no leader: 0),
// or back on (v -> w) (the loop's length: v is its smallest vertex).  Back at v on another half-edge before either is IRREGULAR
// (ExtractFaces ends its loop there); a link without its way back, an entry that names no vertex, or H steps without an end is OPEN.
__device__ __forceinline__ uint32_t hl_lead(const HlSolid& S, uint32_t v, uint32_t w, uint32_t H, uint32_t& st)
{
    uint32_t prev = v, cur = w;
    for (uint32_t k = 1; k <= H; ++k)
    {
        bool bad = false;
        const uint32_t x = hl_next(S, prev, cur, bad);
        if (bad || x >= S.nv) { st |= SURTR_HULL_OPEN; return 0u; }
        prev = cur; cur = x;
        if (prev == v)
        {
            if (cur == w) return k;
            st |= SURTR_HULL_IRREGULAR;
            return 0u;
        }
        if (prev < v) return 0u;
    }
    st |= SURTR_HULL_OPEN;
    return 0u;
}

struct HlD3 { double x, y, z; };
__device__ __forceinline__ HlD3 hl_pos(const HlSolid& S, uint32_t v)
{
    return HlD3{(double)S.pos[3 * (size_t)v], (double)S.pos[3 * (size_t)v + 1], (double)S.pos[3 * (size_t)v + 2]};
}

// The leader (v -> w) of a loop of k vertices writes it (16-bit, solid-local) and its polygon.  N = sum_{i=1}^{k-2} (q_i - q_0) x
// (q_{i+1} - q_0) in loop order, n = N / |N|, d = -(max t + min t) / 2 over t_i = n . q_i; N == 0: the plane is zero (a flat face).
__device__ void hl_write(const HlSolid& S, uint32_t v, uint32_t w, uint32_t k, uint32_t index_base, surtr_hull_polygon* poly, uint16_t* idx)
{
    const HlD3 q0 = hl_pos(S, v);
    double Nx = 0.0, Ny = 0.0, Nz = 0.0;
    HlD3 a{0.0, 0.0, 0.0};
    uint32_t prev = v, cur = w;
    idx[0] = (uint16_t)v;
    for (uint32_t i = 1; i < k; ++i)
    {
        idx[i] = (uint16_t)cur;
        const HlD3 q = hl_pos(S, cur);
        const HlD3 b{q.x - q0.x, q.y - q0.y, q.z - q0.z};
        if (i >= 2u)
        {
            const double cx = a.y * b.z - a.z * b.y, cy = a.z * b.x - a.x * b.z, cz = a.x * b.y - a.y * b.x;
            Nx = Nx + cx; Ny = Ny + cy; Nz = Nz + cz;
        }
        a = b;
        bool bad = false;
        const uint32_t x = hl_next(S, prev, cur, bad);
        prev = cur; cur = x < S.nv ? x : v;      // (the count kernel walked this loop: x names a vertex)
    }
    surtr_hull_polygon P;
    P.plane[0] = 0.f; P.plane[1] = 0.f; P.plane[2] = 0.f; P.plane[3] = 0.f;
    P.n_verts = (uint16_t)k; P.index_base = (uint16_t)index_base;
    if (Nx != 0.0 || Ny != 0.0 || Nz != 0.0)
    {
        const double len = sqrt((Nx * Nx + Ny * Ny) + Nz * Nz);
        const double nx = Nx / len, ny = Ny / len, nz = Nz / len;
        double tmin = 0.0, tmax = 0.0;
        for (uint32_t i = 0; i < k; ++i)
        {
            const HlD3 q = hl_pos(S, idx[i]);
            const double t = (nx * q.x + ny * q.y) + nz * q.z;
            if (i == 0u) { tmin = t; tmax = t; }
            else { tmin = t < tmin ? t : tmin; tmax = t > tmax ? t : tmax; }
        }
        P.plane[0] = (float)nx; P.plane[1] = (float)ny; P.plane[2] = (float)nz; P.plane[3] = (float)(-(tmax + tmin) / 2.0);
    }
    *poly = P;
}

// Inclusive scan of x over the lanes (lane order); *total = the wave's sum.
__device__ __forceinline__ uint32_t hl_scan_lanes(uint32_t x, uint32_t* total)
{
    const uint32_t l = lane_id();
    for (uint32_t o = 1; o < SURTR_LANES; o <<= 1) { const uint32_t t = __shfl_up(x, o, SURTR_LANES); if (l >= o) x += t; }
    *total = __shfl(x, SURTR_LANES - 1, SURTR_LANES);
    return x;
}
__device__ __forceinline__ uint32_t hl_sum_lanes(uint32_t x)
{
    for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1) x += __shfl_down(x, o, SURTR_LANES);
    return __shfl(x, 0, SURTR_LANES);
}

__global__ __launch_bounds__(SURTR_LANES) void k_hl_count(HlSrc src, HlWork W)
{
    const uint32_t l = lane_id();
    uint32_t n = hl_count(src);
    if (n > W.nmax) n = W.nmax;
    for (uint32_t f = blockIdx.x; f < n; f += gridDim.x)
    {
        const HlSolid S = hl_solid(src, f);
        surtr_hull r;
        memset(&r, 0, sizeof(r));
        r.nv = S.nv;
        // from the counts, before any walk (the same in every lane)
        uint32_t st = S.nv < 4u ? SURTR_HULL_FEW : 0u, H = 0;
        if (S.nv > 65535u) st |= SURTR_HULL_LARGE;
        else
        {
            for (uint32_t v = l; v < S.nv; v += SURTR_LANES) H += hl_len(S, v);
            H = hl_sum_lanes(H);
            if (H > 65535u) st |= SURTR_HULL_LARGE;
        }
        if (st)
        {
            if (S.nv > 255u) st |= SURTR_HULL_OVER_255;
            r.status = st;
            if (l == 0u) W.rec[f] = r;
            continue;
        }
        uint32_t faces = 0, entries = 0, longest = 0;
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        for (uint32_t v = l; v < S.nv; v += SURTR_LANES)
        {
            for (int c = 0; c < 3; ++c)
            {
                const float x = S.pos[3 * (size_t)v + c];
                lo[c] = fminf(lo[c], x); hi[c] = fmaxf(hi[c], x);
                if (!hl_finite(x)) st |= SURTR_HULL_OPEN;
            }
            const int32_t* ring = S.nbr + S.loff[v];
            const uint32_t len = hl_len(S, v);
            for (uint32_t s = 0; s < len; ++s)
            {
                const uint32_t w = (uint32_t)ring[s];
                if (w >= S.nv) { st |= SURTR_HULL_OPEN; continue; }
                if (hl_repeat(ring, s)) { st |= SURTR_HULL_IRREGULAR; continue; }
                const uint32_t k = hl_lead(S, v, w, H, st);
                if (k) { ++faces; entries += k; longest = k > longest ? k : longest; }
            }
        }
        for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1)
        {
            st |= __shfl_down(st, o, SURTR_LANES);
            faces += __shfl_down(faces, o, SURTR_LANES); entries += __shfl_down(entries, o, SURTR_LANES);
            const uint32_t t = __shfl_down(longest, o, SURTR_LANES);
            longest = t > longest ? t : longest;
            for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], __shfl_down(lo[c], o, SURTR_LANES)); hi[c] = fmaxf(hi[c], __shfl_down(hi[c], o, SURTR_LANES)); }
        }
        if (l == 0u)
        {
            if ((H & 1u) || (long long)S.nv - (long long)(H / 2u) + (long long)faces != 2ll) st |= SURTR_HULL_IRREGULAR;
            if (!(st & HL_WITHHOLD))
            {
                r.n_faces = faces; r.n_idx = entries; r.max_loop = longest;
                const float ex = hi[0] - lo[0], ey = hi[1] - lo[1], ez = hi[2] - lo[2];
                r.extent = fmaxf(fmaxf(ex, ey), ez);
            }
            if (S.nv > 255u || r.n_faces > 255u) st |= SURTR_HULL_OVER_255;
            r.status = st;
            W.rec[f] = r;
        }
    }
}

// Exclusive scan of two per-thread values in thread order (thread 0 adds up the group); returns the totals in *ta, *tb.
__device__ void hl_scan_threads(uint32_t& a, uint32_t& b, uint32_t* ta, uint32_t* tb)
{
    __shared__ uint32_t sc[2][HL_WG + 1];
    sc[0][threadIdx.x] = a; sc[1][threadIdx.x] = b;
    __syncthreads();
    if (threadIdx.x == 0u)
        for (int q = 0; q < 2; ++q)
        {
            uint32_t run = 0;
            for (uint32_t t = 0; t < group_size(); ++t) { const uint32_t x = sc[q][t]; sc[q][t] = run; run += x; }
            sc[q][HL_WG] = run;
        }
    __syncthreads();
    a = sc[0][threadIdx.x]; b = sc[1][threadIdx.x];
    *ta = sc[0][HL_WG]; *tb = sc[1][HL_WG];
    __syncthreads();
}

// records_bytes >= 48 (checked on the host): the header is always written; the records only when everything fits.
__global__ __launch_bounds__(HL_WG) void k_hl_scan(HlSrc src, HlWork W, surtr_hull* __restrict__ out, size_t records_bytes, size_t polys_cap, size_t idx_cap)
{
    const uint32_t all = hl_count(src);
    const uint32_t n = all < W.nmax ? all : W.nmax;
    const uint32_t G = group_size(), seg = (n + G - 1u) / G;
    const uint32_t f0 = threadIdx.x * seg < n ? threadIdx.x * seg : n, f1 = f0 + seg < n ? f0 + seg : n;
    uint32_t nf = 0, ni = 0;
    for (uint32_t f = f0; f < f1; ++f) { nf += W.rec[f].n_faces; ni += W.rec[f].n_idx; }
    uint32_t tf = 0, ti = 0;
    hl_scan_threads(nf, ni, &tf, &ti);
    const bool fits = all <= W.nmax && ((size_t)n + 1u) * sizeof(surtr_hull) <= records_bytes && tf <= polys_cap && ti <= idx_cap;
    for (uint32_t f = f0; f < f1; ++f)
    {
        surtr_hull r = W.rec[f];
        r.face_off = nf; r.idx_off = ni;
        nf += r.n_faces; ni += r.n_idx;
        W.rec[f] = r;
        if (fits) out[1u + f] = r;
    }
    if (threadIdx.x == 0u)
    {
        surtr_hull h;
        memset(&h, 0, sizeof(h));
        h.nv = all; h.n_faces = tf; h.n_idx = ti; h.status = fits ? SURTR_OK : SURTR_E_CAPACITY;
        out[0] = h;
        W.hdr[0] = n; W.hdr[1] = fits ? 1u : 0u;
    }
}

__global__ __launch_bounds__(SURTR_LANES) void k_hl_emit(HlSrc src, HlWork W, surtr_hull_polygon* __restrict__ polys, uint16_t* __restrict__ idx)
{
    if (!W.hdr[1]) return;      // a buffer of the caller's is too small: nothing but the header is written
    const uint32_t l = lane_id(), n = W.hdr[0];
    for (uint32_t f = blockIdx.x; f < n; f += gridDim.x)
    {
        const surtr_hull r = W.rec[f];
        if (r.n_faces == 0u) continue;
        const HlSolid S = hl_solid(src, f);
        const uint32_t H = r.n_idx;      // a solid that is not withheld: every half-edge is on one loop that was written
        uint32_t run_f = 0, run_i = 0, unused = 0;
        for (uint32_t v0 = 0; v0 < S.nv; v0 += SURTR_LANES)
        {
            const uint32_t v = v0 + l;
            const int32_t* ring = v < S.nv ? S.nbr + S.loff[v] : nullptr;
            const uint32_t len = v < S.nv ? hl_len(S, v) : 0u;
            uint32_t cnt = 0, ent = 0;
            for (uint32_t s = 0; s < len; ++s) { const uint32_t k = hl_lead(S, v, (uint32_t)ring[s], H, unused); if (k) { ++cnt; ent += k; } }
            uint32_t tot_f = 0, tot_i = 0;
            uint32_t at_f = run_f + hl_scan_lanes(cnt, &tot_f) - cnt, at_i = run_i + hl_scan_lanes(ent, &tot_i) - ent;
            run_f += tot_f; run_i += tot_i;
            for (uint32_t s = 0; s < len && cnt; ++s)
            {
                const uint32_t w = (uint32_t)ring[s], k = hl_lead(S, v, w, H, unused);
                if (!k) continue;
                if (at_f < r.n_faces && at_i + k <= r.n_idx) hl_write(S, v, w, k, at_i, polys + r.face_off + at_f, idx + r.idx_off + at_i);
                ++at_f; at_i += k; --cnt;
            }
        }
    }
}

__global__ __launch_bounds__(SURTR_LANES) void k_hl_errors(HlSrc src, HlWork W, const surtr_hull_polygon* __restrict__ polys, const uint16_t* __restrict__ idx,
                                                           surtr_hull* __restrict__ out)
{
    if (!W.hdr[1]) return;
    const uint32_t l = lane_id(), n = W.hdr[0];
    for (uint32_t f = blockIdx.x; f < n; f += gridDim.x)
    {
        const surtr_hull r = W.rec[f];
        if (r.n_faces == 0u) continue;
        const HlSolid S = hl_solid(src, f);
        const surtr_hull_polygon* P = polys + r.face_off;
        double conv = -INFINITY, plan = 0.0;
        uint32_t flat = 0, solid = 0;
        for (uint32_t v0 = 0; v0 < S.nv; v0 += SURTR_LANES)      // convexity: this lane's vertex against every plane
        {
            const uint32_t v = v0 + l < S.nv ? v0 + l : S.nv - 1u;
            const HlD3 q = hl_pos(S, v);
            for (uint32_t j = 0; j < r.n_faces; ++j)
            {
                const double nx = P[j].plane[0], ny = P[j].plane[1], nz = P[j].plane[2], d = P[j].plane[3];
                if (nx == 0.0 && ny == 0.0 && nz == 0.0) { flat = 1u; continue; }
                solid = 1u;
                const double e = ((nx * q.x + ny * q.y) + nz * q.z) + d;
                conv = e > conv ? e : conv;
            }
        }
        for (uint32_t j = 0; j < r.n_faces; ++j)                 // planarity: the loop's own vertices, a lane per entry
        {
            const double nx = P[j].plane[0], ny = P[j].plane[1], nz = P[j].plane[2], d = P[j].plane[3];
            if (nx == 0.0 && ny == 0.0 && nz == 0.0) continue;
            const uint32_t k = P[j].n_verts;
            const uint16_t* loop = idx + r.idx_off + P[j].index_base;
            for (uint32_t i = l; i < k; i += SURTR_LANES)
            {
                const uint32_t v = loop[i] < S.nv ? loop[i] : 0u;
                const HlD3 q = hl_pos(S, v);
                const double e = fabs(((nx * q.x + ny * q.y) + nz * q.z) + d);
                plan = e > plan ? e : plan;
            }
        }
        for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1)
        {
            const double a = __shfl_down(conv, o, SURTR_LANES), b = __shfl_down(plan, o, SURTR_LANES);
            conv = a > conv ? a : conv; plan = b > plan ? b : plan;
        }
        if (l == 0u)
        {
            out[1u + f].convexity = solid ? (float)conv : 0.f;
            out[1u + f].planarity = (float)plan;
            if (flat) out[1u + f].status = r.status | SURTR_HULL_FLAT;
        }
    }
}

// The call's scratch: one allocation ordered on the stream (the emulation runs everything in program order).
hipError_t hl_alloc(void** p, size_t bytes, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    return hipMallocAsync(p, bytes, st);
#else
    (void)st;
    return hipMalloc(p, bytes);
#endif
}
void hl_free(void* p, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    (void)hipFreeAsync(p, st);
#else
    (void)st;
    (void)hipFree(p);
#endif
}

int hl_launch(surtr_ctx* ctx, const HlSrc& src, uint32_t nmax, void* dev_records, size_t records_bytes, surtr_hull_polygon* dev_polys, size_t polys_cap,
              uint16_t* dev_idx, size_t idx_cap)
{
    hipStream_t st = ctx->stream;
    HlWork W;
    W.nmax = nmax;
    const size_t o_rec = 16, bytes = o_rec + (size_t)std::max(nmax, 1u) * sizeof(surtr_hull);
    char* base = nullptr;
    HIPCHK(hl_alloc((void**)&base, bytes, st));
    W.hdr = (uint32_t*)base; W.rec = (surtr_hull*)(base + o_rec);
    hipError_t e = hipMemsetAsync(W.hdr, 0, 16, st);
    const uint32_t grid = std::max(1u, std::min(nmax, 65536u));
    if (e == hipSuccess)
    {
        PROF_BEGIN(14);
        hipLaunchKernelGGL(k_hl_count, dim3(grid), dim3(SURTR_LANES), 0, st, src, W);
        hipLaunchKernelGGL(k_hl_scan, dim3(1), dim3(HL_WG), 0, st, src, W, (surtr_hull*)dev_records, records_bytes, polys_cap, idx_cap);
        PROF_END(14);
        PROF_BEGIN(15);
        hipLaunchKernelGGL(k_hl_emit, dim3(grid), dim3(SURTR_LANES), 0, st, src, W, dev_polys, dev_idx);
        hipLaunchKernelGGL(k_hl_errors, dim3(grid), dim3(SURTR_LANES), 0, st, src, W, (const surtr_hull_polygon*)dev_polys, (const uint16_t*)dev_idx,
                           (surtr_hull*)dev_records);
        PROF_END(15);
        e = hipGetLastError();
    }
    hl_free(base, st);
    if (e != hipSuccess) { ctx->err = std::string("hulls: ") + hipGetErrorString(e); return SURTR_E_HIP; }
    return SURTR_OK;
}

// No solids: the header alone (zero solids, zero totals, SURTR_OK).
int hl_empty(surtr_ctx* ctx, void* dev_records)
{
    HIPCHK(hipMemsetAsync(dev_records, 0, sizeof(surtr_hull), ctx->stream));
    return SURTR_OK;
}

bool hl_args_ok(const void* dev_records, const void* dev_polys, size_t polys_cap, const void* dev_idx, size_t idx_cap)
{
    return dev_records && (dev_polys || polys_cap == 0) && (dev_idx || idx_cap == 0);
}

} // namespace

extern "C" int surtr_event_hulls_dev(surtr_ctx* ctx, void* dev_records, size_t records_bytes, surtr_hull_polygon* dev_polys, size_t polys_cap,
                                     uint16_t* dev_idx, size_t idx_cap)
{
    if (!ctx || !hl_args_ok(dev_records, dev_polys, polys_cap, dev_idx, idx_cap)) return SURTR_E_INVALID;
    if (!ctx->have_event) return SURTR_E_STATE;
    if (ctx->last_current && ctx->last.status) return SURTR_E_STATE;
    if (records_bytes < sizeof(surtr_hull)) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    HlSrc s;
    memset(&s, 0, sizeof(s));
    s.frags_on = 1u; s.frags = ctx->d_frags; s.A = ctx->arena; s.counts = ctx->d_counts;
    if (ctx->last_current)
    {
        // the host holds this event's counts: a record buffer too small is refused here (the polygons and indices a solid gives are
        // known on the device only; conv_nbrs / 3 polygons and conv_nbrs indices are always enough)
        const surtr_counts& c = ctx->last;
        if (((size_t)c.n_frag + 1u) * sizeof(surtr_hull) > records_bytes) return SURTR_E_CAPACITY;
        if (c.n_frag == 0) return hl_empty(ctx, dev_records);
        return hl_launch(ctx, s, c.n_frag, dev_records, records_bytes, dev_polys, polys_cap, dev_idx, idx_cap);
    }
    // without a synchronisation: the fragment table's capacity bounds the work; the kernels read the fragment count on the device
    return hl_launch(ctx, s, ctx->cap_frags, dev_records, records_bytes, dev_polys, polys_cap, dev_idx, idx_cap);
}

extern "C" int surtr_pieces_hulls_dev(surtr_ctx* ctx, void* dev_records, size_t records_bytes, surtr_hull_polygon* dev_polys, size_t polys_cap,
                                      uint16_t* dev_idx, size_t idx_cap)
{
    if (!ctx || !hl_args_ok(dev_records, dev_polys, polys_cap, dev_idx, idx_cap)) return SURTR_E_INVALID;
    const PieceSet& P = ctx->cset;
    if (!P.pos || !P.vo) return SURTR_E_STATE;
    if (((size_t)ctx->n_pieces + 1u) * sizeof(surtr_hull) > records_bytes) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    if (ctx->n_pieces == 0) return hl_empty(ctx, dev_records);
    HlSrc s;
    memset(&s, 0, sizeof(s));
    s.pos = P.pos; s.loff = P.loff; s.nbr = P.nbr; s.vo = P.vo; s.n_res = ctx->n_pieces;
    return hl_launch(ctx, s, ctx->n_pieces, dev_records, records_bytes, dev_polys, polys_cap, dev_idx, idx_cap);
}

namespace {
// Count-then-fill around a _dev form: device buffers with room for anything `half_edges` ring entries can give (every loop has at
// least one), one download of the header, then of what the caller has room for.
template <class F>
int hl_host(surtr_ctx* ctx, uint32_t n_solids, uint64_t half_edges, uint32_t* n, surtr_hull* records, uint32_t* n_polys, surtr_hull_polygon* polys,
            uint32_t* n_idx, uint16_t* idx, F dev_call)
{
    const bool fill = records && polys && idx;
    if (!fill && (records || polys || idx)) return SURTR_E_INVALID;
    const size_t hcap = (size_t)std::max<uint64_t>(half_edges, 1u);
    DevBuf<surtr_hull> d_rec; DevBuf<surtr_hull_polygon> d_poly; DevBuf<uint16_t> d_idx;
    int rc = d_rec.grow(ctx, (size_t)n_solids + 1u);
    if (rc == SURTR_OK) rc = d_poly.grow(ctx, hcap);
    if (rc == SURTR_OK) rc = d_idx.grow(ctx, hcap);
    if (rc == SURTR_OK) rc = dev_call(d_rec.p, ((size_t)n_solids + 1u) * sizeof(surtr_hull), d_poly.p, hcap, d_idx.p, hcap);
    if (rc) return rc;
    surtr_hull h;
    HIPCHK(hipMemcpyAsync(&h, d_rec.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (h.status) return (int)h.status;
    const bool small = fill && (*n < h.nv || *n_polys < h.n_faces || *n_idx < h.n_idx);
    *n = h.nv; *n_polys = h.n_faces; *n_idx = h.n_idx;
    if (small) return SURTR_E_CAPACITY;
    if (!fill) return SURTR_OK;
    if (h.nv) HIPCHK(hipMemcpyAsync(records, d_rec.p + 1, (size_t)h.nv * sizeof(surtr_hull), hipMemcpyDeviceToHost, ctx->stream));
    if (h.n_faces) HIPCHK(hipMemcpyAsync(polys, d_poly.p, (size_t)h.n_faces * sizeof(surtr_hull_polygon), hipMemcpyDeviceToHost, ctx->stream));
    if (h.n_idx) HIPCHK(hipMemcpyAsync(idx, d_idx.p, (size_t)h.n_idx * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SURTR_OK;
}
} // namespace

extern "C" int surtr_event_hulls(surtr_ctx* ctx, uint32_t* n, surtr_hull* records, uint32_t* n_polys, surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx)
{
    if (!ctx || !n || !n_polys || !n_idx) return SURTR_E_INVALID;
    surtr_counts c;
    if (!ctx->have_event) return SURTR_E_STATE;
    const int rc = surtr_event_counts(ctx, &c);
    if (rc == SURTR_OK && c.status) return SURTR_E_STATE;
    if (rc && ctx->last_current && ctx->last.status) return SURTR_E_STATE;      // (the counts came back: the event itself had failed)
    if (rc) return rc;
    return hl_host(ctx, c.n_frag, c.conv_nbrs, n, records, n_polys, polys, n_idx, idx,
                   [&](void* r, size_t rb, surtr_hull_polygon* p, size_t pc, uint16_t* i, size_t ic) { return surtr_event_hulls_dev(ctx, r, rb, p, pc, i, ic); });
}

extern "C" int surtr_pieces_hulls(surtr_ctx* ctx, uint32_t* n, surtr_hull* records, uint32_t* n_polys, surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx)
{
    if (!ctx || !n || !n_polys || !n_idx) return SURTR_E_INVALID;
    const PieceSet& P = ctx->cset;
    if (!P.pos || !P.vo) return SURTR_E_STATE;
    const uint64_t H = ctx->h_ho[1].size() > ctx->n_pieces ? ctx->h_ho[1][ctx->n_pieces] : 0u;
    return hl_host(ctx, ctx->n_pieces, H, n, records, n_polys, polys, n_idx, idx,
                   [&](void* r, size_t rb, surtr_hull_polygon* p, size_t pc, uint16_t* i, size_t ic) { return surtr_pieces_hulls_dev(ctx, r, rb, p, pc, i, ic); });
}
