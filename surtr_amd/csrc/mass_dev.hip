// mass_dev.hip -- mass, centre of mass and inertia tensor of every fragment of the last event, or of every resident piece, on the
// device: what PxRigidBodyExt::updateMassAndInertia(body, 10.0f) gives InitCompound (Src/Surtr.cpp:2520) per convex shape.
//
// Definition (so that results can be checked exactly): the faces are the loops Poly::ExtractFaces walks on the neighbour rings,
// each fanned around its lowest-numbered vertex; every tetrahedron (vertex 0, fan triangle) adds its volume integrals
// 1, x, y, z, x^2, y^2, z^2, xy, yz, zx, taken relative to the solid's vertex 0 (the origin shift of Poly::Moments,
// Src/Poly.cpp:55-87).  Positions are converted to double first; every product and sum is in double.
//
//   k_ms_plan     one workgroup: chunks of MS_CV vertices per solid (a large solid spreads over many workgroups), scanned
//   k_ms_chunks   one workgroup per chunk: every half-edge walks its face for at most MS_B vertices; closed -> its fan triangle
//                 (anchor = smallest vertex of the loop); longer faces are only counted
//   k_ms_scan     one workgroup: places the half-edges of long faces in a list (chunk order, then vertex, then ring slot)
//   k_ms_collect  chunks with long faces: per half-edge the smallest vertex of its next MS_B and the half-edge MS_B ahead
//   k_ms_long     one workgroup per solid with long faces: pointer jumping over that list (window MS_B * 2^r) until the
//                 windows cover the loops -> every half-edge knows its loop's smallest vertex; its fan triangle
//   k_ms_final    one lane per solid: the chunk partials in chunk order + the long-face partial -> the record
//   k_ms_bodies   surtr_scene_mass: one wave per compound of the scene adds up its pieces' records as surtr_combine_mass does
// Reductions are wave shuffles, then the waves in order, then chunks in order: no atomics on values, so two calls give the same
// bits whatever the stream or the other work on the GPU.  The context keeps nothing: one temporary allocation per call, ordered
// on the context's stream.
#include <cstring>

#include "surtr_ctx.h"

static_assert(sizeof(surtr_mass) == 96, "surtr_mass is 96 bytes");

#define MS_CV 256u      // vertices per chunk (one per thread of a workgroup)
#define MS_B 32u        // faces of up to MS_B vertices are walked; longer ones go through pointer jumping
#define MS_WG SURTR_WG  // threads per workgroup (256; one in the emulation)
#define MS_NT 10        // integrals: 1, x, y, z, xx, yy, zz, xy, yz, zx

namespace {

// Where the solids are: resident set (CSR, loff[v + 1] - loff[v]) or the arena (FragRec offsets, absolute loff + llen).
struct MsSrc
{
    uint32_t frags_on, set;
    const FragRec* frags; Arena A; const surtr_counts* counts;
    const float* pos; const uint32_t* loff; const int32_t* nbr; const uint32_t* vo; uint32_t n_res;
};
struct MsSolid { const float* pos; const uint32_t* loff; const uint32_t* llen; const int32_t* nbr; uint32_t nv; };

// Scratch of one call (one allocation, carved on the host).
struct MsWork
{
    uint32_t nmax, cmax, lmax;
    uint32_t* hdr;          // [0] chunks [1] long half-edges [2] overflow [3] solids [4] output does not fit
    uint32_t* chunk_off;    // nmax + 1
    double* part;           // MS_NT per chunk
    uint32_t* cflag;        // per chunk: a walk met a missing link
    uint32_t* nlong;        // per chunk
    uint32_t* long_off;     // cmax + 1
    double* plong;          // MS_NT per solid
    uint32_t* lflag;        // per solid
    unsigned long long* key; unsigned long long* nxk;      // per long half-edge: (vertex << 32 | slot) and that MS_B ahead
    uint32_t* m0; uint32_t* m1; uint32_t* nx0; uint32_t* nx1;
};

__device__ __forceinline__ uint32_t ms_count(const MsSrc& s) { return s.frags_on ? s.counts->n_frag : s.n_res; }

__device__ MsSolid ms_solid(const MsSrc& s, uint32_t f)
{
    if (!s.frags_on)
    {
        const uint32_t a = s.vo[f];
        return MsSolid{s.pos + 3 * (size_t)a, s.loff + a, nullptr, s.nbr, s.vo[f + 1] - a};
    }
    const FragRec& fr = s.frags[f];
    const uint32_t off = s.set ? fr.cv_off : fr.mv_off, n = s.set ? fr.cv_n : fr.mv_n;
    return MsSolid{s.A.pos + 3 * (size_t)off, s.A.loff + off, s.A.llen + off, s.A.nbr, n};
}
__device__ __forceinline__ uint32_t ms_len(const MsSolid& S, uint32_t v) { return S.llen ? S.llen[v] : S.loff[v + 1] - S.loff[v]; }
__device__ __forceinline__ uint32_t ms_chunks(uint32_t nv) { return nv < 4u ? 0u : (nv + MS_CV - 1u) / MS_CV; }

// Half-edge (u -> w) -> the next one of its face, (w -> x): x is the ring entry of w listed just before u (FaceLoop,
// Src/Poly.cpp:34-41); *slot = its place in w's ring.  u missing from w's ring (the loop cannot close) sets bad.
__device__ __forceinline__ uint32_t ms_next(const MsSolid& S, uint32_t u, uint32_t w, uint32_t* slot, bool& bad)
{
    const int32_t* r = S.nbr + S.loff[w];
    const uint32_t n = ms_len(S, w);
    if (n == 0u) { bad = true; *slot = 0u; return 0xFFFFFFFFu; }
    uint32_t k = 0;
    while (k < n && (uint32_t)r[k] != u) ++k;
    if (k == n) bad = true;
    const uint32_t q = (k == 0u || k == n) ? n - 1u : k - 1u;
    *slot = q;
    return (uint32_t)r[q];
}

// A ring that lists a neighbour twice (a sliver): ExtractFaces keys its visited set by the FIRST slot holding the neighbour, so the
// later slot never starts a face of its own.
__device__ __forceinline__ bool ms_repeat(const int32_t* r, uint32_t s)
{
    for (uint32_t q = 0; q < s; ++q) if (r[q] == r[s]) return true;
    return false;
}

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 ms_rel(const MsSolid& S, uint32_t v)
{
    return D3{(double)S.pos[3 * (size_t)v] - (double)S.pos[0], (double)S.pos[3 * (size_t)v + 1] - (double)S.pos[1],
              (double)S.pos[3 * (size_t)v + 2] - (double)S.pos[2]};
}

// The tetrahedron (vertex 0, a, b, c): 6V = a . (b x c); integrals times 6, 24 and 120 (scaled back in k_ms_final).
__device__ __forceinline__ void ms_tet(const MsSolid& S, uint32_t ia, uint32_t ib, uint32_t ic, double* acc)
{
    const D3 a = ms_rel(S, ia), b = ms_rel(S, ib), c = ms_rel(S, ic);
    const double v6 = a.x * (b.y * c.z - b.z * c.y) + a.y * (b.z * c.x - b.x * c.z) + a.z * (b.x * c.y - b.y * c.x);
    const D3 s{a.x + b.x + c.x, a.y + b.y + c.y, a.z + b.z + c.z};
    acc[0] += v6;
    acc[1] += v6 * s.x; acc[2] += v6 * s.y; acc[3] += v6 * s.z;
    acc[4] += v6 * (a.x * a.x + b.x * b.x + c.x * c.x + s.x * s.x);
    acc[5] += v6 * (a.y * a.y + b.y * b.y + c.y * c.y + s.y * s.y);
    acc[6] += v6 * (a.z * a.z + b.z * b.z + c.z * c.z + s.z * s.z);
    acc[7] += v6 * (a.x * a.y + b.x * b.y + c.x * c.y + s.x * s.y);
    acc[8] += v6 * (a.y * a.z + b.y * b.z + c.y * c.z + s.y * s.z);
    acc[9] += v6 * (a.z * a.x + b.z * b.x + c.z * c.x + s.z * s.x);
}

// Walks the loop of half-edge e0 = (v -> w) for at most MS_B half-edges: true when it came back to e0 (then *m = the smallest
// vertex of the loop); else *m = the smallest source of e0 .. e(MS_B-1) and (*pu -> ring slot *psl of pu) = e(MS_B).  A loop
// that passes a vertex twice is one loop here, as in ExtractFaces when the vertex is not the loop's smallest; when it is, the
// reference's loops all start there and the fans around it are the same triangles.
__device__ __forceinline__ bool ms_walk(const MsSolid& S, uint32_t v, uint32_t w, uint32_t* m, uint32_t* pu, uint32_t* psl, bool& bad)
{
    uint32_t prev = v, cur = w, mn = v, sl = 0;
    for (uint32_t k = 1; k <= MS_B; ++k)
    {
        const uint32_t x = ms_next(S, prev, cur, &sl, bad);
        if (x >= S.nv) { bad = true; *m = mn; return true; }
        prev = cur; cur = x;
        if (prev == v && cur == w) { *m = mn; return true; }
        if (k == MS_B) break;
        mn = prev < mn ? prev : mn;
    }
    *m = mn; *pu = prev; *psl = sl;
    return false;
}

// Sum of MS_NT doubles (+ a flag word and a count) over the workgroup in a fixed order; thread 0 holds the result.
__device__ void ms_reduce(double* acc, uint32_t& flag, uint32_t& cnt)
{
    __shared__ double red[MS_WG / SURTR_LANES + 1][MS_NT];
    __shared__ uint32_t redf[MS_WG / SURTR_LANES + 1][2];
    for (int t = 0; t < MS_NT; ++t)
        for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1) acc[t] += __shfl_down(acc[t], o, SURTR_LANES);
    for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1) { flag |= __shfl_down(flag, o, SURTR_LANES); cnt += __shfl_down(cnt, o, SURTR_LANES); }
    if (lane_id() == 0u)
    {
        for (int t = 0; t < MS_NT; ++t) red[wave_id()][t] = acc[t];
        redf[wave_id()][0] = flag; redf[wave_id()][1] = cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0u)
        for (uint32_t w = 1; w < group_waves(); ++w)
        {
            for (int t = 0; t < MS_NT; ++t) acc[t] += red[w][t];
            flag |= redf[w][0]; cnt += redf[w][1];
        }
    __syncthreads();
}

// Exclusive scan of per-thread values in thread order (thread 0 adds up the group's totals); returns the group total.
__device__ uint32_t ms_scan_threads(uint32_t& v)
{
    __shared__ uint32_t sc[MS_WG + 1];
    sc[threadIdx.x] = v;
    __syncthreads();
    if (threadIdx.x == 0u)
    {
        uint32_t run = 0;
        for (uint32_t t = 0; t < group_size(); ++t) { const uint32_t x = sc[t]; sc[t] = run; run += x; }
        sc[MS_WG] = run;
    }
    __syncthreads();
    v = sc[threadIdx.x];
    const uint32_t tot = sc[MS_WG];
    __syncthreads();
    return tot;
}

__global__ __launch_bounds__(MS_WG) void k_ms_plan(MsSrc src, MsWork W, size_t capacity)
{
    uint32_t n = ms_count(src);
    if (n > W.nmax) { if (threadIdx.x == 0u) W.hdr[2] = 1u; n = W.nmax; }
    const uint32_t G = group_size(), seg = (n + G - 1u) / G;
    const uint32_t f0 = threadIdx.x * seg, f1 = f0 + seg < n ? f0 + seg : n;
    uint32_t tot = 0;
    for (uint32_t f = f0; f < f1; ++f) tot += ms_chunks(ms_solid(src, f).nv);
    uint32_t base = tot;
    const uint32_t all = ms_scan_threads(base);
    for (uint32_t f = f0; f < f1; ++f) { W.chunk_off[f] = base; base += ms_chunks(ms_solid(src, f).nv); }
    if (threadIdx.x == 0u)
    {
        W.chunk_off[n] = all < W.cmax ? all : W.cmax;
        if (all > W.cmax) W.hdr[2] = 1u;
        W.hdr[0] = all < W.cmax ? all : W.cmax;
        W.hdr[3] = n;
        W.hdr[4] = (size_t)n * sizeof(surtr_mass) > capacity ? 1u : 0u;
    }
}

__device__ __forceinline__ uint32_t ms_solid_of(const MsWork& W, uint32_t n, uint32_t c)
{
    uint32_t lo = 0, hi = n;      // last f with chunk_off[f] <= c
    while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (W.chunk_off[mid] <= c) lo = mid; else hi = mid; }
    return lo;
}

__global__ __launch_bounds__(MS_WG) void k_ms_chunks(MsSrc src, MsWork W)
{
    const uint32_t total = W.hdr[0], n = W.hdr[3];
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x)
    {
        const uint32_t f = ms_solid_of(W, n, c);
        const MsSolid S = ms_solid(src, f);
        const uint32_t v0 = (c - W.chunk_off[f]) * MS_CV, v1 = v0 + MS_CV < S.nv ? v0 + MS_CV : S.nv;
        double acc[MS_NT] = {};
        bool bad = false;
        uint32_t nl = 0;
        for (uint32_t v = v0 + threadIdx.x; v < v1; v += group_size())
        {
            const int32_t* r = S.nbr + S.loff[v];
            const uint32_t len = ms_len(S, v);
            for (uint32_t s = 0; s < len; ++s)
            {
                const uint32_t w = (uint32_t)r[s];
                if (w >= S.nv) { bad = true; continue; }
                if (ms_repeat(r, s)) continue;
                uint32_t m, pu, psl;
                if (!ms_walk(S, v, w, &m, &pu, &psl, bad)) { ++nl; continue; }
                if (v != m && w != m) ms_tet(S, m, v, w, acc);
            }
        }
        uint32_t flag = bad ? 1u : 0u;
        ms_reduce(acc, flag, nl);
        if (threadIdx.x == 0u)
        {
            for (int t = 0; t < MS_NT; ++t) W.part[(size_t)c * MS_NT + t] = acc[t];
            W.cflag[c] = flag; W.nlong[c] = nl;
        }
    }
}

__global__ __launch_bounds__(MS_WG) void k_ms_scan(MsWork W)
{
    const uint32_t T = W.hdr[0], G = group_size(), seg = (T + G - 1u) / G;
    const uint32_t c0 = threadIdx.x * seg, c1 = c0 + seg < T ? c0 + seg : T;
    uint32_t tot = 0;
    for (uint32_t c = c0; c < c1; ++c) tot += W.nlong[c];
    uint32_t base = tot;
    const uint32_t all = ms_scan_threads(base);
    for (uint32_t c = c0; c < c1; ++c) { W.long_off[c] = base; base += W.nlong[c]; }
    if (threadIdx.x == 0u)
    {
        W.long_off[T] = all;
        W.hdr[1] = all;
        if (all > W.lmax) W.hdr[2] = 1u;
    }
}

__global__ __launch_bounds__(MS_WG) void k_ms_collect(MsSrc src, MsWork W)
{
    const uint32_t total = W.hdr[0], n = W.hdr[3];
    if (W.hdr[1] > W.lmax) return;
    for (uint32_t c = blockIdx.x; c < total; c += gridDim.x)
    {
        if (W.nlong[c] == 0u) continue;
        const uint32_t f = ms_solid_of(W, n, c);
        const MsSolid S = ms_solid(src, f);
        const uint32_t v0 = (c - W.chunk_off[f]) * MS_CV, v1 = v0 + MS_CV < S.nv ? v0 + MS_CV : S.nv;
        bool bad = false;
        uint32_t mine = 0;
        for (int pass = 0; pass < 2; ++pass)
        {
            uint32_t at = mine;
            for (uint32_t v = v0 + threadIdx.x; v < v1; v += group_size())
            {
                const int32_t* r = S.nbr + S.loff[v];
                const uint32_t len = ms_len(S, v);
                for (uint32_t s = 0; s < len; ++s)
                {
                    const uint32_t w = (uint32_t)r[s];
                    if (w >= S.nv || ms_repeat(r, s)) continue;
                    uint32_t m, pu, psl;
                    if (ms_walk(S, v, w, &m, &pu, &psl, bad)) continue;
                    if (pass == 1)
                    {
                        const int32_t* rp = S.nbr + S.loff[pu];
                        uint32_t q = 0;
                        while (rp[q] != rp[psl]) ++q;          // the first slot holding that neighbour (the one listed)
                        const uint32_t i = W.long_off[c] + at;
                        W.key[i] = ((unsigned long long)v << 32) | s;
                        W.nxk[i] = ((unsigned long long)pu << 32) | q;
                        W.m0[i] = m;
                    }
                    ++at;
                }
            }
            if (pass == 0) { mine = at; ms_scan_threads(mine); }
        }
    }
}

__global__ __launch_bounds__(MS_WG) void k_ms_long(MsSrc src, MsWork W)
{
    const uint32_t n = W.hdr[3];
    const bool ok = W.hdr[1] <= W.lmax;
    for (uint32_t f = blockIdx.x; f < n; f += gridDim.x)
    {
        const uint32_t ls = ok ? W.long_off[W.chunk_off[f]] : 0u, le = ok ? W.long_off[W.chunk_off[f + 1]] : 0u;
        double acc[MS_NT] = {};
        bool bad = false;
        if (le > ls)
        {
            const MsSolid S = ms_solid(src, f);
            for (uint32_t i = ls + threadIdx.x; i < le; i += group_size())
            {
                uint32_t lo = ls, hi = le;      // keys ascend (chunk, vertex, slot order): binary search
                const unsigned long long k = W.nxk[i];
                while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (W.key[mid] <= k) lo = mid; else hi = mid; }
                if (W.key[lo] == k) W.nx0[i] = lo;
                else { W.nx0[i] = i; bad = true; }
            }
            __syncthreads();
            uint32_t *mc = W.m0, *mn = W.m1, *xc = W.nx0, *xn = W.nx1;
            for (uint32_t win = MS_B; win < le - ls; win <<= 1)
            {
                for (uint32_t i = ls + threadIdx.x; i < le; i += group_size())
                {
                    const uint32_t t = xc[i], a = mc[i], b = mc[t];
                    mn[i] = a < b ? a : b;
                    xn[i] = xc[t];
                }
                __syncthreads();
                uint32_t* t1 = mc; mc = mn; mn = t1; t1 = xc; xc = xn; xn = t1;
            }
            for (uint32_t i = ls + threadIdx.x; i < le; i += group_size())
            {
                const uint32_t v = (uint32_t)(W.key[i] >> 32), s = (uint32_t)W.key[i];
                const uint32_t w = (uint32_t)(S.nbr + S.loff[v])[s], m = mc[i];
                if (v != m && w != m) ms_tet(S, m, v, w, acc);
            }
        }
        uint32_t flag = bad ? 1u : 0u, dummy = 0;
        ms_reduce(acc, flag, dummy);
        if (threadIdx.x == 0u)
        {
            for (int t = 0; t < MS_NT; ++t) W.plong[(size_t)f * MS_NT + t] = acc[t];
            W.lflag[f] = flag;
        }
    }
}

__global__ __launch_bounds__(MS_WG) void k_ms_final(MsSrc src, MsWork W, double rho, surtr_mass* __restrict__ out)
{
    const uint32_t n = W.hdr[3];
    if (W.hdr[4]) return;      // the caller's buffer is too small: nothing is written
    for (uint32_t f = blockIdx.x * blockDim.x + threadIdx.x; f < n; f += gridDim.x * blockDim.x)
    {
        const MsSolid S = ms_solid(src, f);
        surtr_mass r;
        memset(&r, 0, sizeof(r));
        r.nv = S.nv;
        if (S.nv < 4u) { r.status = 1u; out[f] = r; continue; }
        double J[MS_NT] = {};
        uint32_t bad = W.hdr[2];
        for (uint32_t c = W.chunk_off[f]; c < W.chunk_off[f + 1]; ++c)
        {
            for (int t = 0; t < MS_NT; ++t) J[t] += W.part[(size_t)c * MS_NT + t];
            bad |= W.cflag[c];
        }
        for (int t = 0; t < MS_NT; ++t) J[t] += W.plong[(size_t)f * MS_NT + t];
        bad |= W.lflag[f];
        const double vol = J[0] / 6.0;
        r.volume = vol; r.mass = rho * vol;
        const D3 o{(double)S.pos[0], (double)S.pos[1], (double)S.pos[2]};
        if (vol != 0.0)
        {
            const double cx = J[1] / 24.0 / vol, cy = J[2] / 24.0 / vol, cz = J[3] / 24.0 / vol;
            // second moments about the centre of mass: int (x - c)(y - c) = int xy - V cx cy
            const double xx = J[4] / 120.0 - vol * cx * cx, yy = J[5] / 120.0 - vol * cy * cy, zz = J[6] / 120.0 - vol * cz * cz;
            const double xy = J[7] / 120.0 - vol * cx * cy, yz = J[8] / 120.0 - vol * cy * cz, zx = J[9] / 120.0 - vol * cz * cx;
            r.com[0] = o.x + cx; r.com[1] = o.y + cy; r.com[2] = o.z + cz;
            r.inertia[0] = rho * (yy + zz); r.inertia[1] = rho * (xx + zz); r.inertia[2] = rho * (xx + yy);
            r.inertia[3] = -rho * xy; r.inertia[4] = -rho * yz; r.inertia[5] = -rho * zx;
        }
        else { r.com[0] = o.x; r.com[1] = o.y; r.com[2] = o.z; }
        r.status = bad ? 3u : (vol <= 0.0 ? 2u : 0u);
        out[f] = r;
    }
}

// The call's scratch: one allocation ordered on the stream (the emulation runs everything in program order).
hipError_t ms_alloc(void** p, size_t bytes, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    return hipMallocAsync(p, bytes, st);
#else
    (void)st;
    return hipMalloc(p, bytes);
#endif
}
void ms_free(void* p, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    (void)hipFreeAsync(p, st);
#else
    (void)st;
    (void)hipFree(p);
#endif
}

int ms_launch(surtr_ctx* ctx, const MsSrc& src, uint32_t nmax, uint64_t vmax, uint64_t hmax, float density, void* dev_out, size_t capacity)
{
    hipStream_t st = ctx->stream;
    MsWork W;
    W.nmax = nmax;
    W.cmax = (uint32_t)std::min<uint64_t>(0xFFFFFFF0ull, (uint64_t)nmax + vmax / MS_CV + 1u);
    W.lmax = (uint32_t)std::min<uint64_t>(0xFFFFFFF0ull, hmax + 1u);
    size_t bytes = 0;
    auto take = [&](size_t b) { const size_t at = bytes; bytes += (b + 15u) & ~(size_t)15u; return at; };
    const size_t o_hdr = take(8 * 4), o_coff = take(((size_t)nmax + 1) * 4), o_part = take((size_t)W.cmax * MS_NT * 8),
                 o_cflag = take((size_t)W.cmax * 4), o_nlong = take((size_t)W.cmax * 4), o_loff = take(((size_t)W.cmax + 1) * 4),
                 o_plong = take((size_t)nmax * MS_NT * 8 + 8), o_lflag = take((size_t)nmax * 4 + 4), o_key = take((size_t)W.lmax * 8),
                 o_nxk = take((size_t)W.lmax * 8), o_m0 = take((size_t)W.lmax * 4), o_m1 = take((size_t)W.lmax * 4),
                 o_nx0 = take((size_t)W.lmax * 4), o_nx1 = take((size_t)W.lmax * 4);
    char* base = nullptr;
    HIPCHK(ms_alloc((void**)&base, bytes, st));
    W.hdr = (uint32_t*)(base + o_hdr); W.chunk_off = (uint32_t*)(base + o_coff); W.part = (double*)(base + o_part);
    W.cflag = (uint32_t*)(base + o_cflag); W.nlong = (uint32_t*)(base + o_nlong); W.long_off = (uint32_t*)(base + o_loff);
    W.plong = (double*)(base + o_plong); W.lflag = (uint32_t*)(base + o_lflag); W.key = (unsigned long long*)(base + o_key);
    W.nxk = (unsigned long long*)(base + o_nxk); W.m0 = (uint32_t*)(base + o_m0); W.m1 = (uint32_t*)(base + o_m1);
    W.nx0 = (uint32_t*)(base + o_nx0); W.nx1 = (uint32_t*)(base + o_nx1);
    hipError_t e = hipMemsetAsync(W.hdr, 0, 32, st);
    // grids from the host's bound on the solids (the event's fragment count when the host holds it); the kernels stride
    const uint32_t g_chunks = std::max(1u, std::min(W.cmax, 4096u)), g_solids = std::max(1u, std::min(nmax, 2048u));
    const uint32_t g_final = std::max(1u, std::min((nmax + MS_WG - 1u) / MS_WG, 1024u));
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(k_ms_plan, dim3(1), dim3(MS_WG), 0, st, src, W, capacity);
        hipLaunchKernelGGL(k_ms_chunks, dim3(g_chunks), dim3(MS_WG), 0, st, src, W);
        hipLaunchKernelGGL(k_ms_scan, dim3(1), dim3(MS_WG), 0, st, W);
        hipLaunchKernelGGL(k_ms_collect, dim3(g_chunks), dim3(MS_WG), 0, st, src, W);
        hipLaunchKernelGGL(k_ms_long, dim3(g_solids), dim3(MS_WG), 0, st, src, W);
        hipLaunchKernelGGL(k_ms_final, dim3(g_final), dim3(MS_WG), 0, st, src, W, (double)density, (surtr_mass*)dev_out);
        e = hipGetLastError();
    }
    ms_free(base, st);
    if (e != hipSuccess) { ctx->err = std::string("mass: ") + hipGetErrorString(e); return SURTR_E_HIP; }
    return SURTR_OK;
}

// The record of every compound of the scene from those of its pieces: surtr_combine_mass on the device, bit for bit.  The additions
// are a chain in piece order, so one lane makes them; the wave's part is to bring the records in, MS_STAGE at a time through LDS with
// coalesced loads (a record is twelve 8-byte words), once for the sums and once more for the inertia about the centre they give.
#define MS_STAGE 64u
__global__ __launch_bounds__(SURTR_LANES) void k_ms_bodies(SceneDev sc, const surtr_mass* __restrict__ rec, surtr_mass* __restrict__ out)
{
    __shared__ unsigned long long stage[MS_STAGE * 12u];
    const uint32_t l = lane_id();
    const unsigned long long* words = (const unsigned long long*)rec;
    for (uint32_t c = blockIdx.x; c < sc.n_comp; c += gridDim.x)
    {
        const uint32_t p0 = sc.comp_off[c], p1 = sc.comp_off[c + 1];
        bool heavy = false;
        for (uint32_t p = p0 + l; p < p1; p += SURTR_LANES) heavy = heavy || rec[p].mass != 0.0;
        const bool by_volume = __ballot(heavy) == 0ull;
        surtr_mass r;
        memset(&r, 0, sizeof(r));
        double m = 0.0, w = 0.0, cx = 0.0, cy = 0.0, cz = 0.0;
        for (int pass = 0; pass < 2; ++pass)
        {
            for (uint32_t k0 = p0; k0 < p1; k0 += MS_STAGE)
            {
                const uint32_t cnt = p1 - k0 < MS_STAGE ? p1 - k0 : MS_STAGE;
                for (uint32_t i = l; i < 12u * cnt; i += SURTR_LANES) stage[i] = words[12 * (size_t)k0 + i];
                __syncthreads();
                if (l == 0u)
                    for (uint32_t k = 0; k < cnt; ++k)
                    {
                        surtr_mass p;
                        memcpy(&p, stage + 12u * k, sizeof(p));
                        if (pass == 0)
                        {
                            r.volume += p.volume; m += p.mass; r.nv += p.nv;
                            if (p.status > r.status) r.status = p.status;
                            const double wp = by_volume ? p.volume : p.mass;
                            w += wp; cx += wp * p.com[0]; cy += wp * p.com[1]; cz += wp * p.com[2];
                        }
                        else
                        {
                            const double dx = p.com[0] - r.com[0], dy = p.com[1] - r.com[1], dz = p.com[2] - r.com[2];
                            r.inertia[0] += p.inertia[0] + p.mass * (dy * dy + dz * dz);
                            r.inertia[1] += p.inertia[1] + p.mass * (dx * dx + dz * dz);
                            r.inertia[2] += p.inertia[2] + p.mass * (dx * dx + dy * dy);
                            r.inertia[3] += p.inertia[3] - p.mass * dx * dy;
                            r.inertia[4] += p.inertia[4] - p.mass * dy * dz;
                            r.inertia[5] += p.inertia[5] - p.mass * dz * dx;
                        }
                    }
                __syncthreads();
            }
            if (pass == 0)
            {
                r.mass = m;
                if (w != 0.0) { r.com[0] = cx / w; r.com[1] = cy / w; r.com[2] = cz / w; }
            }
        }
        if (r.status == 0u && r.volume <= 0.0) r.status = 2u;
        if (l == 0u) out[c] = r;
    }
}

MsSrc ms_pieces_src(surtr_ctx* ctx, int set)
{
    const PieceSet& P = set ? ctx->cset : ctx->mset;
    MsSrc s;
    memset(&s, 0, sizeof(s));
    s.frags_on = 0u; s.set = (uint32_t)set; s.pos = P.pos; s.loff = P.loff; s.nbr = P.nbr; s.vo = P.vo; s.n_res = ctx->n_pieces;
    return s;
}

} // namespace

extern "C" int surtr_event_mass_dev(surtr_ctx* ctx, int set, float density, void* dev_out, size_t capacity_bytes)
{
    if (!ctx || !dev_out || (set != 0 && set != 1)) return SURTR_E_INVALID;
    if (!ctx->have_event) return SURTR_E_STATE;
    (void)hipSetDevice(ctx->device);
    MsSrc s;
    memset(&s, 0, sizeof(s));
    s.frags_on = 1u; s.set = (uint32_t)set; s.frags = ctx->d_frags; s.A = ctx->arena; s.counts = ctx->d_counts;
    if (ctx->last_current)
    {
        // the host holds this event's counts: exact bounds, and a buffer too small is refused here
        const surtr_counts& c = ctx->last;
        if (c.status) return SURTR_E_STATE;
        if ((size_t)c.n_frag * sizeof(surtr_mass) > capacity_bytes) return SURTR_E_CAPACITY;
        if (c.n_frag == 0) return SURTR_OK;
        return ms_launch(ctx, s, c.n_frag, set ? c.conv_verts : c.mesh_verts, set ? c.conv_nbrs : c.mesh_nbrs, density, dev_out, capacity_bytes);
    }
    // without a synchronisation: the arena's capacities bound the work; the kernels read the fragment count on the device
    return ms_launch(ctx, s, ctx->cap_frags, ctx->arena.capV, ctx->arena.capH, density, dev_out, capacity_bytes);
}

extern "C" int surtr_pieces_mass_dev(surtr_ctx* ctx, int set, float density, void* dev_out, size_t capacity_bytes)
{
    if (!ctx || !dev_out || (set != 0 && set != 1)) return SURTR_E_INVALID;
    const PieceSet& P = set ? ctx->cset : ctx->mset;
    if (!P.pos || !P.vo) return SURTR_E_STATE;
    if ((size_t)ctx->n_pieces * sizeof(surtr_mass) > capacity_bytes) return SURTR_E_CAPACITY;
    if (ctx->n_pieces == 0) return SURTR_OK;
    (void)hipSetDevice(ctx->device);
    return ms_launch(ctx, ms_pieces_src(ctx, set), ctx->n_pieces, P.pos.cap / 3u, P.nbr.cap, density, dev_out, capacity_bytes);
}

// One record per compound of the scene, in the resident (body) frame: the pieces' records into one temporary allocation ordered on
// the stream, then k_ms_bodies.  No host synchronisation.
extern "C" int surtr_scene_mass_dev(surtr_ctx* ctx, int set, float density, void* dev_out, size_t capacity_bytes)
{
    if (!ctx || !dev_out || (set != 0 && set != 1)) return SURTR_E_INVALID;
    const PieceSet& P = set ? ctx->cset : ctx->mset;
    if (!P.pos || !P.vo || ctx->n_pieces == 0 || ctx->scene_off.size() < 2) return SURTR_E_STATE;
    const uint32_t nc = (uint32_t)ctx->scene_off.size() - 1u, n = ctx->n_pieces;
    if ((size_t)nc * sizeof(surtr_mass) > capacity_bytes) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    SceneDev sc;
    int rc = scene_sync_device(ctx, &sc);
    if (rc) return rc;
    surtr_mass* rec = nullptr;
    HIPCHK(ms_alloc((void**)&rec, (size_t)n * sizeof(surtr_mass), ctx->stream));
    rc = ms_launch(ctx, ms_pieces_src(ctx, set), n, P.pos.cap / 3u, P.nbr.cap, density, rec, (size_t)n * sizeof(surtr_mass));
    hipError_t e = hipSuccess;
    if (rc == SURTR_OK)
    {
        hipLaunchKernelGGL(k_ms_bodies, dim3(std::min(nc, 65536u)), dim3(SURTR_LANES), 0, ctx->stream, sc, rec, (surtr_mass*)dev_out);
        e = hipGetLastError();
    }
    ms_free(rec, ctx->stream);
    if (e != hipSuccess) { ctx->err = std::string("scene mass: ") + hipGetErrorString(e); return SURTR_E_HIP; }
    return rc;
}

namespace {
template <class F>
int ms_host(surtr_ctx* ctx, uint32_t n, surtr_mass* out, F dev_call)
{
    if (!out || n == 0) return SURTR_OK;
    DevBuf<surtr_mass> d;
    int rc = d.grow(ctx, n);
    if (rc == SURTR_OK) rc = dev_call(d.p, (size_t)n * sizeof(surtr_mass));
    if (rc == SURTR_OK && hipMemcpyAsync(out, d, (size_t)n * sizeof(surtr_mass), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    if (rc == SURTR_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    return rc;
}
} // namespace

extern "C" int surtr_event_mass(surtr_ctx* ctx, int set, float density, uint32_t* n, surtr_mass* out)
{
    if (!ctx || !n || (set != 0 && set != 1)) return SURTR_E_INVALID;
    surtr_counts c;
    const int rc = surtr_event_counts(ctx, &c);
    if (rc) return rc;
    if (out && *n < c.n_frag) { *n = c.n_frag; return SURTR_E_CAPACITY; }
    *n = c.n_frag;
    return ms_host(ctx, c.n_frag, out, [&](void* d, size_t b) { return surtr_event_mass_dev(ctx, set, density, d, b); });
}

extern "C" int surtr_pieces_mass(surtr_ctx* ctx, int set, float density, uint32_t* n, surtr_mass* out)
{
    if (!ctx || !n || (set != 0 && set != 1)) return SURTR_E_INVALID;
    const PieceSet& P = set ? ctx->cset : ctx->mset;
    if (!P.pos || !P.vo) return SURTR_E_STATE;
    if (out && *n < ctx->n_pieces) { *n = ctx->n_pieces; return SURTR_E_CAPACITY; }
    *n = ctx->n_pieces;
    return ms_host(ctx, ctx->n_pieces, out, [&](void* d, size_t b) { return surtr_pieces_mass_dev(ctx, set, density, d, b); });
}

// Parallel-axis theorem over the pieces of every compound (host, O(pieces)).
extern "C" int surtr_combine_mass(uint32_t n_compounds, const uint32_t* compound_off, const int32_t* compound_piece,
                                  const surtr_mass* pieces, surtr_mass* out)
{
    if (!compound_off || !compound_piece || !pieces || !out) return SURTR_E_INVALID;
    for (uint32_t c = 0; c < n_compounds; ++c)
        for (uint32_t k = compound_off[c]; k < compound_off[c + 1]; ++k)
            if (compound_piece[k] < 0) return SURTR_E_INVALID;
    for (uint32_t c = 0; c < n_compounds; ++c)
    {
        surtr_mass r;
        memset(&r, 0, sizeof(r));
        double m = 0.0, w = 0.0, cx = 0.0, cy = 0.0, cz = 0.0;
        bool by_volume = true;
        for (uint32_t k = compound_off[c]; k < compound_off[c + 1]; ++k) if (pieces[compound_piece[k]].mass != 0.0) by_volume = false;
        for (uint32_t k = compound_off[c]; k < compound_off[c + 1]; ++k)
        {
            const surtr_mass& p = pieces[compound_piece[k]];
            r.volume += p.volume; m += p.mass; r.nv += p.nv;
            if (p.status > r.status) r.status = p.status;
            const double wp = by_volume ? p.volume : p.mass;
            w += wp; cx += wp * p.com[0]; cy += wp * p.com[1]; cz += wp * p.com[2];
        }
        r.mass = m;
        if (w != 0.0) { r.com[0] = cx / w; r.com[1] = cy / w; r.com[2] = cz / w; }
        for (uint32_t k = compound_off[c]; k < compound_off[c + 1]; ++k)
        {
            const surtr_mass& p = pieces[compound_piece[k]];
            const double dx = p.com[0] - r.com[0], dy = p.com[1] - r.com[1], dz = p.com[2] - r.com[2];
            r.inertia[0] += p.inertia[0] + p.mass * (dy * dy + dz * dz);
            r.inertia[1] += p.inertia[1] + p.mass * (dx * dx + dz * dz);
            r.inertia[2] += p.inertia[2] + p.mass * (dx * dx + dy * dy);
            r.inertia[3] += p.inertia[3] - p.mass * dx * dy;
            r.inertia[4] += p.inertia[4] - p.mass * dy * dz;
            r.inertia[5] += p.inertia[5] - p.mass * dz * dx;
        }
        if (r.status == 0u && r.volume <= 0.0) r.status = 2u;
        out[c] = r;
    }
    return SURTR_OK;
}

extern "C" int surtr_scene_mass(surtr_ctx* ctx, int set, float density, uint32_t* n, surtr_mass* out)
{
    if (!ctx || !n || (set != 0 && set != 1)) return SURTR_E_INVALID;
    const PieceSet& P = set ? ctx->cset : ctx->mset;
    if (!P.pos || !P.vo || ctx->n_pieces == 0 || ctx->scene_off.size() < 2) return SURTR_E_STATE;
    const uint32_t nc = (uint32_t)ctx->scene_off.size() - 1u;
    if (out && *n < nc) { *n = nc; return SURTR_E_CAPACITY; }
    *n = nc;
    return ms_host(ctx, nc, out, [&](void* d, size_t b) { return surtr_scene_mass_dev(ctx, set, density, d, b); });
}
