// cook_dev.hip -- cooked hulls: per selected solid, weld the points of a Convex, build their convex hull and merge coplanar triangles
// into polygons, on the device: what CookingConvex (Src/Surtr.cpp:2531-2553) asks of PhysX (eWELD_VERTICES, eCOMPUTE_CONVEX,
// planeTolerance 7e-6), for the solids whose ring hull (hull_dev.hip) surtr::HullUsable refuses.  include/surtr_hip.h carries the
// definition in full; every number below is computed in double, one operation at a time.
//
//   k_ck_build<false>  one wave per solid: the whole build in LDS, only the record (counts, status) leaves
//   k_ck_scan          one workgroup: exclusive sums of what will be written, totals, capacity check, header and records
//   k_ck_build<true>   the same build once more (it is deterministic), then the compact emit and the two errors
// Inside the build the lanes share the loops over points (weld test, start simplex, farthest point, final convexity) and over
// triangles or faces (visibility, planes, ranks, the edge check); the horizon walk, the fan, the merge and the loop compaction run on
// lane 0 over the tables in LDS.  No atomics, plain stores to disjoint ranges, maxima with ties to the lowest index: the same bits
// whatever the stream, the in-flight hint or the batch.  The context keeps nothing: one temporary allocation per call, ordered on the
// context's stream.
#include <cmath>
#include <cstring>

#include "surtr_ctx.h"

static_assert(sizeof(surtr_cooked) == 64, "surtr_cooked is 64 bytes");

// LDS of one solid (DESIGN 3.25 has the sum): 320 kept points, 2 V - 4 = 636 triangles of 3 + 3 16-bit entries and a double plane,
// two index buffers of 3 * 640 entries.  57 KB of the 64 KB a workgroup gets without opt-in.
#define CK_MAXV 320u
#define CK_MAXT 640u
#define CK_MAXI 1920u
#define CK_NONE 0xFFFFu
#define CK_WG SURTR_WG
#define CK_WITHHOLD (SURTR_COOK_SKIPPED | SURTR_COOK_FEW | SURTR_COOK_DEGENERATE | SURTR_COOK_NONFINITE | SURTR_COOK_LARGE | SURTR_COOK_FAILED)
#define CK_HULL_UNUSABLE (SURTR_HULL_FEW | SURTR_HULL_OPEN | SURTR_HULL_IRREGULAR | SURTR_HULL_LARGE | SURTR_HULL_FLAT)

namespace {

// Where the solids are: the arena (FragRec offsets) or a CSR point set (the resident Convex set, or uploaded points).
struct CkSrc
{
    uint32_t frags_on;
    const FragRec* frags; const float* apos; const surtr_counts* counts;
    const float* pos; const uint32_t* vo; uint32_t n_res;
};
struct CkSolid { const float* pos; uint32_t nv; };
struct CkPar { const surtr_hull* hulls; float rel_tol; double weld2, tol; };
struct CkWork
{
    uint32_t nmax;
    uint32_t* hdr;          // [0] solids [1] everything fits: the emit runs [2] the hull records do not belong to these solids
    surtr_cooked* rec;
};
struct CkLds
{
    union
    {
        double tp[CK_MAXT][4];                  // triangle planes, until the merge is done
        float fp[CK_MAXT][4];                   // then the float planes of the faces
    };
    float pos[3 * CK_MAXV];                     // kept points
    uint32_t key[CK_MAXT];
    uint32_t sh[8];                             // words lane 0 hands to the wave
    uint16_t ksrc[CK_MAXV], newid[CK_MAXV], deg[CK_MAXV], mark[CK_MAXV];
    uint16_t tv[CK_MAXT][3], ta[CK_MAXT][3];    // vertices (counter-clockwise from outside); ta[t][k]: across edge tv[t][k] -> tv[t][k + 1]
    uint16_t cls[CK_MAXT], lnk[CK_MAXT], tail[CK_MAXT];
    uint16_t ha[CK_MAXV], ho[CK_MAXV], vl[CK_MAXT];
    uint16_t ia[CK_MAXI], ib[CK_MAXI];
    uint16_t fs[CK_MAXT], fl[CK_MAXT], fo[CK_MAXT], fb[CK_MAXT];
    uint8_t vis[CK_MAXT], used[CK_MAXV];
};
static_assert(sizeof(CkLds) <= 65536, "one solid's tables fit the LDS a workgroup gets without opt-in");

struct CkD3 { double x, y, z; };

__device__ __forceinline__ uint32_t ck_count(const CkSrc& s) { return s.frags_on ? s.counts->n_frag : s.n_res; }
__device__ __forceinline__ CkSolid ck_solid(const CkSrc& s, uint32_t f)
{
    if (!s.frags_on) { const uint32_t a = s.vo[f]; return CkSolid{s.pos + 3 * (size_t)a, s.vo[f + 1] - a}; }
    const FragRec& fr = s.frags[f];
    return CkSolid{s.apos + 3 * (size_t)fr.cv_off, fr.cv_n};
}
__device__ __forceinline__ bool ck_finite(float x) { return fabsf(x) <= 3.4028235e38f; }
__device__ __forceinline__ CkD3 ck_in(const CkSolid& S, uint32_t v)
{
    return CkD3{(double)S.pos[3 * (size_t)v], (double)S.pos[3 * (size_t)v + 1], (double)S.pos[3 * (size_t)v + 2]};
}
__device__ __forceinline__ CkD3 ck_kept(const CkLds& L, uint32_t i) { return CkD3{(double)L.pos[3 * i], (double)L.pos[3 * i + 1], (double)L.pos[3 * i + 2]}; }
__device__ __forceinline__ CkD3 ck_sub(const CkD3& a, const CkD3& b) { return CkD3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ CkD3 ck_cross(const CkD3& a, const CkD3& b) { return CkD3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ double ck_dot(const CkD3& a, const CkD3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__device__ __forceinline__ double ck_dist(const double* pl, const CkD3& q) { return ((pl[0] * q.x + pl[1] * q.y) + pl[2] * q.z) + pl[3]; }
__device__ __forceinline__ bool ck_usable(const surtr_hull& h, float rel_tol)
{
    if (h.status & CK_HULL_UNUSABLE) return false;
    const float tol = rel_tol * h.extent;
    return h.convexity <= tol && h.planarity <= tol;
}

// wave reductions; every lane gets the result
__device__ __forceinline__ uint32_t ck_or(uint32_t x)
{
    for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1) x |= __shfl_down(x, o, SURTR_LANES);
    return __shfl(x, 0, SURTR_LANES);
}
__device__ __forceinline__ double ck_max(double x)
{
    for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1) { const double t = __shfl_down(x, o, SURTR_LANES); x = t > x ? t : x; }
    return __shfl(x, 0, SURTR_LANES);
}
// the largest value, ties to the lowest index
__device__ __forceinline__ void ck_argmax(double& v, uint32_t& i)
{
    for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1)
    {
        const double tv = __shfl_down(v, o, SURTR_LANES);
        const uint32_t ti = __shfl_down(i, o, SURTR_LANES);
        if (tv > v || (tv == v && ti < i)) { v = tv; i = ti; }
    }
    v = __shfl(v, 0, SURTR_LANES); i = __shfl(i, 0, SURTR_LANES);
}

// The plane of triangle t from its three kept points; false when it has no area.
__device__ __forceinline__ bool ck_tri_plane(CkLds& L, uint32_t t)
{
    const CkD3 a = ck_kept(L, L.tv[t][0]), b = ck_kept(L, L.tv[t][1]), c = ck_kept(L, L.tv[t][2]);
    const CkD3 N = ck_cross(ck_sub(b, a), ck_sub(c, a));
    if (N.x == 0.0 && N.y == 0.0 && N.z == 0.0) { L.tp[t][0] = 0.0; L.tp[t][1] = 0.0; L.tp[t][2] = 0.0; L.tp[t][3] = 0.0; return false; }
    const double len = sqrt(ck_dot(N, N));
    const CkD3 n{N.x / len, N.y / len, N.z / len};
    L.tp[t][0] = n.x; L.tp[t][1] = n.y; L.tp[t][2] = n.z; L.tp[t][3] = -ck_dot(n, a);
    return true;
}

// The plane of the collision hulls (hull_dev.hip, hl_write) of the loop loop[(rot + i) % k] of kept points; false when N is zero.
__device__ __forceinline__ bool ck_newell(const CkLds& L, const uint16_t* loop, uint32_t k, uint32_t rot, double* pl)
{
    const CkD3 q0 = ck_kept(L, loop[rot]);
    double Nx = 0.0, Ny = 0.0, Nz = 0.0;
    CkD3 a{0.0, 0.0, 0.0};
    for (uint32_t i = 1; i < k; ++i)
    {
        const CkD3 b = ck_sub(ck_kept(L, loop[(rot + i) % k]), q0);
        if (i >= 2u) { const CkD3 c = ck_cross(a, b); Nx = Nx + c.x; Ny = Ny + c.y; Nz = Nz + c.z; }
        a = b;
    }
    if (Nx == 0.0 && Ny == 0.0 && Nz == 0.0) return false;
    const double len = sqrt((Nx * Nx + Ny * Ny) + Nz * Nz);
    const CkD3 n{Nx / len, Ny / len, Nz / len};
    double tmin = 0.0, tmax = 0.0;
    for (uint32_t i = 0; i < k; ++i)
    {
        const double t = ck_dot(n, ck_kept(L, loop[(rot + i) % k]));
        if (i == 0u) { tmin = t; tmax = t; }
        else { tmin = t < tmin ? t : tmin; tmax = t > tmax ? t : tmax; }
    }
    pl[0] = n.x; pl[1] = n.y; pl[2] = n.z; pl[3] = -(tmax + tmin) / 2.0;
    return true;
}

// Lane 0: the boundary of the triangles of classes A and B (lists headed by A and B; A == B: one class) into L.ia, as one closed
// counter-clockwise walk.  -> its length, 0 when the boundary is not one simple loop.
__device__ __forceinline__ uint32_t ck_boundary(CkLds& L, uint32_t A, uint32_t B, uint32_t nt, uint32_t stamp)
{
    uint32_t nb = 0, ft = CK_NONE, fk = 0;
    for (uint32_t pass = 0; pass < (A == B ? 1u : 2u); ++pass)
        for (uint32_t x = pass ? B : A; x != CK_NONE; x = L.lnk[x])
            for (uint32_t k = 0; k < 3u; ++k)
            {
                const uint32_t c = L.cls[L.ta[x][k]];
                if (c != A && c != B) { ++nb; if (ft == CK_NONE) { ft = x; fk = k; } }
            }
    if (nb < 3u || nb > CK_MAXV) return 0u;
    uint32_t t = ft, k = fk, cnt = 0;
    do
    {
        const uint32_t v = L.tv[t][k];
        if (L.mark[v] == stamp) return 0u;
        L.mark[v] = (uint16_t)stamp;
        L.ia[cnt++] = (uint16_t)v;
        const uint32_t b = L.tv[t][(k + 1u) % 3u];
        k = (k + 1u) % 3u;
        for (uint32_t guard = 0;; ++guard)      // turn about b to the next boundary edge that starts there
        {
            const uint32_t u = L.ta[t][k], c = L.cls[u];
            if (c != A && c != B) break;
            if (guard > nt) return 0u;
            uint32_t j = 0;
            while (j < 3u && L.tv[u][j] != b) ++j;
            if (j == 3u) return 0u;
            t = u; k = j;
        }
    } while (!(t == ft && k == fk) && cnt < nb);
    return (t == ft && k == fk && cnt == nb) ? nb : 0u;
}

__device__ __forceinline__ uint32_t ck_argmin16(const uint16_t* a, uint32_t n)
{
    uint32_t r = 0;
    for (uint32_t i = 1; i < n; ++i) if (a[i] < a[r]) r = i;
    return r;
}

// Lane 0: the merge of step 3.
__device__ __forceinline__ void ck_merge(CkLds& L, uint32_t nt, uint32_t nk, double tol)
{
    for (uint32_t t = 0; t < nt; ++t) { L.cls[t] = (uint16_t)t; L.lnk[t] = CK_NONE; L.tail[t] = (uint16_t)t; }
    uint32_t stamp = 0;
    bool changed = true;
    for (uint32_t pass = 0; changed && pass < 8u; ++pass)
    {
        changed = false;
        for (uint32_t t = 0; t < nt; ++t)
            for (uint32_t k = 0; k < 3u; ++k)
            {
                const uint32_t u = L.ta[t][k], A = L.cls[t], B = L.cls[u];
                if (u < t || A == B) continue;
                const uint32_t nb = ck_boundary(L, A, B, nt, ++stamp);
                if (!nb) continue;
                double pl[4];
                if (!ck_newell(L, L.ia, nb, ck_argmin16(L.ia, nb), pl)) continue;
                bool ok = true;
                for (uint32_t pass2 = 0; ok && pass2 < 2u; ++pass2)
                    for (uint32_t x = pass2 ? B : A; ok && x != CK_NONE; x = L.lnk[x])
                        for (uint32_t j = 0; j < 3u; ++j)
                            if (!(fabs(ck_dist(pl, ck_kept(L, L.tv[x][j]))) <= tol)) { ok = false; break; }
                for (uint32_t i = 0; ok && i < nk; ++i)
                    if (!(ck_dist(pl, ck_kept(L, i)) <= 2.0 * tol)) ok = false;
                if (!ok) continue;
                for (uint32_t x = B; x != CK_NONE; x = L.lnk[x]) L.cls[x] = (uint16_t)A;
                L.lnk[L.tail[A]] = (uint16_t)B; L.tail[A] = L.tail[B];
                changed = true;
            }
    }
}

// Lane 0: point p (kept index) goes into the table of nt triangles whose visibility the wave has marked.  -> the new triangles in
// L.vl[0 .. nh) and the table's new end in L.sh[1]; -> nh, 0 when the horizon does not close.
__device__ __forceinline__ uint32_t ck_insert(CkLds& L, uint32_t p, uint32_t nt, uint32_t stamp)
{
    uint32_t nvis = 0, nh = 0, st = CK_NONE, sk = 0;
    for (uint32_t t = 0; t < nt; ++t)
    {
        if (!L.vis[t]) continue;
        L.vl[nvis++] = (uint16_t)t;
        for (uint32_t k = 0; k < 3u; ++k)
            if (!L.vis[L.ta[t][k]]) { ++nh; if (st == CK_NONE) { st = t; sk = k; } }
    }
    // (a disk of nvis triangles with I vertices inside it has nvis + 2 - 2 I boundary edges: a vertex all of whose triangles go leaves the hull)
    if (nh < 3u || nh > nvis + 2u || ((nvis + 2u - nh) & 1u) || nh > CK_MAXV || nt + 2u > CK_MAXT) return 0u;
    uint32_t t = st, k = sk, cnt = 0;
    do
    {
        const uint32_t v = L.tv[t][k];
        if (L.deg[v] == stamp) return 0u;      // the walk meets a vertex twice: a pinched horizon
        L.deg[v] = (uint16_t)stamp;
        L.ha[cnt] = (uint16_t)v; L.ho[cnt] = L.ta[t][k]; ++cnt;
        const uint32_t b = L.tv[t][(k + 1u) % 3u];
        k = (k + 1u) % 3u;
        for (uint32_t guard = 0; L.vis[L.ta[t][k]]; ++guard)
        {
            if (guard > nt) return 0u;
            const uint32_t u = L.ta[t][k];
            uint32_t j = 0;
            while (j < 3u && L.tv[u][j] != b) ++j;
            if (j == 3u) return 0u;
            t = u; k = j;
        }
    } while (!(t == st && k == sk) && cnt < nh);
    if (!(t == st && k == sk) || cnt != nh) return 0u;
    // the fan: edge i takes the i-th removed slot; past them, the slots nt and nt + 1
    L.vl[nvis] = (uint16_t)nt; L.vl[nvis + 1u] = (uint16_t)(nt + 1u);
    for (uint32_t i = 0; i < nh; ++i)
    {
        const uint32_t id = L.vl[i], a = L.ha[i], b = L.ha[(i + 1u) % nh], o = L.ho[i];
        L.tv[id][0] = (uint16_t)a; L.tv[id][1] = (uint16_t)b; L.tv[id][2] = (uint16_t)p;
        L.ta[id][0] = (uint16_t)o; L.ta[id][1] = L.vl[(i + 1u) % nh]; L.ta[id][2] = L.vl[(i + nh - 1u) % nh];
        L.vis[id] = 0;
        uint32_t j = 0;
        while (j < 3u && L.tv[o][j] != b) ++j;      // the edge b -> a of the triangle outside
        if (j == 3u || L.tv[o][(j + 1u) % 3u] != a) return 0u;
        L.ta[o][j] = (uint16_t)id;
    }
    L.used[p] = 1;
    if (nh >= nvis) { L.sh[1] = nt + (nh - nvis); return nh; }
    // removed slots left over: the triangles from the table's end, last first, move into them, lowest first (none of them is new:
    // the new ones took the lowest removed slots)
    const uint32_t nt2 = nt - (nvis - nh);
    for (uint32_t i = nh; i < nvis; ++i) L.vis[L.vl[i]] = 2;
    uint32_t s = nt;
    for (uint32_t i = nh; i < nvis && L.vl[i] < nt2; ++i)
    {
        const uint32_t h = L.vl[i];
        do { --s; } while (s > nt2 && L.vis[s] == 2);
        if (L.vis[s] == 2 || s < nt2) return 0u;
        for (uint32_t k = 0; k < 3u; ++k) { L.tv[h][k] = L.tv[s][k]; L.ta[h][k] = L.ta[s][k]; }
        for (uint32_t c = 0; c < 4u; ++c) L.tp[h][c] = L.tp[s][c];
        L.vis[h] = 0;
        for (uint32_t k = 0; k < 3u; ++k)
        {
            const uint32_t u = L.ta[h][k];
            for (uint32_t j = 0; j < 3u; ++j) if (L.ta[u][j] == s) L.ta[u][j] = (uint16_t)h;
        }
    }
    L.sh[1] = nt2;
    return nh;
}

struct CkResult { uint32_t status, nv, n_faces, n_idx, max_loop, n_welded; float extent, reach; uint32_t nk; };

// The whole build of one solid; every lane of the wave runs it and gets the same result.  On a status without a withholding bit the
// LDS holds: newid / ksrc / pos (points), fo (faces by rank), fs / fl / fb, ib (loops), and the float planes L.fp.
__device__ __forceinline__ CkResult ck_build(CkLds& L, const CkSolid& S, const CkPar& par)
{
    const uint32_t l = lane_id();
    CkResult R;
    memset(&R, 0, sizeof(R));
    if (S.nv > 65535u) { R.status = SURTR_COOK_LARGE; return R; }
    // box and finiteness of the input
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    uint32_t bad = 0;
    for (uint32_t v = l; v < S.nv; v += SURTR_LANES)
        for (int c = 0; c < 3; ++c)
        {
            const float x = S.pos[3 * (size_t)v + c];
            lo[c] = fminf(lo[c], x); hi[c] = fmaxf(hi[c], x);
            if (!ck_finite(x)) bad = 1u;
        }
    if (ck_or(bad)) { R.status = SURTR_COOK_NONFINITE; return R; }
    for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1)
        for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], __shfl_down(lo[c], o, SURTR_LANES)); hi[c] = fmaxf(hi[c], __shfl_down(hi[c], o, SURTR_LANES)); }
    float extent = fmaxf(fmaxf(hi[0] - lo[0], hi[1] - lo[1]), hi[2] - lo[2]);
    extent = __shfl(extent, 0, SURTR_LANES);
    float reach = 0.f;
    for (int c = 0; c < 3; ++c) reach = fmaxf(reach, fmaxf(fabsf(lo[c]), fabsf(hi[c])));
    reach = __shfl(reach, 0, SURTR_LANES);
    // 1 weld
    uint32_t nk = 0;
    __syncthreads();
    for (uint32_t i = 0; i < S.nv; ++i)
    {
        const CkD3 p = ck_in(S, i);
        uint32_t hit = 0;
        for (uint32_t j = l; j < nk; j += SURTR_LANES)
        {
            const CkD3 d = ck_sub(p, ck_kept(L, j));
            if (ck_dot(d, d) <= par.weld2) hit = 1u;
        }
        if (ck_or(hit)) continue;
        if (nk == CK_MAXV) { R.status = SURTR_COOK_LARGE; return R; }
        if (l == 0u) { for (int c = 0; c < 3; ++c) L.pos[3 * nk + c] = S.pos[3 * (size_t)i + c]; L.ksrc[nk] = (uint16_t)i; }
        ++nk;
        __syncthreads();
    }
    R.n_welded = S.nv - nk; R.nk = nk;
    if (nk < 4u) { R.status = SURTR_COOK_FEW; return R; }
    const double tol = par.tol, tol2 = tol * tol;
    // 2 start simplex
    for (uint32_t i = l; i < nk; i += SURTR_LANES) { L.used[i] = 0; L.deg[i] = 0; L.mark[i] = 0; }
    __syncthreads();
    const CkD3 pa = ck_kept(L, 0u);
    double bv = -1.0; uint32_t bi = 0xFFFFFFFFu;
    for (uint32_t i = l; i < nk; i += SURTR_LANES) { const CkD3 d = ck_sub(ck_kept(L, i), pa); const double v = ck_dot(d, d); if (v > bv) { bv = v; bi = i; } }
    ck_argmax(bv, bi);
    if (!(bv > tol2) || bi >= nk) { R.status = SURTR_COOK_DEGENERATE; return R; }
    uint32_t ib_ = bi;
    const CkD3 ab = ck_sub(ck_kept(L, ib_), pa);
    const double ab2 = bv;
    bv = -1.0; bi = 0xFFFFFFFFu;
    for (uint32_t i = l; i < nk; i += SURTR_LANES) { const CkD3 c = ck_cross(ab, ck_sub(ck_kept(L, i), pa)); const double v = ck_dot(c, c); if (v > bv) { bv = v; bi = i; } }
    ck_argmax(bv, bi);
    if (!(bv > tol2 * ab2) || !(bv > 0.0) || bi >= nk) { R.status = SURTR_COOK_DEGENERATE; return R; }
    uint32_t ic_ = bi;
    double pl0[4];
    {
        const CkD3 N = ck_cross(ab, ck_sub(ck_kept(L, ic_), pa));
        const double len = sqrt(ck_dot(N, N));
        const CkD3 n{N.x / len, N.y / len, N.z / len};
        pl0[0] = n.x; pl0[1] = n.y; pl0[2] = n.z; pl0[3] = -ck_dot(n, pa);
    }
    bv = -1.0; bi = 0xFFFFFFFFu;
    for (uint32_t i = l; i < nk; i += SURTR_LANES) { const double v = fabs(ck_dist(pl0, ck_kept(L, i))); if (v > bv) { bv = v; bi = i; } }
    ck_argmax(bv, bi);
    if (!(bv > tol) || !(bv > 0.0) || bi >= nk) { R.status = SURTR_COOK_DEGENERATE; return R; }
    const uint32_t id_ = bi;
    if (ck_dist(pl0, ck_kept(L, id_)) > 0.0) { const uint32_t t = ib_; ib_ = ic_; ic_ = t; }
    if (l == 0u)
    {
        const uint16_t q0 = 0, q1 = (uint16_t)ib_, q2 = (uint16_t)ic_, q3 = (uint16_t)id_;
        L.tv[0][0] = q0; L.tv[0][1] = q1; L.tv[0][2] = q2;
        L.tv[1][0] = q0; L.tv[1][1] = q3; L.tv[1][2] = q1;
        L.tv[2][0] = q1; L.tv[2][1] = q3; L.tv[2][2] = q2;
        L.tv[3][0] = q2; L.tv[3][1] = q3; L.tv[3][2] = q0;
        for (uint32_t t = 0; t < 4u; ++t) L.vis[t] = 0;
        for (uint32_t t = 0; t < 4u; ++t)
            for (uint32_t k = 0; k < 3u; ++k)
                for (uint32_t u = 0; u < 4u; ++u)
                    for (uint32_t j = 0; j < 3u; ++j)
                        if (L.tv[u][j] == L.tv[t][(k + 1u) % 3u] && L.tv[u][(j + 1u) % 3u] == L.tv[t][k]) L.ta[t][k] = (uint16_t)u;
        L.used[q0] = 1; L.used[q1] = 1; L.used[q2] = 1; L.used[q3] = 1;
    }
    __syncthreads();
    uint32_t fail = 0, nt = 4;
    for (uint32_t t = l; t < nt; t += SURTR_LANES) if (!ck_tri_plane(L, t)) fail = 1u;
    fail = ck_or(fail);
    // insertion: the farthest point in front of any triangle, until none stands more than tol in front
    for (uint32_t round = 1; !fail && round <= nk; ++round)
    {
        __syncthreads();
        bv = -INFINITY; bi = 0xFFFFFFFFu;
        for (uint32_t i = l; i < nk; i += SURTR_LANES)
        {
            if (L.used[i]) continue;
            const CkD3 q = ck_kept(L, i);
            double m = -INFINITY;
            for (uint32_t t = 0; t < nt; ++t) { const double e = ck_dist(L.tp[t], q); m = e > m ? e : m; }
            if (m > bv) { bv = m; bi = i; }
        }
        ck_argmax(bv, bi);
        if (!(bv > tol) || bi >= nk) break;
        const CkD3 q = ck_kept(L, bi);
        for (uint32_t t = l; t < nt; t += SURTR_LANES) L.vis[t] = ck_dist(L.tp[t], q) > 0.0 ? 1 : 0;
        __syncthreads();
        if (l == 0u)
        {
            L.sh[0] = ck_insert(L, bi, nt, round);
        }
        __syncthreads();
        const uint32_t nh = L.sh[0];
        if (!nh) { fail = 1u; break; }
        nt = L.sh[1];
        uint32_t f2 = 0;
        for (uint32_t i = l; i < nh; i += SURTR_LANES) if (!ck_tri_plane(L, L.vl[i])) f2 = 1u;
        fail = ck_or(f2);
    }
    if (fail) { R.status = SURTR_COOK_FAILED; return R; }
    __syncthreads();
    // 3 merge, then the loops of the classes, vertex degrees, the fix-up, compaction: lane 0
    if (l == 0u)
    {
        ck_merge(L, nt, nk, tol);
        uint32_t nf = 0, off = 0, ok = 1;
        // FIX-UP.  The merge tested the plane of a class's boundary while the vertices that will leave the loops were still on it; what
        // is written is the plane of the FINAL loop.  So, until nothing is taken apart (every repetition takes at least one merged
        // class apart, and a hull of triangles alone passes): a merged class goes back to its triangles when a vertex that leaves
        // would leave a face on it with fewer than three vertices, or when its final plane, as it will be written, does not hold.
        for (uint32_t fix = 0; fix <= nt; ++fix)
        {
            for (uint32_t i = 0; i < nk; ++i) { L.deg[i] = 0; L.mark[i] = 0; }
            nf = 0; off = 0; ok = 1;
            uint32_t stamp = 0;
            // (the loops go to ib, then compacted into ia: a loop never grows)
            for (uint32_t t = 0; ok && t < nt; ++t)
            {
                if (L.cls[t] != t) continue;
                const uint32_t nb = ck_boundary(L, t, t, nt, ++stamp);
                if (!nb || off + nb > CK_MAXI) { ok = 0; break; }
                for (uint32_t i = 0; i < nb; ++i) { L.ib[off + i] = L.ia[i]; ++L.deg[L.ia[i]]; }
                L.fs[nf] = (uint16_t)off; L.fl[nf] = (uint16_t)nb; L.fb[nf] = (uint16_t)t; L.fo[nf] = 0; ++nf; off += nb;
            }
            if (!ok) break;
            uint32_t apart = 0;
            for (uint32_t f = 0; f < nf; ++f)
            {
                const uint32_t s = L.fs[f], n = L.fl[f];
                uint32_t m = 0;
                for (uint32_t i = 0; i < n; ++i) m += L.deg[L.ib[s + i]] >= 3u ? 1u : 0u;
                if (m >= 3u) continue;
                for (uint32_t i = 0; i < n; ++i) if (L.deg[L.ib[s + i]] < 3u) L.mark[L.ib[s + i]] = CK_NONE;
            }
            for (uint32_t f = 0; f < nf; ++f)
            {
                if (L.lnk[L.fb[f]] == CK_NONE) continue;      // a triangle
                const uint32_t s = L.fs[f], n = L.fl[f];
                uint32_t m = 0, best = CK_NONE, at = 0, hit = 0;
                for (uint32_t i = 0; i < n; ++i)
                {
                    const uint32_t v = L.ib[s + i];
                    if (L.mark[v] == CK_NONE) hit = 1u;
                    if (L.deg[v] < 3u) continue;
                    if (best == CK_NONE || v < best) { best = v; at = i; }      // (kept numbers ascend with the final numbers)
                    ++m;
                }
                bool holds = !hit && m >= 3u;
                if (holds)
                {
                    uint32_t w = 0;
                    for (uint32_t i = 0; i < n; ++i) { const uint32_t v = L.ib[s + (at + i) % n]; if (L.deg[v] >= 3u) L.ia[w++] = (uint16_t)v; }
                    double pl[4];
                    holds = ck_newell(L, L.ia, m, 0u, pl);
                    if (holds)
                    {
                        for (int c = 0; c < 4; ++c) pl[c] = (double)(float)pl[c];
                        const double sf = ((fabs(pl[0]) + fabs(pl[1])) + fabs(pl[2])) * (double)reach + fabs(pl[3]);
                        const double room = sf / 16777216.0;
                        for (uint32_t i = 0; holds && i < m; ++i) if (!(fabs(ck_dist(pl, ck_kept(L, L.ia[i]))) <= tol + room)) holds = false;
                        for (uint32_t i = 0; holds && i < nk; ++i) if (!(ck_dist(pl, ck_kept(L, i)) <= 2.0 * tol + room)) holds = false;
                    }
                }
                if (!holds) { L.fo[f] = 1; ++apart; }
            }
            if (!apart) break;
            for (uint32_t f = 0; f < nf; ++f)
            {
                if (!L.fo[f]) continue;
                for (uint32_t x = L.fb[f]; x != CK_NONE;)
                {
                    const uint32_t nx = L.lnk[x];
                    L.cls[x] = (uint16_t)x; L.lnk[x] = CK_NONE; L.tail[x] = (uint16_t)x;
                    x = nx;
                }
            }
        }
        uint32_t nv = 0, nidx = 0, longest = 0;
        if (ok)
        {
            for (uint32_t i = 0; i < nk; ++i) L.newid[i] = L.deg[i] >= 3u ? (uint16_t)nv++ : (uint16_t)CK_NONE;
            // ia takes the final loops (new numbers, from the smallest vertex); then ib[e] = the vertex after ia[e] on its loop
            for (uint32_t f = 0; ok && f < nf; ++f)
            {
                const uint32_t s = L.fs[f], n = L.fl[f];
                uint32_t m = 0, best = CK_NONE, at = 0;
                for (uint32_t i = 0; i < n; ++i)
                {
                    const uint32_t v = L.newid[L.ib[s + i]];
                    if (v == CK_NONE) continue;
                    ++m;
                    if (best == CK_NONE || v < best) { best = v; at = i; }
                }
                if (m < 3u) { ok = 0; break; }
                uint32_t w = nidx;
                for (uint32_t i = 0; i < n; ++i)
                {
                    const uint32_t kv = L.ib[s + (at + i) % n];
                    if (L.newid[kv] != CK_NONE) L.ia[w++] = (uint16_t)kv;      // (kept numbers for now: the planes read L.pos)
                }
                L.fs[f] = (uint16_t)nidx; L.fl[f] = (uint16_t)m;
                L.key[f] = ((uint32_t)L.newid[L.ia[nidx]] << 16) | L.newid[L.ia[nidx + 1u]];
                nidx += m; longest = m > longest ? m : longest;
            }
        }
        if (ok)
            for (uint32_t f = 0; f < nf; ++f)
                for (uint32_t i = 0; i < L.fl[f]; ++i) L.ib[L.fs[f] + i] = L.ia[L.fs[f] + (i + 1u) % L.fl[f]];
        if (ok && ((nidx & 1u) || (long long)nv - (long long)(nidx / 2u) + (long long)nf != 2ll)) ok = 0;
        L.sh[0] = ok; L.sh[1] = nf; L.sh[2] = nv; L.sh[3] = nidx; L.sh[4] = longest;
    }
    __syncthreads();
    if (!L.sh[0]) { R.status = SURTR_COOK_FAILED; return R; }
    const uint32_t nf = L.sh[1], nv = L.sh[2], nidx = L.sh[3];
    // every directed edge once, its reverse once; the rank of every face; the planes
    uint32_t wrong = 0;
    for (uint32_t e = l; e < nidx; e += SURTR_LANES)
    {
        const uint32_t a = L.ia[e], b = L.ib[e];
        uint32_t same = 0, rev = 0;
        for (uint32_t g = 0; g < nidx; ++g) { same += (L.ia[g] == a && L.ib[g] == b) ? 1u : 0u; rev += (L.ia[g] == b && L.ib[g] == a) ? 1u : 0u; }
        if (same != 1u || rev != 1u) wrong = 1u;
    }
    for (uint32_t f = l; f < nf; f += SURTR_LANES)
    {
        uint32_t r = 0;
        for (uint32_t g = 0; g < nf; ++g) r += L.key[g] < L.key[f] ? 1u : 0u;
        L.fo[r < CK_MAXT ? r : 0u] = (uint16_t)f;
    }
    if (ck_or(wrong)) { R.status = SURTR_COOK_FAILED; return R; }
    __syncthreads();      // (the triangle planes are read no more: the float planes of the faces take their place)
    uint32_t flat = 0;
    for (uint32_t f = l; f < nf; f += SURTR_LANES)
    {
        double pl[4];
        if (!ck_newell(L, L.ia + L.fs[f], L.fl[f], 0u, pl)) { flat = 1u; continue; }
        for (int c = 0; c < 4; ++c) L.fp[f][c] = (float)pl[c];
    }
    if (ck_or(flat)) { R.status = SURTR_COOK_FAILED; return R; }
    __syncthreads();
    // what status 0 promises, on the planes as written: a face's own vertices within tol + s_f, every kept point at most 2 tol + s_f in front
    uint32_t over = 0;
    for (uint32_t i = l; i < nk; i += SURTR_LANES)
    {
        const CkD3 q = ck_kept(L, i);
        for (uint32_t f = 0; f < nf; ++f)
        {
            const double pl[4] = {(double)L.fp[f][0], (double)L.fp[f][1], (double)L.fp[f][2], (double)L.fp[f][3]};
            const double room = (((fabs(pl[0]) + fabs(pl[1])) + fabs(pl[2])) * (double)reach + fabs(pl[3])) / 16777216.0;
            if (!(ck_dist(pl, q) <= 2.0 * tol + room)) over = 1u;
        }
    }
    for (uint32_t f = l; f < nf; f += SURTR_LANES)
    {
        const double pl[4] = {(double)L.fp[f][0], (double)L.fp[f][1], (double)L.fp[f][2], (double)L.fp[f][3]};
        const double room = (((fabs(pl[0]) + fabs(pl[1])) + fabs(pl[2])) * (double)reach + fabs(pl[3])) / 16777216.0;
        for (uint32_t i = 0; i < L.fl[f]; ++i) if (!(fabs(ck_dist(pl, ck_kept(L, L.ia[L.fs[f] + i]))) <= tol + room)) over = 1u;
    }
    if (ck_or(over)) { R.status = SURTR_COOK_FAILED; return R; }
    if (l == 0u)
    {
        uint32_t run = 0;
        for (uint32_t r = 0; r < nf; ++r) { const uint32_t f = L.fo[r]; L.fb[f] = (uint16_t)run; run += L.fl[f]; }
    }
    __syncthreads();
    R.status = (nv > 255u || nf > 255u) ? SURTR_COOK_OVER_255 : 0u;
    R.nv = nv; R.n_faces = nf; R.n_idx = nidx; R.max_loop = L.sh[4]; R.extent = extent; R.reach = reach;
    return R;
}

template <bool EMIT>
__global__ __launch_bounds__(SURTR_LANES) void k_ck_build(CkSrc src, CkWork W, CkPar par, surtr_cooked* __restrict__ out, float* __restrict__ points,
                                                          uint32_t* __restrict__ srcs, surtr_hull_polygon* __restrict__ polys, uint16_t* __restrict__ idx)
{
    __shared__ CkLds L;
    const uint32_t l = lane_id();
    uint32_t n;
    if (EMIT) { if (!W.hdr[1]) return; n = W.hdr[0]; }
    else { n = ck_count(src); if (n > W.nmax) n = W.nmax; }
    for (uint32_t f = blockIdx.x; f < n; f += gridDim.x)
    {
        const CkSolid S = ck_solid(src, f);
        if (!EMIT)
        {
            surtr_cooked r;
            memset(&r, 0, sizeof(r));
            r.nv_in = S.nv;
            bool skip = false;
            if (par.hulls)
            {
                const surtr_hull h0 = par.hulls[0];
                if (h0.status != SURTR_OK || h0.nv != ck_count(src)) skip = true;      // (k_ck_scan reports it)
                else skip = ck_usable(par.hulls[1u + f], par.rel_tol);
            }
            if (skip) { r.status = SURTR_COOK_SKIPPED; if (l == 0u) W.rec[f] = r; continue; }
            __syncthreads();
            const CkResult R = ck_build(L, S, par);
            r.status = R.status; r.n_welded = R.n_welded;
            if (!(R.status & CK_WITHHOLD)) { r.nv = R.nv; r.n_faces = R.n_faces; r.n_idx = R.n_idx; r.max_loop = R.max_loop; r.extent = R.extent; r.reach = R.reach; }
            if (l == 0u) W.rec[f] = r;
            continue;
        }
        const surtr_cooked r = W.rec[f];
        if (r.nv == 0u) continue;
        __syncthreads();
        const CkResult R = ck_build(L, S, par);
        if ((R.status & CK_WITHHOLD) || R.nv != r.nv || R.n_faces != r.n_faces || R.n_idx != r.n_idx) continue;      // (the same build: it cannot differ)
        for (uint32_t i = l; i < R.nk; i += SURTR_LANES)
        {
            const uint32_t v = L.newid[i];
            if (v >= r.nv) continue;
            for (int c = 0; c < 3; ++c) points[3 * ((size_t)r.pt_off + v) + c] = L.pos[3 * i + c];
            srcs[(size_t)r.pt_off + v] = L.ksrc[i];
        }
        double plan = 0.0, conv = -INFINITY;
        for (uint32_t k = l; k < r.n_faces; k += SURTR_LANES)
        {
            const uint32_t g = L.fo[k], s = L.fs[g], m = L.fl[g], base = L.fb[g];
            surtr_hull_polygon P;
            for (int c = 0; c < 4; ++c) P.plane[c] = L.fp[g][c];
            P.n_verts = (uint16_t)m; P.index_base = (uint16_t)base;
            polys[(size_t)r.face_off + k] = P;
            const double pl[4] = {(double)P.plane[0], (double)P.plane[1], (double)P.plane[2], (double)P.plane[3]};
            for (uint32_t i = 0; i < m; ++i)
            {
                const uint32_t kv = L.ia[s + i];
                if (base + i < r.n_idx) idx[(size_t)r.idx_off + base + i] = L.newid[kv];
                const double e = fabs(ck_dist(pl, ck_kept(L, kv)));
                plan = e > plan ? e : plan;
            }
        }
        for (uint32_t v0 = 0; v0 < S.nv; v0 += SURTR_LANES)      // convexity: every input point against every written plane
        {
            const CkD3 q = ck_in(S, v0 + l < S.nv ? v0 + l : S.nv - 1u);
            for (uint32_t g = 0; g < r.n_faces; ++g)
            {
                const double pl[4] = {(double)L.fp[g][0], (double)L.fp[g][1], (double)L.fp[g][2], (double)L.fp[g][3]};
                const double e = ck_dist(pl, q);
                conv = e > conv ? e : conv;
            }
        }
        conv = ck_max(conv); plan = ck_max(plan);
        if (l == 0u) { out[1u + f].convexity = (float)conv; out[1u + f].planarity = (float)plan; }
    }
}

// records_bytes >= 64 (checked on the host): the header is always written; the records only when everything fits.
__global__ __launch_bounds__(CK_WG) void k_ck_scan(CkSrc src, CkWork W, CkPar par, surtr_cooked* __restrict__ out, size_t records_bytes, size_t points_cap,
                                                   size_t polys_cap, size_t idx_cap)
{
    __shared__ uint32_t sc[3][CK_WG + 1];
    const uint32_t all = ck_count(src);
    const uint32_t n = all < W.nmax ? all : W.nmax;
    const uint32_t G = group_size(), seg = (n + G - 1u) / G;
    const uint32_t f0 = threadIdx.x * seg < n ? threadIdx.x * seg : n, f1 = f0 + seg < n ? f0 + seg : n;
    uint32_t s[3] = {0, 0, 0};
    for (uint32_t f = f0; f < f1; ++f) { s[0] += W.rec[f].nv; s[1] += W.rec[f].n_faces; s[2] += W.rec[f].n_idx; }
    for (int q = 0; q < 3; ++q) sc[q][threadIdx.x] = s[q];
    __syncthreads();
    if (threadIdx.x == 0u)
        for (int q = 0; q < 3; ++q)
        {
            uint32_t run = 0;
            for (uint32_t t = 0; t < G; ++t) { const uint32_t x = sc[q][t]; sc[q][t] = run; run += x; }
            sc[q][CK_WG] = run;
        }
    __syncthreads();
    const uint32_t tot[3] = {sc[0][CK_WG], sc[1][CK_WG], sc[2][CK_WG]};
    for (int q = 0; q < 3; ++q) s[q] = sc[q][threadIdx.x];
    bool stale = false;
    if (par.hulls) { const surtr_hull h0 = par.hulls[0]; stale = h0.status != SURTR_OK || h0.nv != all; }
    const bool fits = !stale && all <= W.nmax && ((size_t)n + 1u) * sizeof(surtr_cooked) <= records_bytes && tot[0] <= points_cap && tot[1] <= polys_cap &&
                      tot[2] <= idx_cap;
    for (uint32_t f = f0; f < f1; ++f)
    {
        surtr_cooked r = W.rec[f];
        r.pt_off = s[0]; r.face_off = s[1]; r.idx_off = s[2];
        s[0] += r.nv; s[1] += r.n_faces; s[2] += r.n_idx;
        W.rec[f] = r;
        if (fits) out[1u + f] = r;
    }
    if (threadIdx.x == 0u)
    {
        surtr_cooked h;
        memset(&h, 0, sizeof(h));
        h.nv_in = all; h.nv = stale ? 0u : tot[0]; h.n_faces = stale ? 0u : tot[1]; h.n_idx = stale ? 0u : tot[2];
        h.status = stale ? SURTR_E_STATE : (fits ? SURTR_OK : SURTR_E_CAPACITY);
        out[0] = h;
        W.hdr[0] = n; W.hdr[1] = fits ? 1u : 0u;
    }
}

hipError_t ck_alloc(void** p, size_t bytes, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    return hipMallocAsync(p, bytes, st);
#else
    (void)st;
    return hipMalloc(p, bytes);
#endif
}
void ck_free(void* p, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    (void)hipFreeAsync(p, st);
#else
    (void)st;
    (void)hipFree(p);
#endif
}

struct CkOut
{
    void* records; size_t records_bytes; float* points; size_t points_cap; uint32_t* src; surtr_hull_polygon* polys; size_t polys_cap;
    uint16_t* idx; size_t idx_cap;
};

int ck_launch(surtr_ctx* ctx, const CkSrc& src, uint32_t nmax, const CkPar& par, const CkOut& o)
{
    hipStream_t st = ctx->stream;
    CkWork W;
    W.nmax = nmax;
    const size_t o_rec = 16, bytes = o_rec + (size_t)std::max(nmax, 1u) * sizeof(surtr_cooked);
    char* base = nullptr;
    HIPCHK(ck_alloc((void**)&base, bytes, st));
    W.hdr = (uint32_t*)base; W.rec = (surtr_cooked*)(base + o_rec);
    hipError_t e = hipMemsetAsync(W.hdr, 0, 16, st);
    const uint32_t grid = std::max(1u, std::min(nmax, 65536u));
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(k_ck_build<false>, dim3(grid), dim3(SURTR_LANES), 0, st, src, W, par, (surtr_cooked*)o.records, o.points, o.src, o.polys, o.idx);
        hipLaunchKernelGGL(k_ck_scan, dim3(1), dim3(CK_WG), 0, st, src, W, par, (surtr_cooked*)o.records, o.records_bytes, o.points_cap, o.polys_cap, o.idx_cap);
        hipLaunchKernelGGL(k_ck_build<true>, dim3(grid), dim3(SURTR_LANES), 0, st, src, W, par, (surtr_cooked*)o.records, o.points, o.src, o.polys, o.idx);
        e = hipGetLastError();
    }
    ck_free(base, st);
    if (e != hipSuccess) { ctx->err = std::string("cook: ") + hipGetErrorString(e); return SURTR_E_HIP; }
    return SURTR_OK;
}

int ck_empty(surtr_ctx* ctx, void* dev_records)
{
    HIPCHK(hipMemsetAsync(dev_records, 0, sizeof(surtr_cooked), ctx->stream));
    return SURTR_OK;
}

bool ck_tol_ok(float x) { return x >= 0.f && x <= 3.4028235e38f; }
bool ck_args_ok(const CkOut& o, float rel_tol, float weld_dist, float plane_tol)
{
    return o.records && ((o.points && o.src) || o.points_cap == 0) && (o.polys || o.polys_cap == 0) && (o.idx || o.idx_cap == 0) && ck_tol_ok(rel_tol) &&
           ck_tol_ok(weld_dist) && ck_tol_ok(plane_tol);
}
CkPar ck_par(const void* hulls, float rel_tol, float weld_dist, float plane_tol)
{
    CkPar p;
    p.hulls = (const surtr_hull*)hulls; p.rel_tol = rel_tol; p.weld2 = (double)weld_dist * (double)weld_dist; p.tol = (double)plane_tol;
    return p;
}

int ck_event_dev(surtr_ctx* ctx, const CkPar& par, const CkOut& o)
{
    if (!ctx->have_event) return SURTR_E_STATE;
    if (ctx->last_current && ctx->last.status) return SURTR_E_STATE;
    if (o.records_bytes < sizeof(surtr_cooked)) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    CkSrc s;
    memset(&s, 0, sizeof(s));
    s.frags_on = 1u; s.frags = ctx->d_frags; s.apos = ctx->arena.pos; s.counts = ctx->d_counts;
    if (ctx->last_current)
    {
        const surtr_counts& c = ctx->last;
        if (((size_t)c.n_frag + 1u) * sizeof(surtr_cooked) > o.records_bytes) return SURTR_E_CAPACITY;
        if (c.n_frag == 0) return ck_empty(ctx, o.records);
        return ck_launch(ctx, s, c.n_frag, par, o);
    }
    return ck_launch(ctx, s, ctx->cap_frags, par, o);
}

int ck_pieces_dev(surtr_ctx* ctx, const CkPar& par, const CkOut& o)
{
    const PieceSet& P = ctx->cset;
    if (!P.pos || !P.vo) return SURTR_E_STATE;
    if (((size_t)ctx->n_pieces + 1u) * sizeof(surtr_cooked) > o.records_bytes) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    if (ctx->n_pieces == 0) return ck_empty(ctx, o.records);
    CkSrc s;
    memset(&s, 0, sizeof(s));
    s.pos = P.pos; s.vo = P.vo; s.n_res = ctx->n_pieces;
    return ck_launch(ctx, s, ctx->n_pieces, par, o);
}

struct CkHostOut
{
    uint32_t* n; surtr_cooked* records; uint32_t* n_points; float* points; uint32_t* src; uint32_t* n_polys; surtr_hull_polygon* polys;
    uint32_t* n_idx; uint16_t* idx;
};

// Count-then-fill around a device form: device buffers at the Euler bounds of `verts` input points, the hull records uploaded behind
// a header of their own, one download of the header, then of what the caller has room for.
template <class F>
int ck_host(surtr_ctx* ctx, uint32_t n_solids, uint64_t verts, const surtr_hull* hulls, uint32_t n_hull, float rel_tol, float weld_dist, float plane_tol,
            const CkHostOut& h, F dev_call)
{
    if (!h.n || !h.n_points || !h.n_polys || !h.n_idx) return SURTR_E_INVALID;
    const bool fill = h.records && h.points && h.src && h.polys && h.idx;
    if (!fill && (h.records || h.points || h.src || h.polys || h.idx)) return SURTR_E_INVALID;
    if (hulls && n_hull != n_solids) return SURTR_E_INVALID;
    if (!ck_tol_ok(rel_tol) || !ck_tol_ok(weld_dist) || !ck_tol_ok(plane_tol)) return SURTR_E_INVALID;
    const size_t vcap = (size_t)std::max<uint64_t>(verts, 1u);
    DevBuf<surtr_cooked> d_rec; DevBuf<float> d_pts; DevBuf<uint32_t> d_src; DevBuf<surtr_hull_polygon> d_poly; DevBuf<uint16_t> d_idx; DevBuf<surtr_hull> d_hull;
    int rc = d_rec.grow(ctx, (size_t)n_solids + 1u);
    if (rc == SURTR_OK) rc = d_pts.grow(ctx, 3 * vcap);
    if (rc == SURTR_OK) rc = d_src.grow(ctx, vcap);
    if (rc == SURTR_OK) rc = d_poly.grow(ctx, 2 * vcap);
    if (rc == SURTR_OK) rc = d_idx.grow(ctx, 6 * vcap);
    if (rc == SURTR_OK && hulls) rc = d_hull.grow(ctx, (size_t)n_solids + 1u);
    if (rc) return rc;
    std::vector<surtr_hull> up;
    if (hulls)
    {
        up.resize((size_t)n_solids + 1u);
        memset(&up[0], 0, sizeof(surtr_hull));
        up[0].nv = n_solids;
        if (n_solids) memcpy(&up[1], hulls, (size_t)n_solids * sizeof(surtr_hull));
        const hipError_t ue = hipMemcpyAsync(d_hull.p, up.data(), up.size() * sizeof(surtr_hull), hipMemcpyHostToDevice, ctx->stream);
        if (ue != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); HIPCHK(ue); }
    }
    CkOut o{d_rec.p, ((size_t)n_solids + 1u) * sizeof(surtr_cooked), d_pts.p, vcap, d_src.p, d_poly.p, 2 * vcap, d_idx.p, 6 * vcap};
    rc = dev_call(ck_par(hulls ? d_hull.p : nullptr, rel_tol, weld_dist, plane_tol), o);
    surtr_cooked hd;
    hipError_t he = hipSuccess;
    if (rc == SURTR_OK) he = hipMemcpyAsync(&hd, d_rec.p, sizeof(hd), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t hs = hipStreamSynchronize(ctx->stream);      // (whatever happened: before `up` and the buffers go)
    if (rc) return rc;
    HIPCHK(he);
    HIPCHK(hs);
    if (hd.status) return (int)hd.status;
    const bool small = fill && (*h.n < hd.nv_in || *h.n_points < hd.nv || *h.n_polys < hd.n_faces || *h.n_idx < hd.n_idx);
    *h.n = hd.nv_in; *h.n_points = hd.nv; *h.n_polys = hd.n_faces; *h.n_idx = hd.n_idx;
    if (small) return SURTR_E_CAPACITY;
    if (!fill) return SURTR_OK;
    if (hd.nv_in) HIPCHK(hipMemcpyAsync(h.records, d_rec.p + 1, (size_t)hd.nv_in * sizeof(surtr_cooked), hipMemcpyDeviceToHost, ctx->stream));
    if (hd.nv) HIPCHK(hipMemcpyAsync(h.points, d_pts.p, (size_t)hd.nv * 12, hipMemcpyDeviceToHost, ctx->stream));
    if (hd.nv) HIPCHK(hipMemcpyAsync(h.src, d_src.p, (size_t)hd.nv * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (hd.n_faces) HIPCHK(hipMemcpyAsync(h.polys, d_poly.p, (size_t)hd.n_faces * sizeof(surtr_hull_polygon), hipMemcpyDeviceToHost, ctx->stream));
    if (hd.n_idx) HIPCHK(hipMemcpyAsync(h.idx, d_idx.p, (size_t)hd.n_idx * sizeof(uint16_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SURTR_OK;
}

} // namespace

extern "C" uint32_t surtr_cook_max_vertices(void) { return CK_MAXV; }

extern "C" int surtr_event_cook_dev(surtr_ctx* ctx, const void* dev_hull_records_or_null, float rel_tol, float weld_dist, float plane_tol, void* dev_records,
                                    size_t records_bytes, float* dev_points, size_t points_cap, uint32_t* dev_src, surtr_hull_polygon* dev_polys,
                                    size_t polys_cap, uint16_t* dev_idx, size_t idx_cap)
{
    const CkOut o{dev_records, records_bytes, dev_points, points_cap, dev_src, dev_polys, polys_cap, dev_idx, idx_cap};
    if (!ctx || !ck_args_ok(o, rel_tol, weld_dist, plane_tol)) return SURTR_E_INVALID;
    return ck_event_dev(ctx, ck_par(dev_hull_records_or_null, rel_tol, weld_dist, plane_tol), o);
}

extern "C" int surtr_pieces_cook_dev(surtr_ctx* ctx, const void* dev_hull_records_or_null, float rel_tol, float weld_dist, float plane_tol, void* dev_records,
                                     size_t records_bytes, float* dev_points, size_t points_cap, uint32_t* dev_src, surtr_hull_polygon* dev_polys,
                                     size_t polys_cap, uint16_t* dev_idx, size_t idx_cap)
{
    const CkOut o{dev_records, records_bytes, dev_points, points_cap, dev_src, dev_polys, polys_cap, dev_idx, idx_cap};
    if (!ctx || !ck_args_ok(o, rel_tol, weld_dist, plane_tol)) return SURTR_E_INVALID;
    return ck_pieces_dev(ctx, ck_par(dev_hull_records_or_null, rel_tol, weld_dist, plane_tol), o);
}

extern "C" int surtr_event_cook(surtr_ctx* ctx, const surtr_hull* hull_records_or_null, uint32_t n_hull, float rel_tol, float weld_dist, float plane_tol,
                                uint32_t* n, surtr_cooked* records, uint32_t* n_points, float* points, uint32_t* src, uint32_t* n_polys,
                                surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx)
{
    if (!ctx) return SURTR_E_INVALID;
    surtr_counts c;
    if (!ctx->have_event) return SURTR_E_STATE;
    const int rc = surtr_event_counts(ctx, &c);
    if (rc == SURTR_OK && c.status) return SURTR_E_STATE;
    if (rc && ctx->last_current && ctx->last.status) return SURTR_E_STATE;
    if (rc) return rc;
    const CkHostOut h{n, records, n_points, points, src, n_polys, polys, n_idx, idx};
    return ck_host(ctx, c.n_frag, c.conv_verts, hull_records_or_null, n_hull, rel_tol, weld_dist, plane_tol, h,
                   [&](const CkPar& p, const CkOut& o) { return ck_event_dev(ctx, p, o); });
}

extern "C" int surtr_event_hulls_cook(surtr_ctx* ctx, float rel_tol, float weld_dist, float plane_tol, uint32_t* n, surtr_hull* hulls, uint32_t* n_hull_polys,
                                      surtr_hull_polygon* hull_polys, uint32_t* n_hull_idx, uint16_t* hull_idx, surtr_cooked* records, uint32_t* n_points,
                                      float* points, uint32_t* src, uint32_t* n_polys, surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx)
{
    if (!ctx || !n || !hulls || !n_hull_polys || !hull_polys || !n_hull_idx || !hull_idx || !records || !n_points || !points || !src || !n_polys || !polys ||
        !n_idx || !idx)
        return SURTR_E_INVALID;
    if (!ck_tol_ok(rel_tol) || !ck_tol_ok(weld_dist) || !ck_tol_ok(plane_tol)) return SURTR_E_INVALID;
    surtr_counts c;
    if (!ctx->have_event) return SURTR_E_STATE;
    int rc = surtr_event_counts(ctx, &c);
    if (rc == SURTR_OK && c.status) return SURTR_E_STATE;
    if (rc && ctx->last_current && ctx->last.status) return SURTR_E_STATE;
    if (rc) return rc;
    // device buffers at the bounds that are always enough: one ring entry per hull polygon and index, Euler's for the cooker
    const size_t nr = (size_t)c.n_frag + 1u, hcap = std::max<size_t>(c.conv_nbrs, 1u), vcap = std::max<size_t>(c.conv_verts, 1u);
    DevBuf<surtr_hull> d_h; DevBuf<surtr_hull_polygon> d_hp; DevBuf<uint16_t> d_hi;
    DevBuf<surtr_cooked> d_rec; DevBuf<float> d_pts; DevBuf<uint32_t> d_src; DevBuf<surtr_hull_polygon> d_poly; DevBuf<uint16_t> d_idx;
    rc = d_h.grow(ctx, nr);
    if (rc == SURTR_OK) rc = d_hp.grow(ctx, hcap);
    if (rc == SURTR_OK) rc = d_hi.grow(ctx, hcap);
    if (rc == SURTR_OK) rc = d_rec.grow(ctx, nr);
    if (rc == SURTR_OK) rc = d_pts.grow(ctx, 3 * vcap);
    if (rc == SURTR_OK) rc = d_src.grow(ctx, vcap);
    if (rc == SURTR_OK) rc = d_poly.grow(ctx, 2 * vcap);
    if (rc == SURTR_OK) rc = d_idx.grow(ctx, 6 * vcap);
    if (rc) return rc;
    // the cooker right behind the hulls on the stream: it selects from the records where they are
    rc = surtr_event_hulls_dev(ctx, d_h.p, nr * sizeof(surtr_hull), d_hp.p, hcap, d_hi.p, hcap);
    if (rc == SURTR_OK)
    {
        const CkOut o{d_rec.p, nr * sizeof(surtr_cooked), d_pts.p, vcap, d_src.p, d_poly.p, 2 * vcap, d_idx.p, 6 * vcap};
        rc = ck_event_dev(ctx, ck_par(d_h.p, rel_tol, weld_dist, plane_tol), o);
    }
    surtr_hull hh; surtr_cooked ch;
    hipError_t e1 = hipSuccess, e2 = hipSuccess;
    if (rc == SURTR_OK)
    {
        e1 = hipMemcpyAsync(&hh, d_h.p, sizeof(hh), hipMemcpyDeviceToHost, ctx->stream);
        e2 = hipMemcpyAsync(&ch, d_rec.p, sizeof(ch), hipMemcpyDeviceToHost, ctx->stream);
    }
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (rc) return rc;
    HIPCHK(e1); HIPCHK(e2); HIPCHK(es);
    if (hh.status) return (int)hh.status;
    if (ch.status) return (int)ch.status;
    const bool small = *n < hh.nv || *n_hull_polys < hh.n_faces || *n_hull_idx < hh.n_idx || *n_points < ch.nv || *n_polys < ch.n_faces || *n_idx < ch.n_idx;
    *n = hh.nv; *n_hull_polys = hh.n_faces; *n_hull_idx = hh.n_idx; *n_points = ch.nv; *n_polys = ch.n_faces; *n_idx = ch.n_idx;
    if (small) return SURTR_E_CAPACITY;
    // one download of both answers
    hipError_t e = hipSuccess;
    auto get = [&](void* dst, const void* from, size_t bytes) { if (bytes && e == hipSuccess) e = hipMemcpyAsync(dst, from, bytes, hipMemcpyDeviceToHost, ctx->stream); };
    get(hulls, d_h.p + 1, (size_t)hh.nv * sizeof(surtr_hull));
    get(hull_polys, d_hp.p, (size_t)hh.n_faces * sizeof(surtr_hull_polygon));
    get(hull_idx, d_hi.p, (size_t)hh.n_idx * sizeof(uint16_t));
    get(records, d_rec.p + 1, (size_t)ch.nv_in * sizeof(surtr_cooked));
    get(points, d_pts.p, (size_t)ch.nv * 12);
    get(src, d_src.p, (size_t)ch.nv * 4);
    get(polys, d_poly.p, (size_t)ch.n_faces * sizeof(surtr_hull_polygon));
    get(idx, d_idx.p, (size_t)ch.n_idx * sizeof(uint16_t));
    const hipError_t es2 = hipStreamSynchronize(ctx->stream);
    HIPCHK(e); HIPCHK(es2);
    return SURTR_OK;
}

extern "C" int surtr_pieces_cook(surtr_ctx* ctx, const surtr_hull* hull_records_or_null, uint32_t n_hull, float rel_tol, float weld_dist, float plane_tol,
                                 uint32_t* n, surtr_cooked* records, uint32_t* n_points, float* points, uint32_t* src, uint32_t* n_polys,
                                 surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx)
{
    if (!ctx) return SURTR_E_INVALID;
    const PieceSet& P = ctx->cset;
    if (!P.pos || !P.vo) return SURTR_E_STATE;
    const uint64_t V = ctx->h_vo[1].size() > ctx->n_pieces ? ctx->h_vo[1][ctx->n_pieces] : 0u;
    const CkHostOut h{n, records, n_points, points, src, n_polys, polys, n_idx, idx};
    return ck_host(ctx, ctx->n_pieces, V, hull_records_or_null, n_hull, rel_tol, weld_dist, plane_tol, h,
                   [&](const CkPar& p, const CkOut& o) { return ck_pieces_dev(ctx, p, o); });
}

extern "C" int surtr_cook_points(surtr_ctx* ctx, uint32_t n_solids, const uint32_t* vert_off, const float* pos, float weld_dist, float plane_tol,
                                 uint32_t* n, surtr_cooked* records, uint32_t* n_points, float* points, uint32_t* src, uint32_t* n_polys,
                                 surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx)
{
    if (!ctx || !vert_off || vert_off[0] != 0u) return SURTR_E_INVALID;
    for (uint32_t s = 0; s < n_solids; ++s) if (vert_off[s + 1] < vert_off[s]) return SURTR_E_INVALID;
    const uint32_t V = vert_off[n_solids];
    if (V && !pos) return SURTR_E_INVALID;
    (void)hipSetDevice(ctx->device);
    DevBuf<float> d_pos; DevBuf<uint32_t> d_vo;
    int rc = d_pos.grow(ctx, 3 * (size_t)std::max(V, 1u));
    if (rc == SURTR_OK) rc = d_vo.grow(ctx, (size_t)n_solids + 1u);
    if (rc) return rc;
    if (V) HIPCHK(hipMemcpyAsync(d_pos.p, pos, (size_t)V * 12, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(d_vo.p, vert_off, ((size_t)n_solids + 1u) * 4, hipMemcpyHostToDevice, ctx->stream));
    const CkHostOut h{n, records, n_points, points, src, n_polys, polys, n_idx, idx};
    rc = ck_host(ctx, n_solids, V, nullptr, 0, 0.f, weld_dist, plane_tol, h, [&](const CkPar& p, const CkOut& o) {
        if (n_solids == 0) return ck_empty(ctx, o.records);
        CkSrc s;
        memset(&s, 0, sizeof(s));
        s.pos = d_pos.p; s.vo = d_vo.p; s.n_res = n_solids;
        return ck_launch(ctx, s, n_solids, p, o);
    });
    (void)hipStreamSynchronize(ctx->stream);      // the uploads are read by the stream until here
    return rc;
}
