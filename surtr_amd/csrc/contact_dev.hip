// contact_dev.hip -- scene contacts: which bodies of the resident scene are within a margin of each other, through which pieces, how
// far apart, at which points and along which normal, from the resident Convex solids and the poses, on the device (the definition is
// in include/surtr_hip.h).  A post-pass on resident data: it touches no clip kernel, no event and no commit.
//
//   bounds          surtr_scene_bounds_dev's own launch (k_bounds_pieces, k_bounds_bodies) into the context's buffers
//   k_ct_bodies     count, then fill: a wave owns a row, body a against the bodies b > a.  The four rows of a workgroup share the
//                   column records through LDS in tiles of SURTR_WG; lanes stride the columns; ballot + popcount give the count and,
//                   behind the row's offset, the slot.  O(n^2) box tests
//   k_ct_pieces     count, then fill: a wave owns piece p of body a and walks a's candidate bodies b in order, lanes striding the
//                   pieces q of b.  Rows ascend by p and columns by q: the list is in (piece_a, piece_b) order without a sort
//   k_ct_distance   one wave per candidate piece pair: GJK in double.  The simplex and the search direction are wave-uniform (every lane
//                   computes the same doubles); the support function is the parallel part: each lane the dot product of its vertices,
//                   then a wave reduction of (value, lowest index).  A solid of at most SURTR_LANES vertices is transformed once and
//                   lives in its lanes' registers; a larger one is strided over (12-byte positions, coalesced) and transformed on the fly
//   k_ct_header     one thread: the totals, the capacity checks, the caller's header
//   k_ct_gather     flag -> scan -> gather: the reported pairs, in order
// The three exclusive sums are hipcub's (integers: the same bits however they are arranged).  No atomics anywhere.
#include <cmath>
#include <cstring>
#include <hipcub/hipcub.hpp>      // (the emulation header brings its own exclusive sum)

#include "surtr_ctx.h"

static_assert(sizeof(surtr_contact) == 64 && sizeof(surtr_contact_header) == 64, "surtr_contact and its header are 64 bytes each");

#define CT_ITER_CAP 96u
#define CT_REL 1.4551915228366852e-11      // 2^-36
#define CT_ABS 5.6843418860808015e-14      // 2^-44
#define CT_FLT_EPS 5.9604644775390625e-08  // 2^-24
#define CT_FLAT 5.6843418860808015e-14      // 2^-44: see ct_tet

namespace {

struct CtWork
{
    uint32_t nc, np, cap_bp, cap_pp;
    const surtr_bounds* body; const surtr_bounds* piece;
    const uint32_t* comp_off; const uint32_t* piece_comp;
    const float* cpos; const uint32_t* cvo; const float* posef;      // the resident Convex set; 16 floats per compound, or null
    uint32_t* row_cnt; uint32_t* row_off;      // nc + 1: candidates of row a, their exclusive sums (row_off[nc]: body pairs)
    uint32_t* bp;                              // cap_bp: body b of every candidate, row after row
    uint32_t* pc_cnt; uint32_t* pc_off;        // np + 1: candidates of piece p (pc_off[np]: piece pairs)
    uint2* pp;                                 // cap_pp: (p, q)
    uint32_t* flag; uint32_t* flag_off;        // cap_pp + 1: reported
    surtr_contact* res;                        // cap_pp
    uint32_t* go;                              // [0] the caller's buffer holds everything: the gather runs
};

__device__ __forceinline__ uint32_t ct_rank(unsigned long long m) { return (uint32_t)__builtin_popcountll(m & ((1ull << lane_id()) - 1ull)); }

// The broad and mid phase predicate, in double on the float records.
__device__ __forceinline__ bool ct_near(const surtr_bounds& a, const surtr_bounds& b, double margin)
{
    bool near = true;
    for (int k = 0; k < 3; ++k)
        near = near && (double)a.lo[k] - (double)b.hi[k] <= margin && (double)b.lo[k] - (double)a.hi[k] <= margin;
    return near;
}

template <bool FILL>
__global__ __launch_bounds__(SURTR_WG) void k_ct_bodies(CtWork W, float margin)
{
    __shared__ surtr_bounds tile[SURTR_WG];
    const uint32_t a0 = blockIdx.x * group_waves(), a = a0 + wave_id();
    const bool row = a < W.nc;
    surtr_bounds A;
    memset(&A, 0, sizeof(A));
    if (row) A = W.body[a];
    const bool a_ok = row && (A.status & SURTR_BOUNDS_NONFINITE) == 0u;
    if (FILL && W.row_off[W.nc] > W.cap_bp) return;      // (uniform over the grid: the list has no room, k_ct_header says so)
    const uint32_t base = FILL && row ? W.row_off[a] : 0u;
    uint32_t count = 0;
    for (uint32_t t0 = a0 + 1u; t0 < W.nc; t0 += group_size())
    {
        const uint32_t tn = W.nc - t0 < group_size() ? W.nc - t0 : group_size();
        __syncthreads();
        if (threadIdx.x < tn) tile[threadIdx.x] = W.body[t0 + threadIdx.x];
        __syncthreads();
        for (uint32_t j0 = 0; j0 < tn; j0 += SURTR_LANES)
        {
            const uint32_t j = j0 + lane_id(), b = t0 + j;
            const bool hit = a_ok && j < tn && b > a && (tile[j].status & SURTR_BOUNDS_NONFINITE) == 0u && ct_near(A, tile[j], (double)margin);
            const unsigned long long m = __ballot(hit);
            if (FILL && hit) W.bp[base + count + ct_rank(m)] = b;
            count += (uint32_t)__builtin_popcountll(m);
        }
    }
    if (!FILL && row && lane_id() == 0u) W.row_cnt[a] = count;
}

template <bool FILL>
__global__ __launch_bounds__(SURTR_WG) void k_ct_pieces(CtWork W, float margin)
{
    const uint32_t p = blockIdx.x * group_waves() + wave_id();
    if (p >= W.np) return;
    if (W.row_off[W.nc] > W.cap_bp) { if (!FILL && lane_id() == 0u) W.pc_cnt[p] = 0u; return; }
    if (FILL && W.pc_off[W.np] > W.cap_pp) return;
    const uint32_t a = W.piece_comp[p];
    const surtr_bounds P = W.piece[p];
    const uint32_t base = FILL ? W.pc_off[p] : 0u;
    uint32_t count = 0;
    for (uint32_t e = W.row_off[a]; e < W.row_off[a + 1u]; ++e)
    {
        const uint32_t b = W.bp[e], q1 = W.comp_off[b + 1u];
        for (uint32_t q0 = W.comp_off[b]; q0 < q1; q0 += SURTR_LANES)
        {
            const uint32_t q = q0 + lane_id();
            const bool hit = q < q1 && ct_near(P, W.piece[q], (double)margin);
            const unsigned long long m = __ballot(hit);
            if (FILL && hit) W.pp[base + count + ct_rank(m)] = make_uint2(p, q);
            count += (uint32_t)__builtin_popcountll(m);
        }
    }
    if (!FILL && lane_id() == 0u) W.pc_cnt[p] = count;
}

// ------------------------------------------------------------------ narrow phase
struct CtSolid { const float* pos; uint32_t n; bool posed; bool reg; float W[16]; };

__device__ __forceinline__ void ct_solid(const CtWork& K, uint32_t p, CtSolid& S)
{
    const uint32_t v0 = K.cvo[p];
    S.pos = K.cpos + 3 * (size_t)v0; S.n = K.cvo[p + 1u] - v0; S.posed = false; S.reg = S.n <= SURTR_LANES;
    for (int k = 0; k < 16; ++k) S.W[k] = k % 5 == 0 ? 1.f : 0.f;
    if (K.posef)
    {
        const float* src = K.posef + 16 * (size_t)K.piece_comp[p];
        for (int k = 0; k < 16; ++k)
        {
            S.W[k] = src[k];
            S.posed = S.posed || __float_as_uint(S.W[k]) != (k % 5 == 0 ? 0x3F800000u : 0u);      // (k_bounds_pieces' identity short-cut)
        }
    }
}
// World vertex i: the float position surtr_scene_apply_pose would write, as a double.
__device__ __forceinline__ void ct_vertex(const CtSolid& S, uint32_t i, double out[3])
{
    float x[3] = {S.pos[3 * (size_t)i], S.pos[3 * (size_t)i + 1], S.pos[3 * (size_t)i + 2]};
    if (S.posed) transform_coord(S.W, x[0], x[1], x[2], x);
    out[0] = (double)x[0]; out[1] = (double)x[1]; out[2] = (double)x[2];
}
__device__ __forceinline__ double ct_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ void ct_cross(const double a[3], const double b[3], double o[3])
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double ct_wave_max(double x)
{
    for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1) { const double t = __shfl_down(x, o, SURTR_LANES); x = t > x ? t : x; }
    return __shfl(x, 0, SURTR_LANES);
}
// First pass over a solid: the largest absolute coordinate; a solid that fits the wave leaves lane l's vertex in mine.
__device__ __forceinline__ double ct_load(const CtSolid& S, double mine[3])
{
    double s = 0.0;
    mine[0] = mine[1] = mine[2] = 0.0;
    if (S.reg) { if (lane_id() < S.n) { ct_vertex(S, lane_id(), mine); for (int k = 0; k < 3; ++k) s = fabs(mine[k]) > s ? fabs(mine[k]) : s; } }
    else
        for (uint32_t i = lane_id(); i < S.n; i += SURTR_LANES)
        {
            double q[3];
            ct_vertex(S, i, q);
            for (int k = 0; k < 3; ++k) s = fabs(q[k]) > s ? fabs(q[k]) : s;
        }
    return s;
}
// The vertex of S furthest along d (ties: the lowest number), for every lane of the wave.
__device__ __forceinline__ uint32_t ct_support(const CtSolid& S, const double mine[3], const double d[3], double out[3])
{
    double bv = -INFINITY;
    uint32_t bi = 0xFFFFFFFFu;
    if (S.reg) { if (lane_id() < S.n) { bv = ct_dot(mine, d); bi = lane_id(); } }
    else
        for (uint32_t i = lane_id(); i < S.n; i += SURTR_LANES)
        {
            double q[3];
            ct_vertex(S, i, q);
            const double v = ct_dot(q, d);
            if (v > bv || bi == 0xFFFFFFFFu) { bv = v; bi = i; }
        }
    for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1)
    {
        const double tv = __shfl_down(bv, o, SURTR_LANES);
        const uint32_t ti = __shfl_down(bi, o, SURTR_LANES);
        if (ti != 0xFFFFFFFFu && (bi == 0xFFFFFFFFu || tv > bv || (tv == bv && ti < bi))) { bv = tv; bi = ti; }
    }
    bi = __shfl(bi, 0, SURTR_LANES);
    if (S.reg) { for (int k = 0; k < 3; ++k) out[k] = __shfl(mine[k], (int)bi, SURTR_LANES); }
    else ct_vertex(S, bi, out);
    return bi;
}

// One point of the simplex: w = a - b with a a vertex of A and b one of B.
struct CtPt { double w[3], a[3], b[3]; uint32_t ia, ib; };

// The point of segment pq nearest the origin: weights of p and q.
__device__ __forceinline__ void ct_seg(const double p[3], const double q[3], double& lp, double& lq)
{
    const double d[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
    const double dd = ct_dot(d, d);
    double t = dd > 0.0 ? -ct_dot(p, d) / dd : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    lp = 1.0 - t; lq = t;
}
__device__ __forceinline__ double ct_norm2(const double a[3], const double b[3], const double c[3], const double l[3])
{
    const double x[3] = {l[0] * a[0] + l[1] * b[0] + l[2] * c[0], l[0] * a[1] + l[1] * b[1] + l[2] * c[1], l[0] * a[2] + l[1] * b[2] + l[2] * c[2]};
    return ct_dot(x, x);
}
// The point of triangle abc nearest the origin, by Voronoi regions: its weights; -> its squared norm.  A triangle without area
// falls through to the best of its edges.
__device__ double ct_tri(const double a[3], const double b[3], const double c[3], double l[3])
{
    const double ab[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, ac[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
    const double d1 = -ct_dot(ab, a), d2 = -ct_dot(ac, a), d3 = -ct_dot(ab, b), d4 = -ct_dot(ac, b), d5 = -ct_dot(ab, c), d6 = -ct_dot(ac, c);
    // The areas opposite c, b and a as n . (a x b), n . (c x a), n . (b x c) with n = ab x ac: the same numbers as d1 d4 - d3 d2 and so
    // on, but n comes from exact differences, so a needle of a triangle (support points of two touching faces) keeps its digits.
    double n[3], cab[3], cca[3], cbc[3];
    ct_cross(ab, ac, n); ct_cross(a, b, cab); ct_cross(c, a, cca); ct_cross(b, c, cbc);
    const double vc = ct_dot(n, cab), vb = ct_dot(n, cca), va = ct_dot(n, cbc);
    l[0] = l[1] = l[2] = 0.0;
    if (d1 <= 0.0 && d2 <= 0.0) l[0] = 1.0;
    else if (d3 >= 0.0 && d4 <= d3) l[1] = 1.0;
    else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0) { const double v = d1 / (d1 - d3); l[0] = 1.0 - v; l[1] = v; }
    else if (d6 >= 0.0 && d5 <= d6) l[2] = 1.0;
    else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0) { const double w = d2 / (d2 - d6); l[0] = 1.0 - w; l[2] = w; }
    else if (va <= 0.0 && d4 - d3 >= 0.0 && d5 - d6 >= 0.0) { const double w = (d4 - d3) / ((d4 - d3) + (d5 - d6)); l[1] = 1.0 - w; l[2] = w; }
    else if (va + vb + vc > 0.0) { const double k = 1.0 / (va + vb + vc); l[1] = vb * k; l[2] = vc * k; l[0] = 1.0 - l[1] - l[2]; }
    else
    {
        double e[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
        ct_seg(a, b, e[0][0], e[0][1]); ct_seg(a, c, e[1][0], e[1][2]); ct_seg(b, c, e[2][1], e[2][2]);
        double best = ct_norm2(a, b, c, e[0]);
        for (int k = 0; k < 3; ++k) l[k] = e[0][k];
        for (int s = 1; s < 3; ++s)
        {
            const double n2 = ct_norm2(a, b, c, e[s]);
            if (n2 < best) { best = n2; for (int k = 0; k < 3; ++k) l[k] = e[s][k]; }
        }
    }
    return ct_norm2(a, b, c, l);
}
__device__ __forceinline__ double ct_orient(const double a[3], const double b[3], const double c[3], const double d[3])
{
    const double x[3] = {a[0] - d[0], a[1] - d[1], a[2] - d[2]}, y[3] = {b[0] - d[0], b[1] - d[1], b[2] - d[2]}, z[3] = {c[0] - d[0], c[1] - d[1], c[2] - d[2]};
    double yz[3];
    ct_cross(y, z, yz);
    return ct_dot(x, yz);
}
// The point of tetrahedron p0..p3 nearest the origin: its weights; -> true when the origin is inside (the weights are then its
// barycentric coordinates).  Otherwise the nearest of the four faces (ties: the first), so at least one weight is zero.
__device__ bool ct_tet(const double p0[3], const double p1[3], const double p2[3], const double p3[3], double l[4])
{
    const double O[3] = {0.0, 0.0, 0.0};
    const double V = ct_orient(p0, p1, p2, p3);
    // flat: the volume is within the rounding of its own sum, |p0 - p3| |(p1 - p3) x (p2 - p3)| in the 1-norm times 2^-44
    const double x[3] = {p0[0] - p3[0], p0[1] - p3[1], p0[2] - p3[2]}, y[3] = {p1[0] - p3[0], p1[1] - p3[1], p1[2] - p3[2]}, z[3] = {p2[0] - p3[0], p2[1] - p3[1], p2[2] - p3[2]};
    double yz[3];
    ct_cross(y, z, yz);
    const double mag = (fabs(x[0]) + fabs(x[1]) + fabs(x[2])) * (fabs(yz[0]) + fabs(yz[1]) + fabs(yz[2]));
    if (fabs(V) > CT_FLAT * mag)
    {
        const double b0 = ct_orient(O, p1, p2, p3) / V, b1 = ct_orient(p0, O, p2, p3) / V, b2 = ct_orient(p0, p1, O, p3) / V, b3 = ct_orient(p0, p1, p2, O) / V;
        if (b0 > 0.0 && b1 > 0.0 && b2 > 0.0 && b3 > 0.0)
        {
            const double s = b0 + b1 + b2 + b3;
            l[0] = b0 / s; l[1] = b1 / s; l[2] = b2 / s; l[3] = b3 / s;
            return true;
        }
    }
    double t[3];
    double best = ct_tri(p1, p2, p3, t);                           // without p0
    l[0] = 0.0; l[1] = t[0]; l[2] = t[1]; l[3] = t[2];
    double n2 = ct_tri(p0, p2, p3, t);                             // without p1
    if (n2 < best) { best = n2; l[0] = t[0]; l[1] = 0.0; l[2] = t[1]; l[3] = t[2]; }
    n2 = ct_tri(p0, p1, p3, t);                                    // without p2
    if (n2 < best) { best = n2; l[0] = t[0]; l[1] = t[1]; l[2] = 0.0; l[3] = t[2]; }
    n2 = ct_tri(p0, p1, p2, t);                                    // without p3
    if (n2 < best) { best = n2; l[0] = t[0]; l[1] = t[1]; l[2] = t[2]; l[3] = 0.0; }
    return false;
}

// GJK on the Minkowski difference A - B, wave-uniform but for the support function.  Every index into the simplex is a
// compile-time constant after unrolling: it stays in registers.
__device__ void ct_gjk(const CtSolid& A, const CtSolid& B, double margin, surtr_contact& r, uint32_t& report)
{
    double mineA[3], mineB[3];
    const double sa = ct_load(A, mineA), sb = ct_load(B, mineB);
    const double S = ct_wave_max(sa > sb ? sa : sb), thr = CT_FLT_EPS * S;
    CtPt P[4] = {};
    double lam[4] = {1.0, 0.0, 0.0, 0.0};
    ct_vertex(A, 0u, P[0].a); ct_vertex(B, 0u, P[0].b);
    for (int k = 0; k < 3; ++k) P[0].w[k] = P[0].a[k] - P[0].b[k];
    uint32_t n = 1, status = 0;
    double v[3] = {P[0].w[0], P[0].w[1], P[0].w[2]};
    for (uint32_t it = 0;; ++it)
    {
        const double vv = ct_dot(v, v);
        if (vv <= thr * thr) break;
        if (it == CT_ITER_CAP) { status |= SURTR_CONTACT_ITER; break; }
        CtPt N;
        const double nv[3] = {-v[0], -v[1], -v[2]};
        N.ia = ct_support(A, mineA, nv, N.a);
        N.ib = ct_support(B, mineB, v, N.b);
        for (int k = 0; k < 3; ++k) N.w[k] = N.a[k] - N.b[k];
        bool dup = false;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) dup = dup || (i < n && P[i].ia == N.ia && P[i].ib == N.ib);
        if (dup) break;
        if (vv - ct_dot(v, N.w) <= CT_REL * vv + CT_ABS * S * sqrt(vv)) break;
#pragma unroll
        for (uint32_t i = 0; i < 4u; ++i) if (i == n) P[i] = N;      // (n <= 3 here: a tetrahedron that does not hold the origin loses a vertex)
        ++n;
        bool inside = false;
        lam[0] = lam[1] = lam[2] = lam[3] = 0.0;
        if (n == 2u) ct_seg(P[0].w, P[1].w, lam[0], lam[1]);
        else if (n == 3u) { double t[3]; (void)ct_tri(P[0].w, P[1].w, P[2].w, t); lam[0] = t[0]; lam[1] = t[1]; lam[2] = t[2]; }
        else inside = ct_tet(P[0].w, P[1].w, P[2].w, P[3].w, lam);
        // the vertices the nearest point does not rest on leave the simplex (from the back, so that the others keep their order)
#pragma unroll
        for (int i = 3; i >= 0; --i)
            if ((uint32_t)i < n && lam[i] == 0.0 && n > 1u)
            {
#pragma unroll
                for (int k = i; k < 3; ++k) { P[k] = P[k + 1]; lam[k] = lam[k + 1]; }
                lam[3] = 0.0;
                --n;
            }
        for (int k = 0; k < 3; ++k) v[k] = lam[0] * P[0].w[k] + lam[1] * P[1].w[k] + lam[2] * P[2].w[k] + lam[3] * P[3].w[k];
        if (inside) { v[0] = v[1] = v[2] = 0.0; break; }
        // The old nearest point lies in the new simplex, so the new one is nearer, or the arithmetic has reached its own rounding
        // (coplanar support points of two touching faces can otherwise be taken up and dropped in turn, without end).
        if (ct_dot(v, v) >= vv) break;
    }
    double pa[3], pb[3], u[3];
    for (int k = 0; k < 3; ++k)
    {
        pa[k] = lam[0] * P[0].a[k] + lam[1] * P[1].a[k] + lam[2] * P[2].a[k] + lam[3] * P[3].a[k];
        pb[k] = lam[0] * P[0].b[k] + lam[1] * P[1].b[k] + lam[2] * P[2].b[k] + lam[3] * P[3].b[k];
        u[k] = pb[k] - pa[k];
    }
    const double d = sqrt(ct_dot(u, u));
    if (d <= thr || (v[0] == 0.0 && v[1] == 0.0 && v[2] == 0.0))
    {
        status |= SURTR_CONTACT_OVERLAP;
        r.distance = 0.f;
        for (int k = 0; k < 3; ++k) { r.point_a[k] = r.point_b[k] = (float)(0.5 * (pa[k] + pb[k])); r.normal[k] = 0.f; }
        report = 1u;
    }
    else
    {
        r.distance = (float)d;
        for (int k = 0; k < 3; ++k) { r.point_a[k] = (float)pa[k]; r.point_b[k] = (float)pb[k]; r.normal[k] = (float)(u[k] / d); }
        report = d <= margin ? 1u : 0u;
    }
    r.status = status;
}

__global__ __launch_bounds__(SURTR_LANES) void k_ct_distance(CtWork W, float margin)
{
    if (W.row_off[W.nc] > W.cap_bp) return;
    const uint32_t n_pp = W.pc_off[W.np];
    if (n_pp > W.cap_pp) return;
    for (uint32_t i = blockIdx.x; i < n_pp; i += gridDim.x)
    {
        const uint2 pq = W.pp[i];
        CtSolid A, B;
        ct_solid(W, pq.x, A); ct_solid(W, pq.y, B);
        surtr_contact r;
        memset(&r, 0, sizeof(r));
        r.body_a = W.piece_comp[pq.x]; r.body_b = W.piece_comp[pq.y]; r.piece_a = pq.x; r.piece_b = pq.y;
        uint32_t report = 0;
        if (A.n != 0u && B.n != 0u) ct_gjk(A, B, (double)margin, r, report);
        if (lane_id() == 0u) { W.res[i] = r; W.flag[i] = report; }
    }
}

__global__ void k_ct_header(CtWork W, surtr_contact_header* __restrict__ out, size_t records_bytes)
{
    if (blockIdx.x != 0u || threadIdx.x != 0u) return;
    surtr_contact_header h;
    memset(&h, 0, sizeof(h));
    h.n_bodies = W.nc; h.n_pieces = W.np;
    h.n_body_pairs = W.row_off[W.nc];
    if (h.n_body_pairs > W.cap_bp) h.lists |= 1u;
    else
    {
        h.n_piece_pairs = W.pc_off[W.np];
        if (h.n_piece_pairs > W.cap_pp) h.lists |= 2u;
        else h.n_records = W.flag_off[W.cap_pp];
    }
    const bool fits = ((size_t)h.n_records + 1u) * sizeof(surtr_contact) <= records_bytes;
    h.status = h.lists || !fits ? SURTR_E_CAPACITY : SURTR_OK;
    *out = h;
    W.go[0] = h.status == SURTR_OK ? 1u : 0u;
}

__global__ void k_ct_gather(CtWork W, surtr_contact* __restrict__ out)
{
    if (!W.go[0]) return;
    const uint32_t n_pp = W.pc_off[W.np];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_pp; i += gridDim.x * blockDim.x)
        if (W.flag[i]) out[W.flag_off[i]] = W.res[i];
}

hipError_t ct_alloc(void** p, size_t bytes, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    return hipMallocAsync(p, bytes, st);
#else
    (void)st;
    return hipMalloc(p, bytes);
#endif
}
void ct_free(void* p, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    (void)hipFreeAsync(p, st);
#else
    (void)st;
    (void)hipFree(p);
#endif
}

// The temporaries of one call, kept by the host form until it has fetched the records.
struct CtRun { CtWork W; char* base = nullptr; };

int ct_check(surtr_ctx* ctx, float margin)
{
    if (!ctx || !(margin >= 0.f) || !(margin <= 3.4028235e38f)) return SURTR_E_INVALID;
    const PieceSet& P = ctx->cset;
    if (!P.pos || !P.vo || ctx->n_pieces == 0 || ctx->scene_off.size() < 2) return SURTR_E_STATE;
    return SURTR_OK;
}

// Header and gather alone, over temporaries that are still there.
int ct_emit(surtr_ctx* ctx, const CtWork& W, void* dev_records, size_t records_bytes)
{
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_ct_header, dim3(1), dim3(1), 0, st, W, (surtr_contact_header*)dev_records, records_bytes);
    const uint32_t grid = std::max(1u, std::min((W.cap_pp + 255u) / 256u, 4096u));
    hipLaunchKernelGGL(k_ct_gather, dim3(grid), dim3(256), 0, st, W, (surtr_contact*)dev_records + 1);
    HIPCHK(hipGetLastError());
    return SURTR_OK;
}

int ct_launch(surtr_ctx* ctx, float margin, void* dev_records, size_t records_bytes, CtRun* keep)
{
    int rc = ct_check(ctx, margin);
    if (rc) return rc;
    if (!dev_records) return SURTR_E_INVALID;
    if (records_bytes < sizeof(surtr_contact_header)) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    const uint32_t nc = (uint32_t)ctx->scene_off.size() - 1u, np = ctx->n_pieces;
    const bool prof = ctx->profiling;
    if (prof && !ctx->contact_ev.e[0]) for (hipEvent_t& e : ctx->contact_ev.e) HIPCHK(hipEventCreate(&e));
    ctx->contact_ev.valid = false;
    auto stamp = [&](int k) { if (prof) (void)hipEventRecord(ctx->contact_ev.e[k], st); };
    stamp(0);
    // ---- the bounds, by their own launch, into the context's buffers (this also brings the scene's tables and float poses up to date)
    if ((rc = ctx->d_bounds_body.grow(ctx, nc, (size_t)nc + nc / 4 + 64)) != SURTR_OK) return rc;
    if ((rc = surtr_scene_bounds_dev(ctx, 1, ctx->d_bounds_body.p, (size_t)nc * sizeof(surtr_bounds), nullptr, 0)) != SURTR_OK) return rc;
    SceneDev sc;
    if ((rc = scene_sync_device(ctx, &sc)) != SURTR_OK) return rc;
    stamp(1);
    // ---- the lists' room: the worst case of this scene (every body near every other), up to SURTR_CONTACT_MAX_PAIRS
    uint64_t worst_bp = (uint64_t)nc * (nc - 1u) / 2u, sq = 0;
    for (uint32_t c = 0; c < nc; ++c) { const uint64_t k = ctx->scene_off[c + 1] - ctx->scene_off[c]; sq += k * k; }
    uint64_t worst_pp = ((uint64_t)np * np - sq) / 2u;
    CtWork W;
    memset(&W, 0, sizeof(W));
    W.nc = nc; W.np = np;
    W.cap_bp = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(worst_bp, 1u), SURTR_CONTACT_MAX_PAIRS);
    W.cap_pp = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(worst_pp, 1u), SURTR_CONTACT_MAX_PAIRS);
    W.body = ctx->d_bounds_body.p; W.piece = ctx->d_bounds_piece.p; W.comp_off = sc.comp_off; W.piece_comp = sc.piece_comp;
    W.cpos = ctx->cset.pos; W.cvo = ctx->cset.vo; W.posef = ctx->scene_pose.empty() ? nullptr : ctx->d_posef.p;
    size_t tmp_bytes = 0, tb = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)nc + 1, st); tmp_bytes = std::max(tmp_bytes, tb);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)np + 1, st); tmp_bytes = std::max(tmp_bytes, tb);
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, tb, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)W.cap_pp + 1, st); tmp_bytes = std::max(tmp_bytes, tb);
    size_t at = 0;
    auto take = [&](size_t bytes) { const size_t r = at; at += (bytes + 255) & ~(size_t)255; return r; };
    // (the counts first and next to each other: one fill clears them)
    const size_t o_go = take(16), o_rowc = take(((size_t)nc + 1) * 4), o_pcc = take(((size_t)np + 1) * 4), o_flag = take(((size_t)W.cap_pp + 1) * 4);
    const size_t zero_bytes = at;
    const size_t o_rowo = take(((size_t)nc + 1) * 4), o_pco = take(((size_t)np + 1) * 4), o_flago = take(((size_t)W.cap_pp + 1) * 4);
    const size_t o_bp = take((size_t)W.cap_bp * 4), o_pp = take((size_t)W.cap_pp * 8), o_res = take((size_t)W.cap_pp * sizeof(surtr_contact));
    const size_t o_tmp = take(tmp_bytes);
    char* base = nullptr;
    HIPCHK(ct_alloc((void**)&base, at, st));
    W.go = (uint32_t*)(base + o_go); W.row_cnt = (uint32_t*)(base + o_rowc); W.pc_cnt = (uint32_t*)(base + o_pcc); W.flag = (uint32_t*)(base + o_flag);
    W.row_off = (uint32_t*)(base + o_rowo); W.pc_off = (uint32_t*)(base + o_pco); W.flag_off = (uint32_t*)(base + o_flago);
    W.bp = (uint32_t*)(base + o_bp); W.pp = (uint2*)(base + o_pp); W.res = (surtr_contact*)(base + o_res);
    void* tmp = base + o_tmp;
    hipError_t e = hipMemsetAsync(base, 0, zero_bytes, st);
    const uint32_t g_rows = (nc + SURTR_NWAVE - 1u) / SURTR_NWAVE, g_pieces = (np + SURTR_NWAVE - 1u) / SURTR_NWAVE;
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(k_ct_bodies<false>, dim3(g_rows), dim3(SURTR_WG), 0, st, W, margin);
        tb = tmp_bytes; e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, W.row_cnt, W.row_off, (int)nc + 1, st);
    }
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(k_ct_bodies<true>, dim3(g_rows), dim3(SURTR_WG), 0, st, W, margin);
        hipLaunchKernelGGL(k_ct_pieces<false>, dim3(g_pieces), dim3(SURTR_WG), 0, st, W, margin);
        tb = tmp_bytes; e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, W.pc_cnt, W.pc_off, (int)np + 1, st);
    }
    if (e == hipSuccess)
    {
        hipLaunchKernelGGL(k_ct_pieces<true>, dim3(g_pieces), dim3(SURTR_WG), 0, st, W, margin);
        stamp(2);
        hipLaunchKernelGGL(k_ct_distance, dim3(std::max(1u, std::min(W.cap_pp, 16384u))), dim3(SURTR_LANES), 0, st, W, margin);
        stamp(3);
        tb = tmp_bytes; e = hipcub::DeviceScan::ExclusiveSum(tmp, tb, W.flag, W.flag_off, (int)W.cap_pp + 1, st);
    }
    if (e == hipSuccess) e = hipGetLastError();
    rc = SURTR_OK;
    if (e != hipSuccess) { ctx->err = std::string("contacts: ") + hipGetErrorString(e); rc = SURTR_E_HIP; }
    if (rc == SURTR_OK) rc = ct_emit(ctx, W, dev_records, records_bytes);
    if (rc == SURTR_OK) { stamp(4); ctx->contact_ev.valid = prof; }
    if (keep && rc == SURTR_OK) { keep->W = W; keep->base = base; }
    else ct_free(base, st);
    return rc;
}

// One run into a header of the call's own: the totals on the host, the temporaries kept for the records.
int ct_run_host(surtr_ctx* ctx, float margin, DevBuf<surtr_contact>& d_out, CtRun& run, surtr_contact_header& h)
{
    int rc = d_out.grow(ctx, 1);
    if (rc == SURTR_OK) rc = ct_launch(ctx, margin, d_out.p, sizeof(surtr_contact_header), &run);
    if (rc) return rc;
    const hipError_t e = hipMemcpyAsync(&h, d_out.p, sizeof(h), hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(ctx->stream) : e;
    if (e2 != hipSuccess) { ct_free(run.base, ctx->stream); run.base = nullptr; ctx->err = std::string("contacts: ") + hipGetErrorString(e2); return SURTR_E_HIP; }
    return SURTR_OK;
}

} // namespace

extern "C" {

int surtr_scene_contacts_dev(surtr_ctx* ctx, float margin, void* dev_records, size_t records_bytes)
{
    return ct_launch(ctx, margin, dev_records, records_bytes, nullptr);
}

int surtr_scene_contacts_totals(surtr_ctx* ctx, float margin, surtr_contact_header* totals)
{
    int rc = ct_check(ctx, margin);
    if (rc) return rc;
    if (!totals) return SURTR_E_INVALID;
    DevBuf<surtr_contact> d_out;
    CtRun run;
    if ((rc = ct_run_host(ctx, margin, d_out, run, *totals)) != SURTR_OK) return rc;
    ct_free(run.base, ctx->stream);
    if (!totals->lists) totals->status = SURTR_OK;      // (the header alone was asked for: that the records do not fit it is no error)
    return totals->lists ? SURTR_E_CAPACITY : SURTR_OK;
}

int surtr_scene_contacts(surtr_ctx* ctx, float margin, uint32_t* n, surtr_contact* out)
{
    int rc = ct_check(ctx, margin);
    if (rc) return rc;
    if (!n) return SURTR_E_INVALID;
    DevBuf<surtr_contact> d_out;
    CtRun run;
    surtr_contact_header h;
    if ((rc = ct_run_host(ctx, margin, d_out, run, h)) != SURTR_OK) return rc;
    rc = SURTR_OK;
    if (h.lists) rc = SURTR_E_CAPACITY;
    else if (out && *n < h.n_records) { *n = h.n_records; rc = SURTR_E_CAPACITY; }
    else
    {
        *n = h.n_records;
        if (out && h.n_records)
        {
            // the records of the same run: header and gather once more, into room for all of them
            const size_t bytes = ((size_t)h.n_records + 1u) * sizeof(surtr_contact);
            rc = d_out.grow(ctx, (size_t)h.n_records + 1u);
            if (rc == SURTR_OK) rc = ct_emit(ctx, run.W, d_out.p, bytes);
            if (rc == SURTR_OK)
            {
                hipError_t e = hipMemcpyAsync(out, d_out.p + 1, bytes - sizeof(surtr_contact), hipMemcpyDeviceToHost, ctx->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
                if (e != hipSuccess) { ctx->err = std::string("contacts: ") + hipGetErrorString(e); rc = SURTR_E_HIP; }
            }
        }
    }
    ct_free(run.base, ctx->stream);
    return rc;
}

int surtr_scene_contacts_times(surtr_ctx* ctx, float ms[4])
{
    if (!ctx || !ms) return SURTR_E_INVALID;
    for (int i = 0; i < 4; ++i) ms[i] = -1.f;
    (void)hipSetDevice(ctx->device);
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (ctx->contact_ev.valid)
        for (int i = 0; i < 4; ++i) { float t = 0.f; if (hipEventElapsedTime(&t, ctx->contact_ev.e[i], ctx->contact_ev.e[i + 1]) == hipSuccess) ms[i] = t; }
    return SURTR_OK;
}

} // extern "C"
