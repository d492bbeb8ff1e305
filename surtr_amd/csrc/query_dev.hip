// query_dev.hip -- ray cast and sphere overlap on the Convex solids of the resident pieces, on the device: what OnMouseDown asks of
// PhysX (gScene->raycast, gScene->overlap, Src/Surtr.cpp:178-254) to place an impact, once the only copy of the pieces is in HBM.
//
// Definition (so that results can be checked): the faces of a solid are the loops Poly::ExtractFaces walks on the neighbour rings
// (the half-edge rule of ms_next in mass_dev.hip, including its rule for rings that list a neighbour twice); the plane of a face is
// ConstructFacePlane (surtr_plane_from_points) through the loop's smallest-numbered vertex and the two that follow it in loop
// order; inside is n.x + d <= 0.
//   ray     Cyrus-Beck: the interval [0, max_dist] clipped by every half-space; t_enter = max over the planes the ray enters from
//           outside, t_exit = min over the planes it leaves; a parallel plane with the origin outside rejects; hit when
//           t_enter <= t_exit, t = max(t_enter, 0), normal = the entering plane's (the first in plane order on a tie).  Origin
//           inside every half-space: t = 0, position = origin, normal = -d, SURTR_RAY_STARTS_INSIDE.  Over all pieces: the smallest
//           t, the lowest piece on a tie.
//           A piece whose box (of its vertices) the ray does not cross is not hit, one whose box the sphere does not reach is not
//           touched: for a convex solid that changes nothing; it bounds what a face plane taken from three nearly collinear
//           vertices -- a plane far from its face -- can claim.
//   sphere  touched when the distance from the centre to the solid is <= r: 0 inside every half-space, else the minimum over the
//           edges (point to segment) and over the faces whose plane projection of the centre falls inside the face (plane distance);
//           squared distances are compared.
// A solid of fewer than four vertices, with a ring that does not close, a face of zero normal or a loop longer than QR_B is never
// hit and never touched; the per-piece status says which (surtr_pieces_query_status).
//
//   k_qr_planes     one wave per piece: every half-edge walks its loop; the one leaving the loop's smallest vertex emits the plane
//                   (+ that half-edge, for the sphere's face test).  Planes are placed by a scan in (vertex, ring slot) order, so
//                   their order is fixed.  Also the piece's box, from the vertices it reads anyway (PieceSet::box is current after a transform
//                   and after surtr_pieces_from_event -- derive_set recomputes it -- but nothing here depends on that), and its status.
//   k_qr_rays       work item = (ray, block of QR_WG pieces): a lane culls its piece by the box and clips the ray by its planes;
//                   the best (t, piece) -- one 64-bit key -- is reduced by wave shuffles, then over the waves in LDS
//   k_qr_ray_final  one lane per ray: the best key over the blocks -> the record
//   k_qr_overlap    one lane per (sphere, piece)
// Planes, the clip of a ray and the distances of a sphere are computed in double from the float positions (see qr_plane); the
// records are float.  Max, min and lowest-index are order-independent: no atomics on values, the same bits whatever the grid or the stream.  The planes
// are rebuilt by every call into one temporary allocation ordered on the context's stream; the context keeps the status only.
#include <cmath>
#include <cstring>

#include "surtr_ctx.h"

static_assert(sizeof(surtr_ray_hit) == 48 && sizeof(surtr_scene_ray_hit) == 48, "the ray records are 48 bytes");

#define QR_WG SURTR_WG          // threads per workgroup of the query kernels (256; one in the emulation)
#define QR_B 256u               // longest face loop walked
#define QR_NONE 0xFFFFFFFFFFFFFFFFull

namespace {

struct QrSet { const float* pos; const uint32_t* loff; const int32_t* nbr; const uint32_t* vo; uint32_t n; };
struct QrSolid { const float* pos; const uint32_t* loff; const int32_t* nbr; uint32_t nv; };
struct QrPlane { double x, y, z, w; };
struct QrPart { unsigned long long key; float n[3]; uint32_t flags; };      // (a QsPart of the posed ray cast is smaller)

// Scratch of one call (one allocation, carved on the host) + the status the context keeps.
struct QrWork
{
    QrPlane* plane;         // per plane: (n, d), double
    uint2* edge;            // per plane: the emitting half-edge (smallest vertex, its successor)
    uint32_t* pcount;       // per piece: planes (0 for a flagged piece)
    float* box;             // per piece: lo[3], hi[3]
    uint32_t* status;       // per piece: SURTR_QUERY_* bits
    QrPart* part;           // per (ray, block of pieces)
};

__device__ __forceinline__ QrSolid qr_solid(const QrSet& s, uint32_t p)
{
    const uint32_t a = s.vo[p];
    return QrSolid{s.pos + 3 * (size_t)a, s.loff + a, s.nbr, s.vo[p + 1] - a};
}
// Piece p's planes start at (its first ring entry) / 3 + p: a face has at least three half-edges, so the regions cannot meet.
__device__ __forceinline__ uint32_t qr_base(const QrSet& s, uint32_t p) { return s.loff[s.vo[p]] / 3u + p; }

__device__ __forceinline__ bool qr_finite(float x) { return fabsf(x) <= 3.4028235e38f; }

// Half-edge (u -> w) -> the vertex after w on its face: the ring entry of w listed just before u (FaceLoop, Src/Poly.cpp:34-41).
__device__ __forceinline__ uint32_t qr_next(const QrSolid& S, uint32_t u, uint32_t w, bool& bad)
{
    const int32_t* r = S.nbr + S.loff[w];
    const uint32_t n = S.loff[w + 1] - S.loff[w];
    if (n == 0u) { bad = true; return 0xFFFFFFFFu; }
    uint32_t k = 0;
    while (k < n && (uint32_t)r[k] != u) ++k;
    if (k == n) bad = true;
    return (uint32_t)r[(k == 0u || k == n) ? n - 1u : k - 1u];
}
// A ring that lists a neighbour twice: the later slot starts no face of its own (ExtractFaces keys by the first slot).
__device__ __forceinline__ bool qr_repeat(const int32_t* r, uint32_t s)
{
    for (uint32_t q = 0; q < s; ++q) if (r[q] == r[s]) return true;
    return false;
}

// Walks the loop of half-edge (v -> w).  0: closed, *m = its smallest vertex, *x1 = the vertex after w; else the status bit.
__device__ __forceinline__ uint32_t qr_walk(const QrSolid& S, uint32_t v, uint32_t w, uint32_t* m, uint32_t* x1)
{
    uint32_t prev = v, cur = w, mn = v;
    bool bad = false;
    for (uint32_t k = 1; k <= QR_B; ++k)
    {
        const uint32_t x = qr_next(S, prev, cur, bad);
        if (bad || x >= S.nv) return SURTR_QUERY_OPEN;
        if (k == 1u) *x1 = x;
        prev = cur; cur = x;
        if (prev == v && cur == w) { *m = mn; return k < 3u ? SURTR_QUERY_OPEN : 0u; }
        mn = prev < mn ? prev : mn;
    }
    return SURTR_QUERY_LONG;
}

// ConstructFacePlane (surtr_plane_from_points) in double.  The float positions convert exactly, so the plane is the definition's
// to 1e-16: where the loop's second and third vertex all but coincide (fragments do have vertices 1e-6 apart) the float
// routine's normal is off by tenths, and no tolerance on the hit could tell a wrong plane from a rounded one.
__device__ __forceinline__ QrPlane qr_plane(const float* p0, const float* p1, const float* p2)
{
    const double ax = (double)p1[0] - (double)p0[0], ay = (double)p1[1] - (double)p0[1], az = (double)p1[2] - (double)p0[2];
    const double bx = (double)p2[0] - (double)p0[0], by = (double)p2[1] - (double)p0[1], bz = (double)p2[2] - (double)p0[2];
    double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    if (len != 0.0) { nx = nx / len; ny = ny / len; nz = nz / len; } else { nx = 0.0; ny = 0.0; nz = 0.0; }
    return QrPlane{nx, ny, nz, -(nx * (double)p0[0] + ny * (double)p0[1] + nz * (double)p0[2])};
}

__global__ __launch_bounds__(SURTR_LANES) void k_qr_planes(QrSet set, QrWork W)
{
    const uint32_t l = lane_id();
    for (uint32_t p = blockIdx.x; p < set.n; p += gridDim.x)
    {
        const QrSolid S = qr_solid(set, p);
        const uint32_t base = qr_base(set, p), cap = set.loff[set.vo[p + 1]] / 3u + p + 1u - base;
        uint32_t st = S.nv < 4u ? SURTR_QUERY_FEW : 0u, run = 0;      // (the same in every lane until the reduction below)
        float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
        uint32_t flt = 0;
        for (uint32_t v0 = 0; st == 0u && v0 < S.nv; v0 += SURTR_LANES)
        {
            const uint32_t v = v0 + l;
            const int32_t* r = v < S.nv ? S.nbr + S.loff[v] : nullptr;
            const uint32_t len = v < S.nv ? S.loff[v + 1] - S.loff[v] : 0u;
            uint32_t cnt = 0, mine = 0, at = 0;
            if (v < S.nv)
                for (int c = 0; c < 3; ++c) { const float x = S.pos[3 * (size_t)v + c]; lo[c] = fminf(lo[c], x); hi[c] = fmaxf(hi[c], x); if (!qr_finite(x)) mine |= SURTR_QUERY_OPEN; }
            for (int pass = 0; pass < 2; ++pass)
            {
                for (uint32_t s = 0; s < len; ++s)
                {
                    const uint32_t w = (uint32_t)r[s];
                    if (w >= S.nv) { mine |= SURTR_QUERY_OPEN; continue; }
                    if (qr_repeat(r, s)) continue;
                    uint32_t m = 0, x1 = 0;
                    const uint32_t rc = qr_walk(S, v, w, &m, &x1);
                    if (rc) { mine |= rc; continue; }
                    if (m != v) continue;
                    if (pass == 0) { ++cnt; continue; }
                    const QrPlane pl = qr_plane(S.pos + 3 * (size_t)v, S.pos + 3 * (size_t)w, S.pos + 3 * (size_t)x1);
                    if (pl.x == 0.0 && pl.y == 0.0 && pl.z == 0.0) mine |= SURTR_QUERY_FLAT;
                    if (at < cap) { W.plane[base + at] = pl; W.edge[base + at] = make_uint2(v, w); }
                    else mine |= SURTR_QUERY_OPEN;
                    ++at;
                }
                if (pass == 1) break;
                uint32_t inc = cnt;      // exclusive scan over the lanes: planes in (vertex, ring slot) order
                for (uint32_t o = 1; o < SURTR_LANES; o <<= 1) { const uint32_t t = __shfl_up(inc, o, SURTR_LANES); if (l >= o) inc += t; }
                at = run + inc - cnt;
                run += __shfl(inc, SURTR_LANES - 1, SURTR_LANES);
            }
            flt |= mine;
        }
        st |= flt;
        for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1)
        {
            st |= __shfl_down(st, o, SURTR_LANES);
            for (int c = 0; c < 3; ++c) { lo[c] = fminf(lo[c], __shfl_down(lo[c], o, SURTR_LANES)); hi[c] = fmaxf(hi[c], __shfl_down(hi[c], o, SURTR_LANES)); }
        }
        if (l == 0u)
        {
            W.status[p] = st;
            W.pcount[p] = st ? 0u : (run < cap ? run : cap);
            for (int c = 0; c < 3; ++c)
            {
                W.box[6 * (size_t)p + c] = lo[c]; W.box[6 * (size_t)p + 3 + c] = hi[c];
            }
        }
    }
}

__device__ __forceinline__ bool qr_ray_ok(const float* q)
{
    for (int c = 0; c < 7; ++c) if (!qr_finite(q[c]) && !(c == 6 && q[6] > 0.f)) return false;      // (max_dist may be +inf)
    return (q[3] != 0.f || q[4] != 0.f || q[5] != 0.f) && q[6] >= 0.f;
}

// The ray against one box: false when the slabs leave nothing of [0, max_dist].
template <class T>
__device__ __forceinline__ bool qr_ray_box(const T* q, const float* box)
{
    double t0 = 0.0, t1 = (double)q[6];
    for (int c = 0; c < 3; ++c)
    {
        const double o = q[c], d = q[3 + c], lo = box[c], hi = box[3 + c];
        if (d == 0.0) { if (o < lo || o > hi) return false; continue; }
        double a = (lo - o) / d, b = (hi - o) / d;
        if (a > b) { const double t = a; a = b; b = t; }
        t0 = fmax(t0, a); t1 = fmin(t1, b);
    }
    return t0 <= t1;
}

// Cyrus-Beck of one ray against the planes of one piece (double: the same numbers as the definition evaluated in float64).
// The ray comes as float (world frame) or as double (taken into a body frame); *ent_out = the entering plane, -1 from inside.
template <class T>
__device__ __forceinline__ bool qr_ray_clip(const T* q, const QrPlane* pl, uint32_t np, float* t_out, int* ent_out, uint32_t* flags)
{
    const double ox = q[0], oy = q[1], oz = q[2], dx = q[3], dy = q[4], dz = q[5];
    double t_in = 0.0, t_ex = (double)q[6];
    int ent = -1;
    bool inside = true;
    for (uint32_t k = 0; k < np; ++k)
    {
        const QrPlane P = pl[k];
        const double den = P.x * dx + P.y * dy + P.z * dz;
        const double dist = P.x * ox + P.y * oy + P.z * oz + P.w;
        if (dist > 0.0) inside = false;
        if (den == 0.0) { if (dist > 0.0) return false; continue; }
        const double t = -dist / den;
        if (den < 0.0) { if (dist > 0.0 && (ent < 0 || t > t_in)) { t_in = t; ent = (int)k; } }
        else t_ex = fmin(t_ex, t);
    }
    if (np == 0u || !(t_in <= t_ex)) return false;
    if (inside) { *t_out = 0.f; *ent_out = -1; *flags = SURTR_RAY_STARTS_INSIDE; return true; }
    if (ent < 0) return false;
    *t_out = (float)t_in; *ent_out = ent; *flags = 0u;
    return true;
}
__device__ __forceinline__ bool qr_ray_piece(const float* q, const QrPlane* pl, uint32_t np, float* t_out, float* nrm, uint32_t* flags)
{
    int ent;
    if (!qr_ray_clip(q, pl, np, t_out, &ent, flags)) return false;
    if (ent < 0) { nrm[0] = -q[3]; nrm[1] = -q[4]; nrm[2] = -q[5]; }
    else { nrm[0] = (float)pl[ent].x; nrm[1] = (float)pl[ent].y; nrm[2] = (float)pl[ent].z; }
    return true;
}

__global__ __launch_bounds__(QR_WG) void k_qr_rays(QrSet set, QrWork W, uint32_t n_rays, const float* __restrict__ rays, uint32_t nblk)
{
    __shared__ unsigned long long red[QR_WG / SURTR_LANES + 1];
    const uint32_t total = n_rays * nblk;
    for (uint32_t item = blockIdx.x; item < total; item += gridDim.x)
    {
        const uint32_t ray = item / nblk, p = (item % nblk) * group_size() + threadIdx.x;
        float q[7];
        for (int c = 0; c < 7; ++c) q[c] = rays[7 * (size_t)ray + c];
        unsigned long long key = QR_NONE;
        float nrm[3] = {0.f, 0.f, 0.f}, t = 0.f;
        uint32_t flags = 0;
        if (qr_ray_ok(q) && p < set.n && W.pcount[p] != 0u && qr_ray_box(q, W.box + 6 * (size_t)p) &&
            qr_ray_piece(q, W.plane + qr_base(set, p), W.pcount[p], &t, nrm, &flags))
            key = ((unsigned long long)__float_as_uint(t) << 32) | p;
        unsigned long long best = key;
        for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1) { const unsigned long long x = __shfl_down(best, o, SURTR_LANES); best = x < best ? x : best; }
        if (lane_id() == 0u) red[wave_id()] = best;
        __syncthreads();
        best = red[0];
        for (uint32_t w = 1; w < group_waves(); ++w) best = red[w] < best ? red[w] : best;
        // the key holds the piece: exactly one lane has the best one
        if (best == QR_NONE ? threadIdx.x == 0u : key == best)
        {
            QrPart r;
            r.key = best; r.n[0] = nrm[0]; r.n[1] = nrm[1]; r.n[2] = nrm[2]; r.flags = flags;
            W.part[item] = r;
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(QR_WG) void k_qr_ray_final(QrWork W, uint32_t n_rays, const float* __restrict__ rays, uint32_t nblk, surtr_ray_hit* __restrict__ out)
{
    for (uint32_t ray = blockIdx.x * blockDim.x + threadIdx.x; ray < n_rays; ray += gridDim.x * blockDim.x)
    {
        float q[7];
        for (int c = 0; c < 7; ++c) q[c] = rays[7 * (size_t)ray + c];
        surtr_ray_hit h;
        memset(&h, 0, sizeof(h));
        h.piece = -1;
        if (!qr_ray_ok(q)) { h.status = SURTR_RAY_INVALID; out[ray] = h; continue; }
        uint32_t bb = 0;
        unsigned long long best = QR_NONE;
        for (uint32_t b = 0; b < nblk; ++b) { const unsigned long long k = W.part[(size_t)ray * nblk + b].key; if (k < best) { best = k; bb = b; } }
        if (best != QR_NONE)
        {
            const QrPart r = W.part[(size_t)ray * nblk + bb];
            h.piece = (int32_t)(uint32_t)best; h.t = __uint_as_float((uint32_t)(best >> 32)); h.status = r.flags;
            for (int c = 0; c < 3; ++c) { h.pos[c] = q[c] + q[3 + c] * h.t; h.normal[c] = r.n[c]; }
        }
        out[ray] = h;
    }
}

// Squared distance from c to the segment a b.
__device__ __forceinline__ double qr_seg2(const double* c, const float* a, const float* b)
{
    const double ex = (double)b[0] - (double)a[0], ey = (double)b[1] - (double)a[1], ez = (double)b[2] - (double)a[2];
    const double hx = c[0] - (double)a[0], hy = c[1] - (double)a[1], hz = c[2] - (double)a[2];
    const double ee = ex * ex + ey * ey + ez * ez, eh = ex * hx + ey * hy + ez * hz;
    double s = ee > 0.0 ? eh / ee : 0.0;
    s = s < 0.0 ? 0.0 : (s > 1.0 ? 1.0 : s);
    const double dx = hx - s * ex, dy = hy - s * ey, dz = hz - s * ez;
    return dx * dx + dy * dy + dz * dz;
}

template <class T>
__device__ bool qr_sphere_piece(const QrSolid& S, const T* sp, const QrPlane* pl, const uint2* edge, uint32_t np, const float* box)
{
    const double c[3] = {sp[0], sp[1], sp[2]}, r2 = (double)sp[3] * (double)sp[3];
    double b2 = 0.0;      // the box first
    for (int k = 0; k < 3; ++k) { const double e = c[k] < box[k] ? box[k] - c[k] : (c[k] > box[3 + k] ? c[k] - box[3 + k] : 0.0); b2 = b2 + e * e; }
    if (b2 > r2 || np == 0u) return false;
    bool inside = true;
    double best = INFINITY;
    for (uint32_t k = 0; k < np; ++k)
    {
        const QrPlane P = pl[k];
        const double dist = P.x * c[0] + P.y * c[1] + P.z * c[2] + P.w;
        if (!(dist > 0.0)) continue;
        inside = false;
        if (!(dist * dist < best)) continue;
        // the projection of the centre onto the plane, against every edge of the face
        const double qx = c[0] - dist * P.x, qy = c[1] - dist * P.y, qz = c[2] - dist * P.z;
        uint32_t prev = edge[k].x, cur = edge[k].y;
        bool in_face = true, bad = false;
        for (uint32_t j = 0; j < QR_B; ++j)
        {
            const float* a = S.pos + 3 * (size_t)prev; const float* b = S.pos + 3 * (size_t)cur;
            const double ex = (double)b[0] - (double)a[0], ey = (double)b[1] - (double)a[1], ez = (double)b[2] - (double)a[2];
            const double hx = qx - (double)a[0], hy = qy - (double)a[1], hz = qz - (double)a[2];
            const double side = (ey * hz - ez * hy) * P.x + (ez * hx - ex * hz) * P.y + (ex * hy - ey * hx) * P.z;
            if (side < 0.0) { in_face = false; break; }
            const uint32_t x = qr_next(S, prev, cur, bad);
            if (bad || x >= S.nv) { in_face = false; break; }
            prev = cur; cur = x;
            if (prev == edge[k].x && cur == edge[k].y) break;
        }
        if (in_face) best = dist * dist;
    }
    if (inside) return true;
    for (uint32_t v = 0; v < S.nv; ++v)
    {
        const int32_t* r = S.nbr + S.loff[v];
        const uint32_t len = S.loff[v + 1] - S.loff[v];
        for (uint32_t s = 0; s < len; ++s)
        {
            const uint32_t w = (uint32_t)r[s];
            if (w <= v || w >= S.nv) continue;      // every edge once
            const double d2 = qr_seg2(c, S.pos + 3 * (size_t)v, S.pos + 3 * (size_t)w);
            best = d2 < best ? d2 : best;
        }
    }
    return best <= r2;
}

__global__ __launch_bounds__(QR_WG) void k_qr_overlap(QrSet set, QrWork W, uint32_t n_sph, const float* __restrict__ sph, const surtr_mass* __restrict__ mass,
                                                      double min_mass, uint8_t* __restrict__ mask)
{
    const size_t total = (size_t)n_sph * set.n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    {
        const uint32_t s = (uint32_t)(i / set.n), p = (uint32_t)(i % set.n);
        float sp[4];
        for (int c = 0; c < 4; ++c) sp[c] = sph[4 * (size_t)s + c];
        uint8_t m = 0;
        const bool ok = qr_finite(sp[0]) && qr_finite(sp[1]) && qr_finite(sp[2]) && qr_finite(sp[3]) && sp[3] >= 0.f;
        if (ok && W.pcount[p] != 0u && qr_sphere_piece(qr_solid(set, p), sp, W.plane + qr_base(set, p), W.edge + qr_base(set, p), W.pcount[p], W.box + 6 * (size_t)p))
            m = (mass && mass[p].mass <= min_mass) ? 2 : 1;
        mask[i] = m;
    }
}

// ---- the same queries on a scene whose bodies have poses (surtr_scene_set_poses): piece p of compound c with pose (A, b) is
// asked in its body frame, o' = A^T (o - b), d' = A^T d, c' = A^T (c - b), in double from the floats; planes, boxes and solids stay as
// they are resident, so a pose change costs an upload of 96 bytes per body and nothing else.  t is the same number in both frames.
struct QsPart { unsigned long long key; uint32_t plane, flags; };      // plane: index of the entering plane in QrWork::plane
static_assert(sizeof(QsPart) <= sizeof(QrPart), "the posed ray cast keeps its parts in the room QrWork::part has");

// m = A^T row-major (9), b (3).  With the identity every product is x * 1 or x * 0: the body-frame numbers are the world's.
__device__ __forceinline__ void qs_to_body(const double* m, const float* x, bool point, double* out)
{
    const double hx = point ? (double)x[0] - m[9] : (double)x[0], hy = point ? (double)x[1] - m[10] : (double)x[1],
                 hz = point ? (double)x[2] - m[11] : (double)x[2];
    for (int r = 0; r < 3; ++r) out[r] = m[3 * r] * hx + m[3 * r + 1] * hy + m[3 * r + 2] * hz;
}

// As k_qr_rays; a lane reads its piece's compound and that compound's 12 doubles.  The pieces of a compound are contiguous, so the
// lanes of a wave mostly read the same 96 bytes: the loads stay per lane (lanes with one address share one request, and the table of
// a few thousand bodies stays in L2), no wave-uniform special case.
__global__ __launch_bounds__(QR_WG) void k_qs_rays(QrSet set, QrWork W, SceneDev sc, uint32_t n_rays, const float* __restrict__ rays, uint32_t nblk)
{
    __shared__ unsigned long long red[QR_WG / SURTR_LANES + 1];
    const uint32_t total = n_rays * nblk;
    QsPart* part = (QsPart*)W.part;
    for (uint32_t item = blockIdx.x; item < total; item += gridDim.x)
    {
        const uint32_t ray = item / nblk, p = (item % nblk) * group_size() + threadIdx.x;
        float q[7];
        for (int c = 0; c < 7; ++c) q[c] = rays[7 * (size_t)ray + c];
        unsigned long long key = QR_NONE;
        float t = 0.f;
        uint32_t flags = 0, plane = 0;
        if (qr_ray_ok(q) && p < set.n && W.pcount[p] != 0u)
        {
            const double* m = sc.pose + 12 * (size_t)sc.piece_comp[p];
            double b[7];
            qs_to_body(m, q, true, b); qs_to_body(m, q + 3, false, b + 3); b[6] = (double)q[6];
            int ent = -1;
            const uint32_t base = qr_base(set, p);
            if (qr_ray_box(b, W.box + 6 * (size_t)p) && qr_ray_clip(b, W.plane + base, W.pcount[p], &t, &ent, &flags))
            {
                key = ((unsigned long long)__float_as_uint(t) << 32) | p;
                plane = ent < 0 ? 0u : base + (uint32_t)ent;
            }
        }
        unsigned long long best = key;
        for (uint32_t o = SURTR_LANES / 2u; o > 0u; o >>= 1) { const unsigned long long x = __shfl_down(best, o, SURTR_LANES); best = x < best ? x : best; }
        if (lane_id() == 0u) red[wave_id()] = best;
        __syncthreads();
        best = red[0];
        for (uint32_t w = 1; w < group_waves(); ++w) best = red[w] < best ? red[w] : best;
        if (best == QR_NONE ? threadIdx.x == 0u : key == best)
        {
            QsPart r;
            r.key = best; r.plane = plane; r.flags = flags;
            part[item] = r;
        }
        __syncthreads();
    }
}

// One lane per ray: the best key over the blocks; the normal goes back to the world, n = A n' in double, rounded, not renormalised.
__global__ __launch_bounds__(QR_WG) void k_qs_ray_final(QrWork W, SceneDev sc, uint32_t n_rays, const float* __restrict__ rays, uint32_t nblk,
                                                        surtr_scene_ray_hit* __restrict__ out)
{
    const QsPart* part = (const QsPart*)W.part;
    for (uint32_t ray = blockIdx.x * blockDim.x + threadIdx.x; ray < n_rays; ray += gridDim.x * blockDim.x)
    {
        float q[7];
        for (int c = 0; c < 7; ++c) q[c] = rays[7 * (size_t)ray + c];
        surtr_scene_ray_hit h;
        memset(&h, 0, sizeof(h));
        h.piece = -1; h.compound = -1;
        if (!qr_ray_ok(q)) { h.status = SURTR_RAY_INVALID; out[ray] = h; continue; }
        uint32_t bb = 0;
        unsigned long long best = QR_NONE;
        for (uint32_t b = 0; b < nblk; ++b) { const unsigned long long k = part[(size_t)ray * nblk + b].key; if (k < best) { best = k; bb = b; } }
        if (best != QR_NONE)
        {
            const QsPart r = part[(size_t)ray * nblk + bb];
            h.piece = (int32_t)(uint32_t)best; h.t = __uint_as_float((uint32_t)(best >> 32)); h.status = r.flags;
            h.compound = (int32_t)sc.piece_comp[(uint32_t)best];
            for (int c = 0; c < 3; ++c) h.pos[c] = q[c] + q[3 + c] * h.t;
            if (r.flags & SURTR_RAY_STARTS_INSIDE) { for (int c = 0; c < 3; ++c) h.normal[c] = -q[3 + c]; }
            else
            {
                const double* m = sc.pose + 12 * (size_t)h.compound;      // A[c][k] = m[3 k + c]
                const QrPlane P = W.plane[r.plane];
                for (int c = 0; c < 3; ++c) h.normal[c] = (float)(m[c] * P.x + m[3 + c] * P.y + m[6 + c] * P.z);
            }
        }
        out[ray] = h;
    }
}

// One lane per (sphere, piece): the piece's byte, 0 or 1, with no gate.
__global__ __launch_bounds__(QR_WG) void k_qs_overlap(QrSet set, QrWork W, SceneDev sc, uint32_t n_sph, const float* __restrict__ sph, uint8_t* __restrict__ mask)
{
    const size_t total = (size_t)n_sph * set.n;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x)
    {
        const uint32_t s = (uint32_t)(i / set.n), p = (uint32_t)(i % set.n);
        float sp[4];
        for (int c = 0; c < 4; ++c) sp[c] = sph[4 * (size_t)s + c];
        uint8_t m = 0;
        const bool ok = qr_finite(sp[0]) && qr_finite(sp[1]) && qr_finite(sp[2]) && qr_finite(sp[3]) && sp[3] >= 0.f;
        if (ok && W.pcount[p] != 0u)
        {
            double b[4];
            qs_to_body(sc.pose + 12 * (size_t)sc.piece_comp[p], sp, true, b); b[3] = (double)sp[3];
            if (qr_sphere_piece(qr_solid(set, p), b, W.plane + qr_base(set, p), W.edge + qr_base(set, p), W.pcount[p], W.box + 6 * (size_t)p)) m = 1;
        }
        mask[i] = m;
    }
}

// One wave per (sphere, compound): the OR of its pieces' bytes by ballot, then the gate on the body's mass (Src/Surtr.cpp:228):
// 0 untouched, 1 touched, 2 touched but mass <= min_mass.
__global__ __launch_bounds__(QR_WG) void k_qs_bodies(SceneDev sc, uint32_t n_pieces, uint32_t n_sph, const uint8_t* __restrict__ mask,
                                                     const surtr_mass* __restrict__ mass, double min_mass, uint8_t* __restrict__ body)
{
    const size_t total = (size_t)n_sph * sc.n_comp;
    for (size_t item = (size_t)blockIdx.x * group_waves() + wave_id(); item < total; item += (size_t)gridDim.x * group_waves())
    {
        const uint32_t s = (uint32_t)(item / sc.n_comp), c = (uint32_t)(item % sc.n_comp);
        bool any = false;
        for (uint32_t p = sc.comp_off[c] + lane_id(); p < sc.comp_off[c + 1]; p += SURTR_LANES) any = any || mask[(size_t)s * n_pieces + p] != 0;
        const bool touched = __ballot(any) != 0ull;
        if (lane_id() == 0u) body[item] = !touched ? 0 : ((mass && mass[c].mass <= min_mass) ? 2 : 1);
    }
}

hipError_t qr_alloc(void** p, size_t bytes, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    return hipMallocAsync(p, bytes, st);
#else
    (void)st;
    return hipMalloc(p, bytes);
#endif
}
void qr_free(void* p, hipStream_t st)
{
#ifdef __HIP_PLATFORM_AMD__
    (void)hipFreeAsync(p, st);
#else
    (void)st;
    (void)hipFree(p);
#endif
}

// Pass 1 + one of the two second passes.  rays != nullptr: ray cast into hits; else the spheres into mask.
// sc != nullptr: the posed forms -- hits are surtr_scene_ray_hit; d_mask (may be nullptr: scratch) takes the piece bytes, d_body the
// bodies', gated by d_mass (one record per compound).
int qr_launch(surtr_ctx* ctx, uint32_t nq, const float* d_rays, void* d_hits, const float* d_sph, const surtr_mass* d_mass,
              float min_mass, uint8_t* d_mask, const SceneDev* sc = nullptr, uint8_t* d_body = nullptr)
{
    const PieceSet& P = ctx->cset;
    const uint32_t n = ctx->n_pieces;
    hipStream_t st = ctx->stream;
    const uint32_t nblk = (n + QR_WG - 1u) / QR_WG;
    if (d_rays && (uint64_t)nq * nblk > 0x7FFFFFFFull) { ctx->err = "query: too many rays for one call"; return SURTR_E_CAPACITY; }
    int rc = ctx->d_qstatus.grow(ctx, n);
    if (rc) return rc;
    ctx->qstatus_n = n;
    const size_t pcap = P.nbr.cap / 3u + (size_t)n + 2u;
    size_t bytes = 0;
    auto take = [&](size_t b) { const size_t at = bytes; bytes += (b + 15u) & ~(size_t)15u; return at; };
    const size_t o_plane = take(pcap * sizeof(QrPlane)), o_edge = take(pcap * sizeof(uint2)), o_cnt = take((size_t)n * 4),
                 o_box = take((size_t)n * 24), o_part = take(d_rays ? (size_t)nq * nblk * sizeof(QrPart) : 0),
                 o_pmask = take(sc && !d_rays && !d_mask ? (size_t)nq * n : 0);
    char* base = nullptr;
    HIPCHK(qr_alloc((void**)&base, bytes, st));
    QrWork W;
    W.plane = (QrPlane*)(base + o_plane); W.edge = (uint2*)(base + o_edge); W.pcount = (uint32_t*)(base + o_cnt);
    W.box = (float*)(base + o_box); W.part = (QrPart*)(base + o_part); W.status = ctx->d_qstatus;
    QrSet S{P.pos, P.loff, P.nbr, P.vo, n};
    hipLaunchKernelGGL(k_qr_planes, dim3(std::min(n, 65536u)), dim3(SURTR_LANES), 0, st, S, W);
    if (sc && d_rays)
    {
        hipLaunchKernelGGL(k_qs_rays, dim3(std::min(nq * nblk, 1u << 20)), dim3(QR_WG), 0, st, S, W, *sc, nq, d_rays, nblk);
        hipLaunchKernelGGL(k_qs_ray_final, dim3(std::min((nq + QR_WG - 1u) / QR_WG, 4096u)), dim3(QR_WG), 0, st, W, *sc, nq, d_rays, nblk,
                           (surtr_scene_ray_hit*)d_hits);
    }
    else if (sc)
    {
        const size_t total = (size_t)nq * n, waves = (size_t)nq * sc->n_comp, per = QR_WG / SURTR_LANES;
        uint8_t* pm = d_mask ? d_mask : (uint8_t*)(base + o_pmask);
        hipLaunchKernelGGL(k_qs_overlap, dim3((uint32_t)std::min<size_t>((total + QR_WG - 1u) / QR_WG, (size_t)1 << 20)), dim3(QR_WG), 0, st, S, W, *sc, nq,
                           d_sph, pm);
        hipLaunchKernelGGL(k_qs_bodies, dim3((uint32_t)std::min<size_t>((waves + per - 1u) / per, (size_t)1 << 20)), dim3(QR_WG), 0, st, *sc, n, nq, pm,
                           d_mass, (double)min_mass, d_body);
    }
    else if (d_rays)
    {
        hipLaunchKernelGGL(k_qr_rays, dim3(std::min(nq * nblk, 1u << 20)), dim3(QR_WG), 0, st, S, W, nq, d_rays, nblk);
        hipLaunchKernelGGL(k_qr_ray_final, dim3(std::min((nq + QR_WG - 1u) / QR_WG, 4096u)), dim3(QR_WG), 0, st, W, nq, d_rays, nblk, (surtr_ray_hit*)d_hits);
    }
    else
    {
        const size_t total = (size_t)nq * n;
        hipLaunchKernelGGL(k_qr_overlap, dim3((uint32_t)std::min<size_t>((total + QR_WG - 1u) / QR_WG, (size_t)1 << 20)), dim3(QR_WG), 0, st, S, W, nq,
                           d_sph, d_mass, (double)min_mass, d_mask);
    }
    const hipError_t e = hipGetLastError();
    qr_free(base, st);
    if (e != hipSuccess) { ctx->err = std::string("query: ") + hipGetErrorString(e); return SURTR_E_HIP; }
    return SURTR_OK;
}

int qr_state(surtr_ctx* ctx)
{
    const PieceSet& P = ctx->cset;
    return (!P.pos || !P.vo || !P.loff || !P.nbr || ctx->n_pieces == 0) ? SURTR_E_STATE : SURTR_OK;
}

bool qr_host_finite(float x) { return std::fabs(x) <= 3.4028235e38f; }

} // namespace

extern "C" int surtr_pieces_raycast_dev(surtr_ctx* ctx, uint32_t n_rays, const float* dev_rays, void* dev_hits, size_t capacity_bytes)
{
    if (!ctx || !dev_rays || !dev_hits || n_rays == 0) return SURTR_E_INVALID;
    if (qr_state(ctx)) return SURTR_E_STATE;
    if ((size_t)n_rays * sizeof(surtr_ray_hit) > capacity_bytes) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    return qr_launch(ctx, n_rays, dev_rays, (surtr_ray_hit*)dev_hits, nullptr, nullptr, 0.f, nullptr);
}

extern "C" int surtr_pieces_overlap_dev(surtr_ctx* ctx, uint32_t n_spheres, const float* dev_spheres, const void* dev_mass_or_null, float min_mass,
                                        uint8_t* dev_mask, size_t capacity_bytes)
{
    if (!ctx || !dev_spheres || !dev_mask || n_spheres == 0) return SURTR_E_INVALID;
    if (qr_state(ctx)) return SURTR_E_STATE;
    if ((size_t)n_spheres * ctx->n_pieces > capacity_bytes) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    return qr_launch(ctx, n_spheres, nullptr, nullptr, dev_spheres, (const surtr_mass*)dev_mass_or_null, min_mass, dev_mask);
}

extern "C" int surtr_pieces_raycast(surtr_ctx* ctx, uint32_t n_rays, const float* rays, surtr_ray_hit* hits)
{
    if (!ctx || !rays || !hits || n_rays == 0) return SURTR_E_INVALID;
    if (qr_state(ctx)) return SURTR_E_STATE;
    for (uint32_t i = 0; i < n_rays; ++i)
    {
        const float* q = rays + 7 * (size_t)i;
        for (int c = 0; c < 6; ++c) if (!qr_host_finite(q[c])) return SURTR_E_INVALID;
        if ((q[3] == 0.f && q[4] == 0.f && q[5] == 0.f) || !(q[6] >= 0.f)) return SURTR_E_INVALID;
    }
    (void)hipSetDevice(ctx->device);
    DevBuf<float> d_r; DevBuf<surtr_ray_hit> d_h;
    int rc = d_r.grow(ctx, 7 * (size_t)n_rays);
    if (rc == SURTR_OK) rc = d_h.grow(ctx, n_rays);
    if (rc == SURTR_OK && hipMemcpyAsync(d_r.p, rays, 28 * (size_t)n_rays, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    if (rc == SURTR_OK) rc = surtr_pieces_raycast_dev(ctx, n_rays, d_r.p, d_h.p, (size_t)n_rays * sizeof(surtr_ray_hit));
    if (rc == SURTR_OK && hipMemcpyAsync(hits, d_h.p, (size_t)n_rays * sizeof(surtr_ray_hit), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == SURTR_OK) rc = SURTR_E_HIP;
    return rc;
}

extern "C" int surtr_pieces_overlap(surtr_ctx* ctx, uint32_t n_spheres, const float* spheres, const surtr_mass* mass_or_null, float min_mass,
                                    uint32_t* n_pieces, uint8_t* mask)
{
    if (!ctx || !n_pieces) return SURTR_E_INVALID;
    if (qr_state(ctx)) return SURTR_E_STATE;
    const uint32_t n = ctx->n_pieces;
    if (!mask) { *n_pieces = n; return SURTR_OK; }
    if (!spheres || n_spheres == 0) return SURTR_E_INVALID;
    if (*n_pieces < n) { *n_pieces = n; return SURTR_E_CAPACITY; }
    *n_pieces = n;
    for (uint32_t i = 0; i < 4u * n_spheres; ++i) if (!qr_host_finite(spheres[i])) return SURTR_E_INVALID;
    for (uint32_t i = 0; i < n_spheres; ++i) if (!(spheres[4 * (size_t)i + 3] >= 0.f)) return SURTR_E_INVALID;
    (void)hipSetDevice(ctx->device);
    const size_t total = (size_t)n_spheres * n;
    DevBuf<float> d_s; DevBuf<uint8_t> d_m; DevBuf<surtr_mass> d_w;
    int rc = d_s.grow(ctx, 4 * (size_t)n_spheres);
    if (rc == SURTR_OK) rc = d_m.grow(ctx, total);
    if (rc == SURTR_OK && mass_or_null) rc = d_w.grow(ctx, n);
    if (rc == SURTR_OK && hipMemcpyAsync(d_s.p, spheres, 16 * (size_t)n_spheres, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    if (rc == SURTR_OK && mass_or_null && hipMemcpyAsync(d_w.p, mass_or_null, (size_t)n * sizeof(surtr_mass), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    if (rc == SURTR_OK) rc = surtr_pieces_overlap_dev(ctx, n_spheres, d_s.p, mass_or_null ? d_w.p : nullptr, min_mass, d_m.p, total);
    if (rc == SURTR_OK && hipMemcpyAsync(mask, d_m.p, total, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == SURTR_OK) rc = SURTR_E_HIP;
    return rc;
}

extern "C" int surtr_pieces_query_status(surtr_ctx* ctx, uint32_t n, uint32_t* status)
{
    if (!ctx || !status) return SURTR_E_INVALID;
    if (!ctx->d_qstatus || ctx->qstatus_n == 0) return SURTR_E_STATE;
    if (n < ctx->qstatus_n) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    HIPCHK(hipMemcpyAsync(status, ctx->d_qstatus.p, (size_t)ctx->qstatus_n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SURTR_OK;
}

// ---- the posed forms (see include/surtr_hip.h)
extern "C" int surtr_scene_raycast_dev(surtr_ctx* ctx, uint32_t n_rays, const float* dev_rays, void* dev_hits, size_t capacity_bytes)
{
    if (!ctx || !dev_rays || !dev_hits || n_rays == 0) return SURTR_E_INVALID;
    if (qr_state(ctx)) return SURTR_E_STATE;
    if ((size_t)n_rays * sizeof(surtr_scene_ray_hit) > capacity_bytes) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    SceneDev sc;
    const int rc = scene_sync_device(ctx, &sc);
    if (rc) return rc;
    return qr_launch(ctx, n_rays, dev_rays, dev_hits, nullptr, nullptr, 0.f, nullptr, &sc, nullptr);
}

extern "C" int surtr_scene_overlap_dev(surtr_ctx* ctx, uint32_t n_spheres, const float* dev_spheres, const void* dev_body_mass_or_null, float min_mass,
                                       uint8_t* dev_piece_mask_or_null, size_t piece_cap, uint8_t* dev_body_mask, size_t body_cap)
{
    if (!ctx || !dev_spheres || !dev_body_mask || n_spheres == 0) return SURTR_E_INVALID;
    if (qr_state(ctx) || ctx->scene_off.size() < 2) return SURTR_E_STATE;
    if ((dev_piece_mask_or_null && (size_t)n_spheres * ctx->n_pieces > piece_cap) || (size_t)n_spheres * (ctx->scene_off.size() - 1) > body_cap)
        return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    SceneDev sc;
    const int rc = scene_sync_device(ctx, &sc);
    if (rc) return rc;
    return qr_launch(ctx, n_spheres, nullptr, nullptr, dev_spheres, (const surtr_mass*)dev_body_mass_or_null, min_mass, dev_piece_mask_or_null, &sc, dev_body_mask);
}

extern "C" int surtr_scene_raycast(surtr_ctx* ctx, uint32_t n_rays, const float* rays, surtr_scene_ray_hit* hits)
{
    if (!ctx || !rays || !hits || n_rays == 0) return SURTR_E_INVALID;
    if (qr_state(ctx)) return SURTR_E_STATE;
    for (uint32_t i = 0; i < n_rays; ++i)
    {
        const float* q = rays + 7 * (size_t)i;
        for (int c = 0; c < 6; ++c) if (!qr_host_finite(q[c])) return SURTR_E_INVALID;
        if ((q[3] == 0.f && q[4] == 0.f && q[5] == 0.f) || !(q[6] >= 0.f)) return SURTR_E_INVALID;
    }
    (void)hipSetDevice(ctx->device);
    DevBuf<float> d_r; DevBuf<surtr_scene_ray_hit> d_h;
    int rc = d_r.grow(ctx, 7 * (size_t)n_rays);
    if (rc == SURTR_OK) rc = d_h.grow(ctx, n_rays);
    if (rc == SURTR_OK && hipMemcpyAsync(d_r.p, rays, 28 * (size_t)n_rays, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    if (rc == SURTR_OK) rc = surtr_scene_raycast_dev(ctx, n_rays, d_r.p, d_h.p, (size_t)n_rays * sizeof(surtr_scene_ray_hit));
    if (rc == SURTR_OK && hipMemcpyAsync(hits, d_h.p, (size_t)n_rays * sizeof(surtr_scene_ray_hit), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == SURTR_OK) rc = SURTR_E_HIP;
    return rc;
}

extern "C" int surtr_scene_overlap(surtr_ctx* ctx, uint32_t n_spheres, const float* spheres, const surtr_mass* body_mass_or_null, float min_mass,
                                   uint32_t* n_compounds, uint8_t* body_mask)
{
    if (!ctx || !n_compounds) return SURTR_E_INVALID;
    if (qr_state(ctx) || ctx->scene_off.size() < 2) return SURTR_E_STATE;
    const uint32_t nc = (uint32_t)ctx->scene_off.size() - 1u;
    if (!body_mask) { *n_compounds = nc; return SURTR_OK; }
    if (!spheres || n_spheres == 0) return SURTR_E_INVALID;
    if (*n_compounds < nc) { *n_compounds = nc; return SURTR_E_CAPACITY; }
    *n_compounds = nc;
    for (uint32_t i = 0; i < 4u * n_spheres; ++i) if (!qr_host_finite(spheres[i])) return SURTR_E_INVALID;
    for (uint32_t i = 0; i < n_spheres; ++i) if (!(spheres[4 * (size_t)i + 3] >= 0.f)) return SURTR_E_INVALID;
    (void)hipSetDevice(ctx->device);
    const size_t total = (size_t)n_spheres * nc;
    DevBuf<float> d_s; DevBuf<uint8_t> d_m; DevBuf<surtr_mass> d_w;
    int rc = d_s.grow(ctx, 4 * (size_t)n_spheres);
    if (rc == SURTR_OK) rc = d_m.grow(ctx, total);
    if (rc == SURTR_OK && body_mass_or_null) rc = d_w.grow(ctx, nc);
    if (rc == SURTR_OK && hipMemcpyAsync(d_s.p, spheres, 16 * (size_t)n_spheres, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    if (rc == SURTR_OK && body_mass_or_null && hipMemcpyAsync(d_w.p, body_mass_or_null, (size_t)nc * sizeof(surtr_mass), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    if (rc == SURTR_OK) rc = surtr_scene_overlap_dev(ctx, n_spheres, d_s.p, body_mass_or_null ? d_w.p : nullptr, min_mass, nullptr, 0, d_m.p, total);
    if (rc == SURTR_OK && hipMemcpyAsync(body_mask, d_m.p, total, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = SURTR_E_HIP;
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && rc == SURTR_OK) rc = SURTR_E_HIP;
    return rc;
}
