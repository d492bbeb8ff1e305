// refit_hull.h -- the greedy limited hull of the refit for a point limit above 4, on ONE wave.
//
// VMACH::ConvexHull::CreateConvexHull (Src/VMACH.cpp:1087-1161) as m_refittingTask calls it through GenerateICHNormal
// (Src/Surtr.cpp:1449-1455, :1961-1974), restated so that every float operation happens in the reference's order:
//   gains (:1099-1108, :1121-1133)  points over lanes; a lane walks the short face lists (all faces, then "visible" and "added")
//                                   in list order, so every sum is the reference's; first maximum by wg_argmax
//   AddPointToHull (:994-1034)      lane 0, on face and edge tables in LDS kept in creation order: the edge list is walked while
//                                   it grows, face1 / face2 are swapped, FindInnerPoint, EraseFace and LinkFace ("both set:
//                                   return") as written
//   CleanUp (:1140-1161)            visible faces and flagged edges leave the tables, the rest keeps its order (compacted in place)
// A hull vertex is a slot (at most 32 of them); faces and edges name slots.  Key2Edge (:941-948) keys an edge by the "%f" text
// of its end points, so two points that print alike share a key: here the key of a coordinate is (sign bit, x * 10^6 rounded
// half-to-even on the exact value), computed in integers (rh_coord_key), every slot carries the first slot with the same three
// keys as its class, and the key of an edge is the unordered pair of its end points' classes.
// An edge that was left with one face and is linked again later can name a face that CleanUp has removed: such a face stays in
// the table ("dead": not a face of the hull any more, still flagged visible) for as long as an edge names it, which is what
// the host builder's tombstones do (host_geom.cpp, LimitedHull).
// Included by surtr_hip.hip after wg_argmax and hull_vol.
#pragma once
#include "clip_core.h"

#define RH_MAXPT 32u         // hull points (the largest RefittingPointLimit)
#define RH_MAXFACE 63u       // faces of a finished hull: two slab planes each, SURTR_MAXF planes at most
#define RH_FCAP 160u         // face table (the hull of the moment, the faces of the point being added, dead faces still named)
#define RH_ECAP 256u         // edge table

namespace surtr {

// Key of one coordinate: *neg = sign bit, *scaled = |x| * 10^6 rounded to an integer, ties to even, on the exact value -- the
// digits of printf("%f").  x = m * 2^e with m < 2^24, and 10^6 = 2^6 * 5^6: m * 15625 has at most 38 bits and is shifted by
// e + 6, with the bits shifted out deciding the rounding.  False: not finite, or the scaled value does not fit 64 bits.
__host__ __device__ inline bool rh_coord_key(float x, uint64_t* scaled, uint32_t* neg)
{
    uint32_t b; memcpy(&b, &x, 4);
    *neg = b >> 31; *scaled = 0;
    const uint32_t E = (b >> 23) & 0xFFu;
    uint32_t m = b & 0x7FFFFFu;
    if (E == 255u) return false;
    int e = -149;
    if (E != 0u) { m |= 0x800000u; e = (int)E - 150; }
    const uint64_t v = (uint64_t)m * 15625ull;
    if (v == 0ull) return true;
    const int s = e + 6;
    if (s >= 0)
    {
        int lead = 0; while (((v << lead) >> 63) == 0ull) ++lead;      // (v != 0, below 2^38)
        if (s > lead) return false;
        *scaled = v << s;
        return true;
    }
    const int r = -s;
    if (r >= 64) return true;      // v < 2^38: far below one half
    uint64_t q = v >> r;
    const uint64_t rem = v & ((1ull << r) - 1ull), half = 1ull << (r - 1);
    if (rem > half || (rem == half && (q & 1ull) != 0ull)) ++q;
    *scaled = q;
    return true;
}

struct RhLds
{
    float pt[RH_MAXPT][3];              // hull points in the order they were added
    uint64_t key[RH_MAXPT][3];          // rh_coord_key of their coordinates
    uint8_t neg[RH_MAXPT];              // bit c: sign of coordinate c
    uint8_t cls[RH_MAXPT];              // first slot with the same keys
    uint8_t fv[RH_FCAP][3];             // faces in creation order: three slots
    uint8_t fst[RH_FCAP];               // bit 0 visible, bit 1 dead (see above)
    uint8_t fmap[RH_FCAP];              // CleanUp: index after the compaction
    uint8_t ee[RH_ECAP][2];             // edges in creation order: end points (slots) as created,
    uint8_t ek[RH_ECAP][2];             // their classes (smaller first): the key,
    int16_t ef[RH_ECAP][2];             // face1 / face2 (-1: none),
    uint8_t erem[RH_ECAP];              // flagged for removal
    uint8_t added[RH_FCAP], visible[RH_FCAP];      // the two face lists of CreateConvexHull (indices into the face table)
    uint32_t nF, nE, nAdded, nVisible, nLive, err;
    float nrm[RH_MAXFACE][3];           // result: unit normals of the live faces in list order
    float4 keep[2 * RH_MAXFACE];        // (k_refit_n: the slab planes while the general clipper runs on a rest of them)
};

__device__ __forceinline__ float rh_vol(const RhLds& H, uint32_t f, const float* p)
{
    return hull_vol(H.pt[H.fv[f][0]], H.pt[H.fv[f][1]], H.pt[H.fv[f][2]], p);
}
__device__ __forceinline__ float rh_pos(float x) { return 0.0f < x ? x : 0.0f; }      // std::max(0.0f, x)

// ---- lane 0 only --------------------------------------------------------------------------------------------------------
__device__ inline void rh_slot(RhLds& H, uint32_t s, const float* p)
{
    uint32_t ng = 0;
    for (int c = 0; c < 3; ++c)
    {
        H.pt[s][c] = p[c];
        uint64_t k; uint32_t g;
        if (!rh_coord_key(p[c], &k, &g)) H.err = (uint32_t)SURTR_E_CAPACITY;
        H.key[s][c] = k; ng |= g << c;
    }
    H.neg[s] = (uint8_t)ng;
    uint32_t t = 0;
    while (t < s && !(H.neg[t] == ng && H.key[t][0] == H.key[s][0] && H.key[t][1] == H.key[s][1] && H.key[t][2] == H.key[s][2])) ++t;
    H.cls[s] = (uint8_t)t;
}

// CreateEdge (:971-983) + ConvexHullEdge::LinkFace
__device__ inline void rh_edge(RhLds& H, uint32_t a, uint32_t b, uint32_t face)
{
    const uint8_t ka = H.cls[a], kb = H.cls[b];
    const uint8_t lo = ka < kb ? ka : kb, hi = ka < kb ? kb : ka;
    uint32_t e = 0;
    while (e < H.nE && !(H.ek[e][0] == lo && H.ek[e][1] == hi)) ++e;
    if (e == H.nE)
    {
        if (H.nE >= RH_ECAP) { H.err = (uint32_t)SURTR_E_CAPACITY; return; }
        H.ee[e][0] = (uint8_t)a; H.ee[e][1] = (uint8_t)b; H.ek[e][0] = lo; H.ek[e][1] = hi;
        H.ef[e][0] = -1; H.ef[e][1] = -1; H.erem[e] = 0;
        H.nE = e + 1u;
    }
    if (H.ef[e][0] >= 0 && H.ef[e][1] >= 0) return;
    H.ef[e][H.ef[e][0] < 0 ? 0 : 1] = (int16_t)face;
}

// CreateFace (:955-969): rewound when Volume(face, inner) < 0; the edges are made of the corners as given
__device__ inline void rh_face(RhLds& H, uint32_t a, uint32_t b, uint32_t c, const float* inner)
{
    if (H.nF >= RH_FCAP) { H.err = (uint32_t)SURTR_E_CAPACITY; return; }
    const uint32_t f = H.nF++;
    H.fv[f][0] = (uint8_t)a; H.fv[f][1] = (uint8_t)b; H.fv[f][2] = (uint8_t)c; H.fst[f] = 0;
    if (rh_vol(H, f, inner) < 0.f) { H.fv[f][0] = (uint8_t)c; H.fv[f][2] = (uint8_t)a; }
    H.added[H.nAdded++] = (uint8_t)f;
    rh_edge(H, a, b, f); rh_edge(H, a, c, f); rh_edge(H, b, c, f);
}

__device__ __forceinline__ bool rh_same(const float* a, const float* b) { return a[0] == b[0] && a[1] == b[1] && a[2] == b[2]; }

// AddPointToHull (:994-1034) for the point in slot p
__device__ inline void rh_add_point(RhLds& H, uint32_t p)
{
    for (uint32_t f = 0; f < H.nF; ++f)
        if ((H.fst[f] & 2u) == 0u && rh_vol(H, f, H.pt[p]) < 0.f) { H.fst[f] |= 1u; H.visible[H.nVisible++] = (uint8_t)f; }
    if (H.nVisible == 0u) return;
    for (uint32_t i = 0; i < H.nE && H.err == 0u; ++i)      // edges appended below are visited too, like the list
    {
        int f1 = H.ef[i][0], f2 = H.ef[i][1];
        if (f1 < 0 || f2 < 0) continue;
        const bool v1 = (H.fst[f1] & 1u) != 0u, v2 = (H.fst[f2] & 1u) != 0u;
        if (v1 && v2) { H.erem[i] = 1; continue; }
        if (!(v1 || v2)) continue;
        if (v1) { const int t = f1; f1 = f2; f2 = t; H.ef[i][0] = (int16_t)f1; H.ef[i][1] = (int16_t)f2; }
        const float* e0 = H.pt[H.ee[i][0]]; const float* e1 = H.pt[H.ee[i][1]];
        const float* inner = H.pt[H.fv[f2][0]];      // FindInnerPoint (:950-962)
        for (int q = 0; q < 3; ++q)
        {
            const float* c = H.pt[H.fv[f2][q]];
            if (!rh_same(c, e0) && !rh_same(c, e1)) { inner = c; break; }
        }
        H.ef[i][H.ef[i][0] == f2 ? 0 : 1] = -1;      // EraseFace(face2)
        rh_face(H, H.ee[i][0], H.ee[i][1], p, inner);
    }
}

// CleanUp (:1140-1161)
__device__ inline void rh_cleanup(RhLds& H)
{
    H.nVisible = 0; H.nAdded = 0;
    uint32_t ne = 0;
    for (uint32_t i = 0; i < H.nE; ++i)
    {
        if (H.erem[i]) continue;
        if (ne != i)
        {
            H.ee[ne][0] = H.ee[i][0]; H.ee[ne][1] = H.ee[i][1]; H.ek[ne][0] = H.ek[i][0]; H.ek[ne][1] = H.ek[i][1];
            H.ef[ne][0] = H.ef[i][0]; H.ef[ne][1] = H.ef[i][1]; H.erem[ne] = 0;
        }
        ++ne;
    }
    H.nE = ne;
    // a visible face is dead from here on; it leaves the table unless an edge that stays still names it
    for (uint32_t f = 0; f < H.nF; ++f) { if (H.fst[f] & 1u) H.fst[f] |= 2u; H.fmap[f] = (H.fst[f] & 2u) ? 0xFFu : 0u; }
    for (uint32_t i = 0; i < ne; ++i)
        for (int s = 0; s < 2; ++s) if (H.ef[i][s] >= 0) H.fmap[H.ef[i][s]] = 0u;
    uint32_t nf = 0, live = 0;
    for (uint32_t f = 0; f < H.nF; ++f)
    {
        if (H.fmap[f] == 0xFFu) continue;
        if (nf != f) { H.fv[nf][0] = H.fv[f][0]; H.fv[nf][1] = H.fv[f][1]; H.fv[nf][2] = H.fv[f][2]; H.fst[nf] = H.fst[f]; }
        if ((H.fst[nf] & 2u) == 0u) ++live;
        H.fmap[f] = (uint8_t)nf; ++nf;
    }
    H.nF = nf; H.nLive = live;
    for (uint32_t i = 0; i < ne; ++i)
        for (int s = 0; s < 2; ++s) if (H.ef[i][s] >= 0) H.ef[i][s] = (int16_t)H.fmap[H.ef[i][s]];
}

// ---- one wave -----------------------------------------------------------------------------------------------------------
// The hull of mp[0..n) with `limit` points (4 <= limit <= RH_MAXPT, limit <= n): H.nLive unit normals in H.nrm.  gain / done:
// one word per point (global scratch of this fragment).  0, or SURTR_E_CAPACITY: more than RH_MAXFACE faces, a table that
// overflowed, a coordinate whose key is out of range -- the engine's limits, not the reference's.  Every lane must call it.
template <class MP>
__device__ inline int rh_build(const MP* mp, const uint32_t n, const uint32_t limit, float* gain, uint32_t* done, RhLds& H, ArgF* slotF, ArgD* slotD)
{
    const uint32_t tid = threadIdx.x;
    // ---- BuildFirstHull (:1036-1085), as in k_refit ----
    ArgF a; a.i = 0xFFFFFFFFu; a.v = 0.f;
    for (uint32_t v = tid; v < n; v += group_size())
    {
        const float x = mp[3 * v];
        if (a.i == 0xFFFFFFFFu || x > a.v) { a.v = x; a.i = v; }
    }
    a = wg_argmax<float, ArgF>(a, slotF);
    const uint32_t i1 = a.i;
    const float p1x = mp[3 * i1], p1y = mp[3 * i1 + 1], p1z = mp[3 * i1 + 2];
    ArgD d; d.i = 0xFFFFFFFFu; d.v = 0.0;
    for (uint32_t v = tid; v < n; v += group_size())
    {
        const double dx = (double)(mp[3 * v] - p1x), dy = (double)(mp[3 * v + 1] - p1y), dz = (double)(mp[3 * v + 2] - p1z);
        const double dist = sqrt(dx * dx + dy * dy + dz * dz);
        if (d.i == 0xFFFFFFFFu || dist > d.v) { d.v = dist; d.i = v; }
    }
    d = wg_argmax<double, ArgD>(d, slotD);
    const uint32_t i2 = d.i;
    const float p2x = mp[3 * i2], p2y = mp[3 * i2 + 1], p2z = mp[3 * i2 + 2];
    a.i = 0xFFFFFFFFu; a.v = 0.f;
    for (uint32_t v = tid; v < n; v += group_size())
    {
        const float ux = p2x - p1x, uy = p2y - p1y, uz = p2z - p1z;
        const float wx = mp[3 * v] - p1x, wy = mp[3 * v + 1] - p1y, wz = mp[3 * v + 2] - p1z;
        const float cx = uy * wz - uz * wy, cy = uz * wx - ux * wz, cz = ux * wy - uy * wx;
        const float area = 0.5f * sqrtf(dot3(cx, cy, cz, cx, cy, cz));
        if (a.i == 0xFFFFFFFFu || area > a.v) { a.v = area; a.i = v; }
    }
    a = wg_argmax<float, ArgF>(a, slotF);
    const uint32_t i3 = a.i;
    const float q1[3] = {p1x, p1y, p1z}, q2[3] = {p2x, p2y, p2z};
    const float q3[3] = {mp[3 * i3], mp[3 * i3 + 1], mp[3 * i3 + 2]};
    a.i = 0xFFFFFFFFu; a.v = 0.f;
    for (uint32_t v = tid; v < n; v += group_size())
    {
        const float pv[3] = {mp[3 * v], mp[3 * v + 1], mp[3 * v + 2]};
        const float vol = hull_vol(q1, q2, q3, pv);
        if (a.i == 0xFFFFFFFFu || vol > a.v) { a.v = vol; a.i = v; }
    }
    a = wg_argmax<float, ArgF>(a, slotF);
    const uint32_t i4 = a.i;
    if (tid == 0)
    {
        const float q4[3] = {mp[3 * i4], mp[3 * i4 + 1], mp[3 * i4 + 2]};
        H.nF = 0; H.nE = 0; H.nAdded = 0; H.nVisible = 0; H.nLive = 4; H.err = 0;
        rh_slot(H, 0, q1); rh_slot(H, 1, q2); rh_slot(H, 2, q3); rh_slot(H, 3, q4);
        rh_face(H, 0, 1, 2, q4); rh_face(H, 0, 1, 3, q3); rh_face(H, 0, 2, 3, q2); rh_face(H, 1, 2, 3, q1);
    }
    __syncthreads();
    // ---- gains of the points outside the first hull (:1099-1108); its four points are processed, with gain 0 ----
    for (uint32_t v = tid; v < n; v += group_size())
    {
        const bool first = v == i1 || v == i2 || v == i3 || v == i4;
        float g = 0.f;
        if (!first)
        {
            const float pv[3] = {mp[3 * v], mp[3 * v + 1], mp[3 * v + 2]};
            for (uint32_t f = 0; f < 4u; ++f) g += rh_pos(rh_vol(H, f, pv));
        }
        gain[v] = g; done[v] = first ? 1u : 0u;
    }
    // (the first four faces stay in `added` until the first CleanUp, as in the reference)
    for (uint32_t used = 4; used < limit; ++used)
    {
        if (H.err != 0u) break;      // (uniform: read after a barrier)
        a.i = 0xFFFFFFFFu; a.v = 0.f;
        for (uint32_t v = tid; v < n; v += group_size())
        {
            const float g = gain[v];
            if (a.i == 0xFFFFFFFFu || g > a.v) { a.v = g; a.i = v; }
        }
        a = wg_argmax<float, ArgF>(a, slotF);      // std::max_element: the first maximum
        const uint32_t k = a.i;
        if (tid == 0)
        {
            const float pk[3] = {mp[3 * k], mp[3 * k + 1], mp[3 * k + 2]};
            rh_slot(H, used, pk);
            if (H.err == 0u) rh_add_point(H, used);
        }
        __syncthreads();
        const uint32_t nVis = H.nVisible, nAdd = H.nAdded;
        for (uint32_t v = tid; v < n; v += group_size())
        {
            if (v == k) { gain[v] = -3.402823466e+38f; done[v] = 1u; continue; }
            if (done[v] != 0u) continue;
            const float pv[3] = {mp[3 * v], mp[3 * v + 1], mp[3 * v + 2]};
            float gone = 0.f, came = 0.f;
            for (uint32_t q = 0; q < nVis; ++q) gone += rh_pos(rh_vol(H, H.visible[q], pv));
            for (uint32_t q = 0; q < nAdd; ++q) came += rh_pos(rh_vol(H, H.added[q], pv));
            float g = gain[v];
            g -= gone; g += came;
            gain[v] = g;
        }
        __syncthreads();
        if (tid == 0 && H.err == 0u) rh_cleanup(H);
        __syncthreads();
    }
    __syncthreads();
    if (H.err != 0u) return (int)H.err;
    // ---- GenerateICHNormal (Src/Surtr.cpp:1961-1974): normalize((v1-v0) x (v2-v0)) per face in list order ----
    if (tid == 0)
    {
        uint32_t m = 0;
        for (uint32_t f = 0; f < H.nF; ++f) if ((H.fst[f] & 2u) == 0u) { if (m < RH_FCAP) H.added[m] = (uint8_t)f; ++m; }
        H.nLive = m;
    }
    __syncthreads();
    const uint32_t F = H.nLive;
    if (F > RH_MAXFACE) return SURTR_E_CAPACITY;
    for (uint32_t j = tid; j < F; j += group_size())
    {
        const uint32_t f = H.added[j];
        const float* v0 = H.pt[H.fv[f][0]]; const float* v1 = H.pt[H.fv[f][1]]; const float* v2 = H.pt[H.fv[f][2]];
        const float ax = v1[0] - v0[0], ay = v1[1] - v0[1], az = v1[2] - v0[2];
        const float bx = v2[0] - v0[0], by = v2[1] - v0[1], bz = v2[2] - v0[2];
        float nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
        const float len = sqrtf(dot3(nx, ny, nz, nx, ny, nz));
        if (len != 0.f) { nx = nx / len; ny = ny / len; nz = nz / len; } else { nx = ny = nz = 0.f; }
        H.nrm[j][0] = nx; H.nrm[j][1] = ny; H.nrm[j][2] = nz;
    }
    __syncthreads();
    return 0;
}

} // namespace surtr
