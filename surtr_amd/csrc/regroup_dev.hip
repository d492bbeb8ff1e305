// regroup_dev.hip -- the step right after the fracture event as a device step: bind sets of
// ApplyFracture (Src/Surtr.cpp:2103-2146), MergeOutOfImpact (:2368-2403, ConvexOutOfSphere :2415-2458) and
// HandleConvexIsland (:2203-2366) on the UN-refitted Convex solids of the last event, which never leave HBM.
//
//   k_rg_count / k_rg_faces   one wave per piece: Poly::ExtractFaces of its Convex; per face the plane
//                             (normalised 3-point plane, |d|) and the polygon's points; ConvexOutOfSphere per fragment
//   (sort)                    faces by (compound, |d|): device radix sort
//   k_rg_pairs                one lane per face: the faces of its compound within 1e-3 of its |d| -> opposite normals ->
//                             point-in-polygon both ways (VMACH::OnYourRight) -> an edge between the two pieces
//   k_rg_labels               min-label propagation over the pieces until nothing changes
//   k_scene_outside           ConvexOutOfSphere of resident pieces before an event (surtr_scene_outside): one wave per piece
//   k_scene_outside_impacts   the same with a sphere per piece, for the impacts of one frame (surtr_scene_outside_impacts)
// Only per-piece flags and labels (a few bytes per piece) cross the bus; the host turns them into the reference's bind sets
// (first group of a compound stays, the others are appended in discovery order).  Pieces are numbered as in
// surtr_regroup: the resident pieces the event skipped (its `outside` mask), ascending, then the event's fragments.  After an event
// over several bodies (surtr_scene_fracture_bodies) a bind set belongs to one body (surtr_event_regroup_bodies); after an event over
// several impacts (surtr_scene_fracture_impacts) every body is tested against its own impact's sphere (surtr_event_regroup_impacts).
#include <array>
#include <cstring>
#include <mutex>
#include <set>
#include <unordered_map>

#include "surtr_ctx.h"
#include <hipcub/hipcub.hpp>

#define RG_MAXH 4096u       // half-edges of one Convex the face extraction handles

namespace {

struct P3 { float x, y, z; };
__device__ __forceinline__ P3 sub3(P3 a, P3 b) { return P3{a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ float dotp(P3 a, P3 b) { float t = a.x * b.x + a.y * b.y; return t + a.z * b.z; }
__device__ __forceinline__ P3 cross3(P3 a, P3 b) { return P3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ P3 unit3(P3 a)
{
    const float l = sqrtf(dotp(a, a));
    if (!(l != 0.f)) return P3{0.f, 0.f, 0.f};
    return P3{a.x / l, a.y / l, a.z / l};
}
__device__ __forceinline__ bool right_of3(P3 a, P3 b, P3 c, P3 n) { return dotp(cross3(sub3(b, a), sub3(c, a)), n) > 0.f; }   // VMACH::OnYourRight

// A piece's Convex wherever it lives: resident (CSR loff, len = loff[v+1]-loff[v]) or in the arena (loff absolute + llen).
struct RgSolid { const float* pos; const uint32_t* loff; const uint32_t* llen; const int32_t* nbr; uint32_t nv; };
struct RgSrc { const uint32_t* kind; const uint32_t* index; };      // per piece: 0 = resident piece `index`, 1 = fragment `index`

__device__ RgSolid rg_solid(uint32_t p, RgSrc src, const FragRec* __restrict__ frags, Arena A, const float* cpos, const uint32_t* cloff,
                            const int32_t* cnbr, const uint32_t* cvo)
{
    const uint32_t i = src.index[p];
    if (src.kind[p] == 0u)
    {
        const uint32_t a = cvo[i];
        return RgSolid{cpos + 3 * (size_t)a, cloff + a, nullptr, cnbr, cvo[i + 1] - a};
    }
    const FragRec fr = frags[i];
    return RgSolid{A.pos + 3 * (size_t)fr.cv_off, A.loff + fr.cv_off, A.llen + fr.cv_off, A.nbr, fr.cv_n};
}
__device__ __forceinline__ uint32_t rg_len(const RgSolid& S, uint32_t v) { return S.llen ? S.llen[v] : S.loff[v + 1] - S.loff[v]; }
__device__ __forceinline__ P3 rg_pos(const RgSolid& S, int v) { return P3{S.pos[3 * (size_t)v], S.pos[3 * (size_t)v + 1], S.pos[3 * (size_t)v + 2]}; }
__device__ __forceinline__ int rg_before(const RgSolid& S, int v, int who)
{
    const int32_t* r = S.nbr + S.loff[v]; const uint32_t n = rg_len(S, (uint32_t)v);
    uint32_t k = 0;
    while (k < n && r[k] != who) ++k;
    return k == 0 ? r[n - 1] : r[k - 1];
}

struct FaceNode { uint32_t piece, pts_off, pts_n, pad; P3 n; float absd; };

// Poly::ExtractFaces of piece p on one lane (visited set keyed by (vertex, neighbour) = the first slot that holds the
// neighbour, as in the reference); emit(face points...) per face with >= 3 points.  Returns false when the solid is too large.
template <class Emit>
__device__ bool rg_walk_faces(const RgSolid& S, uint8_t* seen /* RG_MAXH */, uint32_t* base /* per vertex, nv <= RG_MAXH */, Emit emit)
{
    uint32_t H = 0;
    if (S.nv > RG_MAXH) return false;
    for (uint32_t v = 0; v < S.nv; ++v) { base[v] = H; H += rg_len(S, v); if (H > RG_MAXH) return false; }
    for (uint32_t e = 0; e < H; ++e) seen[e] = 0;
    auto slot = [&](int a, int b) -> uint32_t {
        const int32_t* r = S.nbr + S.loff[a]; const uint32_t n = rg_len(S, (uint32_t)a);
        uint32_t q = 0;
        while (q < n && r[q] != b) ++q;
        return base[a] + (q < n ? q : 0u);
    };
    for (int i = 0; i < (int)S.nv; ++i)
    {
        const uint32_t deg = rg_len(S, (uint32_t)i);
        for (uint32_t s = 0; s < deg; ++s)
        {
            const int adj = (S.nbr + S.loff[i])[s];
            if (seen[slot(i, adj)]) continue;
            emit(i, -1, 0);                                   // start of a face
            int prev = i, cur = adj; uint32_t len = 1;
            while (cur != i && len <= S.nv * 8u + 8u)
            {
                seen[slot(prev, cur)] = 1;
                emit(cur, -1, 1);
                const int nx = rg_before(S, cur, prev);
                prev = cur; cur = nx; ++len;
            }
            seen[slot(prev, cur)] = 1;
            emit(-1, -1, 2);                                  // end of the face
        }
    }
    return true;
}

// pass 0: counts (faces with >= 3 points, their points) per piece; pass 1: the face nodes + ConvexOutOfSphere
__global__ __launch_bounds__(SURTR_LANES) void k_rg_faces(uint32_t n_pieces, RgSrc src, const FragRec* __restrict__ frags, Arena A, const float* cpos,
                                                          const uint32_t* cloff, const int32_t* cnbr, const uint32_t* cvo, uint32_t pass,
                                                          uint32_t* __restrict__ cnt /* 2 per piece */, const uint32_t* __restrict__ face_off,
                                                          const uint32_t* __restrict__ pts_off, FaceNode* __restrict__ nodes, P3* __restrict__ pts,
                                                          uint32_t n_sphere, const float* __restrict__ sphere, float ox, float oy, float oz, float radius,
                                                          uint8_t* __restrict__ out_flag, uint32_t* __restrict__ err,
                                                          const uint32_t* __restrict__ piece_imp, const ImpSphere* __restrict__ imp_tab)
{
    __shared__ uint8_t seen[RG_MAXH];
    __shared__ uint32_t base[RG_MAXH];
    __shared__ uint32_t sh_in;
    const uint32_t p = blockIdx.x;
    if (p >= n_pieces) return;
    bool no_sphere = false;      // surtr_event_regroup_impacts_partial: the piece's impact is not partial, its byte is 0 untested
    if (piece_imp)      // surtr_event_regroup_impacts: the sphere of the impact this piece's body belongs to
    {
        const ImpSphere s = imp_tab[piece_imp[p]];
        ox = s.ox; oy = s.oy; oz = s.oz; radius = s.radius;
        sphere += 3 * (size_t)s.cloud_begin; n_sphere = s.cloud_n;
        no_sphere = s.no_sphere != 0u;
    }
    const RgSolid S = rg_solid(p, src, frags, A, cpos, cloff, cnbr, cvo);
    if (threadIdx.x == 0)
    {
        uint32_t nf = 0, np = 0, cur_n = 0, cur_start = 0;
        const uint32_t f0 = pass ? face_off[p] : 0u, p0 = pass ? pts_off[p] : 0u;
        bool inside_possible = true;      // ConvexOutOfSphere part 1: every vertex at least `radius` from the origin (:2420-2427)
        if (pass && out_flag && !no_sphere)
            for (uint32_t v = 0; v < S.nv; ++v)
            {
                const P3 d = sub3(P3{ox, oy, oz}, rg_pos(S, (int)v));
                if (sqrtf(dotp(d, d)) < radius) { inside_possible = false; break; }
            }
        const bool ok = rg_walk_faces(S, seen, base, [&](int v, int, int what) {
            if (what == 0) { cur_n = 0; cur_start = np; }
            if (what <= 1) { if (pass) pts[p0 + np] = rg_pos(S, v); ++np; ++cur_n; }
            if (what == 2)
            {
                if (cur_n < 3u) { np = cur_start; return; }      // (:2243: faces of fewer than three points are skipped)
                if (pass)
                {
                    const P3 a = pts[p0 + cur_start], b = pts[p0 + cur_start + 1], c = pts[p0 + cur_start + 2];
                    const P3 n = unit3(cross3(sub3(a, b), sub3(a, c)));      // Plane(p0, p1, p2), normalised
                    const float d = -dotp(n, a);
                    FaceNode fn; fn.piece = p; fn.pts_off = p0 + cur_start; fn.pts_n = cur_n; fn.pad = 0;
                    fn.n = unit3(n); fn.absd = fabsf(d);                      // .Normal() re-normalised (:2252-2254)
                    nodes[f0 + nf] = fn;
                }
                ++nf;
            }
        });
        if (!ok) atomicMax(err, (uint32_t)SURTR_E_CAPACITY);
        if (!pass) { cnt[2 * p] = nf; cnt[2 * p + 1] = np; }
        sh_in = inside_possible ? nf : 0xFFFFFFFFu;
    }
    __syncthreads();
    if (pass && out_flag)
    {
        // ConvexOutOfSphere part 2 (:2429-2455): no point of the sphere cloud inside the Convex (all its face planes)
        const uint32_t nf = sh_in;
        bool hit = no_sphere || nf == 0xFFFFFFFFu;
        if (!hit)
            for (uint32_t q = threadIdx.x; q < n_sphere && !hit; q += group_size())
            {
                const P3 po{sphere[3 * q], sphere[3 * q + 1], sphere[3 * q + 2]};
                bool contain = true;
                for (uint32_t f = 0; f < nf && contain; ++f)
                {
                    const FaceNode& fn = nodes[face_off[p] + f];
                    const P3 a = pts[fn.pts_off], b = pts[fn.pts_off + 1], c = pts[fn.pts_off + 2];
                    const P3 n = unit3(cross3(sub3(b, a), sub3(c, a)));
                    const float d = -dotp(a, n);
                    if (dotp(n, po) + d > 0.f) contain = false;
                }
                if (contain) hit = true;
            }
        const bool any = __ballot(hit) != 0ull;
        if (threadIdx.x == 0) out_flag[p] = any ? 0 : 1;
    }
}

// Surtr::ConvexOutOfSphere (Src/Surtr.cpp:2415-2458) of resident Convex solids, one wave per listed piece, in one launch: what
// k_rg_faces' second pass answers for the pieces of an event, here for the pieces a click is about to break (the `outside` mask of
// surtr_scene_fracture_bodies), without a count pass, a face list in memory or a host round trip.
//   1. every vertex at least `radius` from the origin, across the lanes; a piece with a vertex inside ends here (byte 0);
//   2. the faces, one lane per half-edge: Poly::ExtractFaces starts every face at its smallest vertex, so the half-edge (v, adj) leads
//      a face when v is the least vertex of the loop it walks (and adj's first slot in v's ring: the reference's visited set is keyed
//      by (vertex, neighbour)).  A leader forms the plane from v and the two vertices after it -- the float expressions of
//      k_rg_faces' second part and of surtr_convex_out_of_sphere -- and puts it into LDS at a slot counted with a ballot; loops of
//      fewer than three points are skipped.  Leaders are distinct half-edges: at most RG_MAXH planes;
//   3. the cloud, a lane per point, against the planes in LDS (every lane reads the same plane: a broadcast); one store of the byte.
// PRECONDITION for the host's answer bit for bit: the solid is a regular polyhedron -- no ring lists a neighbour twice (PieceSet::dup
// is 0) and no face loop passes through a vertex twice, so that "next half-edge" is a permutation of the half-edges and its orbits
// are the faces.  That is every convex hull and every unflagged fragment.  On any other solid the leaders need not be the faces
// ExtractFaces' visited set yields (a plane may be formed that the host never forms, or one skipped), the byte is still defined and
// deterministic, and nothing is read or written out of bounds: walks are bounded as the host's are and there is room for a plane
// per half-edge.
// LDS: static, RG_MAXH planes = 64 KiB, two one-wave blocks per CU.  The grid is the handful of pieces a click touches; a size
// taken from the largest piece of the list would need dynamic LDS, which the one-lane emulation build does not have.
// (the body, shared by k_scene_outside and k_scene_outside_impacts: listed piece i against one sphere; `plane` is the block's LDS)
__device__ __forceinline__ void scene_outside_piece(uint32_t i, const uint32_t* __restrict__ list, const float* __restrict__ cpos,
                                                    const uint32_t* __restrict__ cloff, const int32_t* __restrict__ cnbr, const uint32_t* __restrict__ cvo,
                                                    uint32_t n_sphere, const float* __restrict__ sphere, float ox, float oy, float oz, float radius,
                                                    uint8_t* __restrict__ out, float4* plane)
{
    const uint32_t lane = threadIdx.x, G = group_size();
    const uint32_t p = list[i], a0 = cvo[p];
    const RgSolid S{cpos + 3 * (size_t)a0, cloff + a0, nullptr, cnbr, cvo[p + 1] - a0};
    bool near = false;
    for (uint32_t v = lane; v < S.nv && !near; v += G)
    {
        const P3 d = sub3(P3{ox, oy, oz}, rg_pos(S, (int)v));
        if (sqrtf(dotp(d, d)) < radius) near = true;
    }
    const bool inside = __ballot(near) != 0ull;
    if (inside || n_sphere == 0u)
    {
        if (lane == 0u) out[i] = inside ? 0 : 1;
        return;
    }
    const uint32_t h0 = S.loff[0], H = S.loff[S.nv] - h0;      // (the host has checked H and nv against RG_MAXH)
    uint32_t nf = 0;
    for (uint32_t e0 = 0; e0 < H; e0 += G)
    {
        const uint32_t e = e0 + lane;
        bool lead = false; float4 pl = make_float4(0.f, 0.f, 0.f, 0.f);
        if (e < H)
        {
            uint32_t lo = 0, hi = S.nv;                         // the vertex of half-edge e: loff[lo] <= h0 + e < loff[hi]
            while (hi - lo > 1u) { const uint32_t mid = (lo + hi) >> 1; if (S.loff[mid] <= h0 + e) lo = mid; else hi = mid; }
            const int v = (int)lo;
            const int32_t* ring = S.nbr + S.loff[v]; const uint32_t s = h0 + e - S.loff[v];
            const int adj = ring[s];
            bool first = true;
            for (uint32_t k = 0; k < s; ++k) if (ring[k] == adj) first = false;
            if (first)
            {
                int prev = v, cur = adj, third = -1; uint32_t len = 1; bool least = true;
                while (cur != v && len <= S.nv * 8u + 8u)
                {
                    if (cur < v) { least = false; break; }
                    if (len == 2u) third = cur;
                    const int nx = rg_before(S, cur, prev);
                    prev = cur; cur = nx; ++len;
                }
                if (least && len >= 3u)
                {
                    const P3 a = rg_pos(S, v), b = rg_pos(S, adj), c = rg_pos(S, third);
                    const P3 nn = unit3(cross3(sub3(b, a), sub3(c, a)));
                    pl = make_float4(nn.x, nn.y, nn.z, -dotp(a, nn));
                    lead = true;
                }
            }
        }
        const unsigned long long m = __ballot(lead);
        if (lead) plane[nf + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = pl;
        nf += (uint32_t)__builtin_popcountll(m);
    }
    __syncthreads();
    bool hit = false;
    for (uint32_t q = lane; q < n_sphere && !hit; q += G)
    {
        const P3 po{sphere[3 * q], sphere[3 * q + 1], sphere[3 * q + 2]};
        bool contain = true;
        for (uint32_t f = 0; f < nf && contain; ++f)
        {
            const float4 w = plane[f];
            if (dotp(P3{w.x, w.y, w.z}, po) + w.w > 0.f) contain = false;
        }
        if (contain) hit = true;
    }
    const bool any = __ballot(hit) != 0ull;
    if (lane == 0u) out[i] = any ? 0 : 1;
}

__global__ __launch_bounds__(SURTR_LANES) void k_scene_outside(uint32_t n, const uint32_t* __restrict__ list, const float* __restrict__ cpos,
                                                               const uint32_t* __restrict__ cloff, const int32_t* __restrict__ cnbr,
                                                               const uint32_t* __restrict__ cvo, uint32_t n_sphere, const float* __restrict__ sphere,
                                                               float ox, float oy, float oz, float radius, uint8_t* __restrict__ out)
{
    __shared__ float4 plane[RG_MAXH];
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    scene_outside_piece(i, list, cpos, cloff, cnbr, cvo, n_sphere, sphere, ox, oy, oz, radius, out, plane);
}

// The same with a sphere per piece (surtr_scene_outside_impacts): listed piece i belongs to impact imp[i], whose origin, radius and
// range of the cloud stand in the small table `tab`.  One launch for the pieces of every impact of a frame; the byte of a piece is
// the one k_scene_outside writes for it with that impact's sphere alone (the same body on the same arguments).
__global__ __launch_bounds__(SURTR_LANES) void k_scene_outside_impacts(uint32_t n, const uint32_t* __restrict__ list, const uint32_t* __restrict__ imp,
                                                                       const ImpSphere* __restrict__ tab, const float* __restrict__ cpos,
                                                                       const uint32_t* __restrict__ cloff, const int32_t* __restrict__ cnbr,
                                                                       const uint32_t* __restrict__ cvo, const float* __restrict__ sphere,
                                                                       uint8_t* __restrict__ out)
{
    __shared__ float4 plane[RG_MAXH];
    const uint32_t i = blockIdx.x;
    if (i >= n) return;
    const ImpSphere s = tab[imp[i]];
    scene_outside_piece(i, list, cpos, cloff, cnbr, cvo, s.cloud_n, sphere + 3 * (size_t)s.cloud_begin, s.ox, s.oy, s.oz, s.radius, out, plane);
}

__global__ void k_rg_keys(uint32_t nf, const FaceNode* __restrict__ nodes, const uint32_t* __restrict__ set_of, unsigned long long* __restrict__ key,
                          uint32_t* __restrict__ val)
{
    const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= nf) return;
    uint32_t bits; const float ad = nodes[f].absd;
    memcpy(&bits, &ad, 4);                                                                               // |d| >= 0: the bits order like the value
    key[f] = ((unsigned long long)set_of[nodes[f].piece] << 32) | bits;
    val[f] = f;
}

__global__ void k_rg_pairs(uint32_t nf, const uint32_t* __restrict__ order, const unsigned long long* __restrict__ skey, const FaceNode* __restrict__ nodes,
                           const P3* __restrict__ pts, uint2* __restrict__ edges, uint32_t cap_edges, uint32_t* __restrict__ n_edges)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf) return;
    const FaceNode A = nodes[order[i]];
    const uint32_t set = (uint32_t)(skey[i] >> 32);
    for (uint32_t j = i + 1; j < nf; ++j)
    {
        if ((uint32_t)(skey[j] >> 32) != set) break;
        const FaceNode B = nodes[order[j]];
        if (fabs((double)A.absd - (double)B.absd) > 1e-3) break;                 // sorted: every later face is farther still
        if (!((double)fabsf(1.f + dotp(A.n, B.n)) < 1e-4)) continue;             // normals must be opposite
        bool touch = false;
        for (uint32_t a = 0; a < A.pts_n && !touch; ++a)
        {
            const P3 ip = pts[A.pts_off + a];
            bool inside = true;
            for (uint32_t v = 0; v < B.pts_n; ++v)
                if (!right_of3(pts[B.pts_off + v], pts[B.pts_off + (v + 1u) % B.pts_n], ip, B.n)) { inside = false; break; }
            if (inside) touch = true;
        }
        for (uint32_t b = 0; b < B.pts_n && !touch; ++b)
        {
            const P3 jp = pts[B.pts_off + b];
            bool inside = true;
            for (uint32_t v = 0; v < A.pts_n; ++v)
                if (!right_of3(pts[A.pts_off + v], pts[A.pts_off + (v + 1u) % A.pts_n], jp, A.n)) { inside = false; break; }
            if (inside) touch = true;
        }
        if (touch && A.piece != B.piece)
        {
            const uint32_t at = atomicAdd(n_edges, 1u);
            if (at < cap_edges) edges[at] = make_uint2(A.piece, B.piece);
        }
    }
}

// one round of min-label propagation over the edges + one pointer jump; *changed != 0 when a label moved
__global__ void k_rg_labels(uint32_t ne, const uint2* __restrict__ edges, uint32_t n_pieces, uint32_t* __restrict__ lab, uint32_t* __restrict__ changed)
{
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e < ne)
    {
        const uint32_t a = edges[e].x, b = edges[e].y;
        const uint32_t la = lab[a], lb = lab[b], m = la < lb ? la : lb;
        if (m < la) { atomicMin(&lab[a], m); *changed = 1u; }
        if (m < lb) { atomicMin(&lab[b], m); *changed = 1u; }
    }
    if (e < n_pieces) { const uint32_t l = lab[e], ll = lab[l]; if (ll < l) { atomicMin(&lab[e], ll); *changed = 1u; } }
}

// The label rounds to convergence in ONE launch: a single workgroup sweeps the edges and the pointer jumps round after round
// (labels only decrease, so a round that changes nothing ends it; at most n_pieces + 8 rounds, as the host loop had) -- no
// host round trip per round.  rounds_out: rounds run, or 0xFFFFFFFF when the bound was hit.
#define RG_LABEL_THREADS 1024u
__global__ __launch_bounds__(RG_LABEL_THREADS) void k_rg_labels_all(uint32_t ne, const uint2* __restrict__ edges, uint32_t n_pieces, uint32_t* __restrict__ lab,
                                                                    uint32_t* __restrict__ rounds_out)
{
    __shared__ uint32_t changed[2];
    const uint32_t tid = threadIdx.x, G = blockDim.x;
    if (tid < 2u) changed[tid] = 0u;
    __syncthreads();
    uint32_t round = 0;
    for (; round < n_pieces + 8u; ++round)
    {
        bool ch = false;
        for (uint32_t e = tid; e < ne; e += G)
        {
            const uint32_t a = edges[e].x, b = edges[e].y;
            const uint32_t la = lab[a], lb = lab[b], m = la < lb ? la : lb;
            if (m < la) { atomicMin(&lab[a], m); ch = true; }
            if (m < lb) { atomicMin(&lab[b], m); ch = true; }
        }
        __syncthreads();
        for (uint32_t v = tid; v < n_pieces; v += G) { const uint32_t l = lab[v], ll = lab[l]; if (ll < l) { atomicMin(&lab[v], ll); ch = true; } }
        if (ch) changed[round & 1u] = 1u;
        __syncthreads();
        const bool any = changed[round & 1u] != 0u;
        if (tid == 0u) changed[(round + 1u) & 1u] = 0u;
        __syncthreads();
        if (!any) break;
    }
    if (tid == 0u) *rounds_out = round < n_pieces + 8u ? round + 1u : 0xFFFFFFFFu;
}

// surtr_regroup_stats: what the last surtr_event_regroup of a context counted, kept on the host beside the context (filled from
// values the call reads back anyway: no launch, no copy and no synchronisation of its own)
enum { RGS_PIECES, RGS_FACES, RGS_POINTS, RGS_EDGES, RGS_CAP_EDGES, RGS_ROUNDS, RGS_OUT, RGS_SPARE };
std::mutex g_stats_lock;
std::unordered_map<const surtr_ctx*, std::array<uint32_t, 8>> g_stats;
struct StatsScope       // collects during the call, publishes when it returns (whatever it returns)
{
    const surtr_ctx* ctx; std::array<uint32_t, 8> v{};
    explicit StatsScope(const surtr_ctx* c) : ctx(c) {}
    ~StatsScope() { std::lock_guard<std::mutex> g(g_stats_lock); g_stats[ctx] = v; }
};

} // namespace

extern "C" int surtr_regroup_stats(surtr_ctx* ctx, uint32_t out[8])
{
    if (!ctx || !out) return SURTR_E_INVALID;
    std::lock_guard<std::mutex> g(g_stats_lock);
    const auto it = g_stats.find(ctx);
    for (int k = 0; k < 8; ++k) out[k] = it == g_stats.end() ? 0u : it->second[k];
    return SURTR_OK;
}

// surtr_destroy: the context's entry goes with it (a later context at the same address starts from zeros)
extern "C" void surtr_regroup_forget(const surtr_ctx* ctx)
{
    std::lock_guard<std::mutex> g(g_stats_lock);
    g_stats.erase(ctx);
}

// The spheres of surtr_event_regroup_impacts: impact i's origin, radius and points [sphere_off[i], sphere_off[i + 1]) of the cloud.
struct ImpactSpheres { uint32_t n; const uint32_t* sphere_off; const float* origins; const float* radii; const uint8_t* partial = nullptr; };

// The bodies of the event: after surtr_scene_fracture_bodies one per target, in the order the targets were given (a bind set belongs
// to one body); after any other event one body holding everything, which is the regrouping as it was before there were bodies.
// With `impacts` (surtr_event_regroup_impacts, after surtr_scene_fracture_impacts) every piece is tested against the sphere of the
// impact its body belongs to; n_sphere / sphere_points are then the whole cloud, and origin / radius are not read.
static int regroup_event(surtr_ctx* ctx, int partial, uint32_t n_sphere, const float* sphere_points, const float origin[3], float radius,
                         uint32_t* n_pieces_out, uint32_t* n_compounds, uint32_t* compound_off, int32_t* compound_piece, uint32_t* body_compound_off,
                         const ImpactSpheres* impacts = nullptr)
{
    if (!ctx || !n_compounds) return SURTR_E_INVALID;
    if (!ctx->have_event) return SURTR_E_STATE;
    if (partial && (!origin || (n_sphere && !sphere_points))) return SURTR_E_INVALID;
    surtr_counts c;
    int rc = surtr_event_counts(ctx, &c);
    if (rc) return rc;
    // pieces: the resident pieces the event skipped, then its fragments; bind sets as ApplyFracture leaves them.  The `outside`
    // mask belongs to the event that took it and to the pieces it ran over: surtr_load_fragments drops it (its fragments are
    // nobody's event), and once surtr_pieces_from_event has replaced the pieces a mask that kept any of them out names solids
    // that are gone -- the compounds of that event can no longer be formed (include/surtr_hip.h)
    const bool masked = std::find_if(ctx->last_outside.begin(), ctx->last_outside.end(), [](uint8_t o) { return o != 0; }) != ctx->last_outside.end();
    if (masked && (!ctx->frags_of_pieces || ctx->last_outside.size() != ctx->n_pieces))
    {
        ctx->err = "surtr_event_regroup: the event kept pieces out of the impact, and the resident pieces have been replaced since";
        return SURTR_E_STATE;
    }
    // (after surtr_scene_fracture_event the mask is zero outside the event's compound: the pieces of other bodies are in no bind set)
    std::vector<uint32_t> skipped;
    for (uint32_t p = 0; masked && p < ctx->n_pieces; ++p)
        if (ctx->last_outside[p]) skipped.push_back(p);
    (void)hipSetDevice(ctx->device);
    hipStream_t st = ctx->stream;
    // (the counts once more, as when this function was two: a small copy and a synchronisation of a stream with nothing queued, kept so
    //  that a regroup enqueues exactly what it always did)
    rc = surtr_event_counts(ctx, &c);
    if (rc) return rc;
    std::vector<uint32_t> kind(skipped.size(), 0u), index(skipped), set_of;
    const uint32_t n_outside = (uint32_t)kind.size();
    std::vector<FragRec> fr(c.n_frag);
    if (c.n_frag) HIPCHK(hipMemcpy(fr.data(), ctx->d_frags, (size_t)c.n_frag * sizeof(FragRec), hipMemcpyDeviceToHost));
    for (uint32_t f = 0; f < c.n_frag; ++f) { kind.push_back(1u); index.push_back(f); }
    const uint32_t n = (uint32_t)kind.size();
    if (n_pieces_out) *n_pieces_out = n;
    if (!compound_off || !compound_piece) { *n_compounds = 0; return SURTR_OK; }      // sizes only: n + bodies + 1 / n entries are enough
    StatsScope stats(ctx);
    stats.v[RGS_PIECES] = n;
    // body of every piece: the target whose compound holds the resident piece (a fragment's: the piece it was cut from)
    const std::vector<uint32_t>& targets = ctx->scene_event_compound;
    const uint32_t nb = (uint32_t)std::max<size_t>(targets.size(), 1);
    auto body_of = [&](uint32_t resident) -> uint32_t {
        if (nb == 1u) return 0u;
        const uint32_t comp = (uint32_t)(std::upper_bound(ctx->scene_off.begin(), ctx->scene_off.end(), resident) - ctx->scene_off.begin()) - 1u;
        for (uint32_t b = 0; b < nb; ++b) if (targets[b] == comp) return b;
        return 0u;
    };
    // bind[b], b < nb: bind 0 of body b (its pieces out of the impact); then the cell binds, cut where the cell OR the body changes
    // (two bodies' fragments of equal cell number are two binds); owner[i]: the body of bind i
    std::vector<std::set<int>> bind(nb);
    std::vector<uint32_t> owner(nb), frag_body(c.n_frag);
    for (uint32_t b = 0; b < nb; ++b) owner[b] = b;
    for (uint32_t p = 0; p < n_outside; ++p) bind[body_of(skipped[p])].insert((int)p);
    for (uint32_t f = 0; f < c.n_frag; ++f)
    {
        frag_body[f] = body_of((uint32_t)fr[f].piece);
        if (f == 0 || fr[f].cell != fr[f - 1].cell || frag_body[f] != frag_body[f - 1]) { bind.emplace_back(); owner.push_back(frag_body[f]); }
        bind.back().insert((int)(n_outside + f));
    }
    if (n == 0)
    {
        *n_compounds = nb;
        for (uint32_t b = 0; b <= nb; ++b) { compound_off[b] = 0; if (body_compound_off) body_compound_off[b] = b; }
        return SURTR_OK;
    }
    // (the call's temporaries: at least 4 elements each)
    auto alloc = [&](auto& b, size_t k) { return b.grow(ctx, std::max<size_t>(k, 4)) == SURTR_OK; };
    DevBuf<uint32_t> d_kind, d_index, d_cnt, d_foff, d_poff, d_set, d_val, d_order, d_lab, d_flag32; DevBuf<uint8_t> d_out; DevBuf<float> d_sph;
    if (!alloc(d_kind, n) || !alloc(d_index, n) || !alloc(d_cnt, 2 * (size_t)n) || !alloc(d_foff, n + 1) || !alloc(d_poff, n + 1) || !alloc(d_set, n) ||
        !alloc(d_lab, n) || !alloc(d_flag32, 4) || !alloc(d_out, n) || !alloc(d_sph, 3 * (size_t)n_sphere + 3)) return SURTR_E_HIP;
    HIPCHK(hipMemcpyAsync(d_kind.p, kind.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_index.p, index.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemsetAsync(d_flag32.p, 0, 16, st));
    if (n_sphere) HIPCHK(hipMemcpyAsync(d_sph.p, sphere_points, (size_t)n_sphere * 12, hipMemcpyHostToDevice, st));
    // the impact of every piece (its body's) and the impacts' spheres; the vectors live until the synchronisations below
    DevBuf<uint32_t> d_pimp; DevBuf<ImpSphere> d_imptab;
    std::vector<uint32_t> pimp; std::vector<ImpSphere> imptab;
    if (impacts && partial)
    {
        const std::vector<uint32_t>& ioff = ctx->scene_event_impacts;
        auto impact_of = [&](uint32_t body) { return (uint32_t)(std::upper_bound(ioff.begin(), ioff.end(), body) - ioff.begin()) - 1u; };
        pimp.resize(n);
        for (uint32_t p = 0; p < n_outside; ++p) pimp[p] = impact_of(body_of(skipped[p]));
        for (uint32_t f = 0; f < c.n_frag; ++f) pimp[n_outside + f] = impact_of(frag_body[f]);
        imptab.resize(impacts->n);
        fill_spheres(imptab.data(), impacts->n, impacts->sphere_off, impacts->origins, impacts->radii, impacts->partial);
        if (!alloc(d_pimp, n) || !alloc(d_imptab, imptab.size())) return SURTR_E_HIP;
        HIPCHK(hipMemcpyAsync(d_pimp.p, pimp.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(d_imptab.p, imptab.data(), imptab.size() * sizeof(ImpSphere), hipMemcpyHostToDevice, st));
    }
    const RgSrc src{d_kind.p, d_index.p};
    const PieceSet& C = ctx->cset;
    const float ox = origin ? origin[0] : 0.f, oy = origin ? origin[1] : 0.f, oz = origin ? origin[2] : 0.f;
    uint32_t* d_err = d_flag32.p;            // [0] error, [1] edges, [2] changed
    hipLaunchKernelGGL(k_rg_faces, dim3(n), dim3(SURTR_LANES), 0, st, n, src, ctx->d_frags, ctx->arena, C.pos, C.loff, C.nbr, C.vo, 0u, d_cnt.p,
                       (const uint32_t*)nullptr, (const uint32_t*)nullptr, (FaceNode*)nullptr, (P3*)nullptr, 0u, (const float*)nullptr, 0.f, 0.f, 0.f, 0.f,
                       (uint8_t*)nullptr, d_err, (const uint32_t*)nullptr, (const ImpSphere*)nullptr);
    std::vector<uint32_t> cnt(2 * (size_t)n), foff(n + 1, 0u), poff(n + 1, 0u);
    HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt.p, cnt.size() * 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (uint32_t p = 0; p < n; ++p) { foff[p + 1] = foff[p] + cnt[2 * p]; poff[p + 1] = poff[p] + cnt[2 * p + 1]; }
    const uint32_t nf = foff[n], npts = poff[n];
    DevBuf<FaceNode> d_nodes; DevBuf<P3> d_pts; DevBuf<unsigned long long> d_key, d_key2; DevBuf<uint2> d_edges;
    // One entry per touching PAIR OF FACES (k_rg_pairs does not merge the pairs of two pieces).  Solids that meet face to face
    // give a face a handful of partners, but the rule has no such bound: every face within 1e-3 of its |d| with the opposite
    // normal and an overlapping projection counts, so a stack of plates thinner than the window (2^-18 thick: up to 262
    // partners of every large face) passes 16 per face.  Such an input gets SURTR_E_CAPACITY, like a Convex of more than
    // RG_MAXH half-edges (tests/test_regroup_scenes.py: test_limit_edges_of_a_stack_of_thin_plates).
    const uint32_t cap_edges = 16u * nf + 1024u;
    stats.v[RGS_FACES] = nf; stats.v[RGS_POINTS] = npts; stats.v[RGS_CAP_EDGES] = cap_edges;
    if (!alloc(d_nodes, nf) || !alloc(d_pts, npts) || !alloc(d_key, nf) || !alloc(d_key2, nf) || !alloc(d_val, nf) || !alloc(d_order, nf) || !alloc(d_edges, cap_edges))
        return SURTR_E_HIP;
    HIPCHK(hipMemcpyAsync(d_foff.p, foff.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_poff.p, poff.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_rg_faces, dim3(n), dim3(SURTR_LANES), 0, st, n, src, ctx->d_frags, ctx->arena, C.pos, C.loff, C.nbr, C.vo, 1u, d_cnt.p,
                       d_foff.p, d_poff.p, d_nodes.p, d_pts.p, n_sphere, d_sph.p, ox, oy, oz, radius, partial ? d_out.p : (uint8_t*)nullptr, d_err,
                       (const uint32_t*)d_pimp.p, (const ImpSphere*)d_imptab.p);
    HIPCHK(hipGetLastError());
    if (partial)       // MergeOutOfImpact (:2368-2403): fragments out of the impact sphere move to bind 0; emptied compounds go
    {
        std::vector<uint8_t> flag(n);
        HIPCHK(hipMemcpyAsync(flag.data(), d_out.p, n, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (size_t i = nb; i < bind.size(); ++i)
        {
            std::set<int> outside;
            for (int cpi : bind[i]) if (flag[cpi]) outside.insert(cpi);
            for (int cpi : outside) { bind[i].erase(cpi); bind[owner[i]].insert(cpi); }      // (to its own body's bind 0)
            stats.v[RGS_OUT] += (uint32_t)outside.size();
        }
        size_t kept = nb;
        for (size_t i = nb; i < bind.size(); ++i)
            if (!bind[i].empty()) { if (kept != i) { bind[kept] = std::move(bind[i]); owner[kept] = owner[i]; } ++kept; }
        bind.resize(kept); owner.resize(kept);
    }
    set_of.assign(n, 0u);
    for (size_t i = 0; i < bind.size(); ++i) for (int p : bind[i]) set_of[p] = (uint32_t)i;
    HIPCHK(hipMemcpyAsync(d_set.p, set_of.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    std::vector<uint32_t> lab(n);
    for (uint32_t p = 0; p < n; ++p) lab[p] = p;
    HIPCHK(hipMemcpyAsync(d_lab.p, lab.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    if (nf)
    {
        const dim3 blk(256), grid((nf + 255) / 256);
        hipLaunchKernelGGL(k_rg_keys, grid, blk, 0, st, nf, d_nodes.p, d_set.p, d_key.p, d_val.p);
        size_t tmp_bytes = 0;
        (void)hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, d_key.p, d_key2.p, d_val.p, d_order.p, (int)nf, 0, 64, st);
        DevBuf<char> d_tmp;
        if (!alloc(d_tmp, tmp_bytes + 16)) return SURTR_E_HIP;
        if (hipcub::DeviceRadixSort::SortPairs(d_tmp.p, tmp_bytes, d_key.p, d_key2.p, d_val.p, d_order.p, (int)nf, 0, 64, st) != hipSuccess) return SURTR_E_HIP;
        HIPCHK(hipStreamSynchronize(st));
        hipLaunchKernelGGL(k_rg_pairs, grid, blk, 0, st, nf, d_order.p, d_key2.p, d_nodes.p, d_pts.p, d_edges.p, cap_edges, d_err + 1);
        uint32_t head[3] = {0, 0, 0};
        HIPCHK(hipMemcpyAsync(head, d_err, 12, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        stats.v[RGS_EDGES] = head[1];
        if (head[0]) return (int)head[0];
        if (head[1] > cap_edges) return SURTR_E_CAPACITY;
        const uint32_t ne = head[1];
        // min-label propagation with one pointer jump per round converges in a number of rounds bounded by the number of
        // pieces (labels only decrease); it runs until a round changes nothing -- a chain numbered against the grain takes as
        // many rounds as it is long, not 64
        uint32_t rounds = 1u;
        if (ne)
        {
            hipLaunchKernelGGL(k_rg_labels_all, dim3(1), dim3(SURTR_LANES == 1u ? 1u : RG_LABEL_THREADS)      /* (the emulation runs one thread per workgroup) */, 0, st, ne, d_edges.p, n, d_lab.p, d_err + 2);
            HIPCHK(hipMemcpyAsync(&rounds, d_err + 2, 4, hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipMemcpyAsync(lab.data(), d_lab.p, (size_t)n * 4, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));        // (the one synchronisation of the label phase)
        if (rounds == 0xFFFFFFFFu) return SURTR_E_STATE;      // (cannot happen: see the bound in the kernel; never hand out unconverged labels)
        ctx->regroup_rounds = rounds;
        stats.v[RGS_ROUNDS] = rounds;
    }
    // HandleConvexIsland's outcome: per compound, groups = label classes in order of their lowest piece; the first stays
    std::vector<std::set<int>> extra; std::vector<uint32_t> extra_owner;
    for (size_t i = 0; i < bind.size(); ++i)
    {
        std::set<int>& local = bind[i];
        if (local.size() <= 1) continue;
        std::vector<std::pair<uint32_t, std::set<int>>> groups;      // (label = lowest piece, members)
        for (int p : local)
        {
            bool found = false;
            for (auto& g : groups) if (g.first == lab[p]) { g.second.insert(p); found = true; break; }
            if (!found) groups.push_back({lab[p], std::set<int>{p}});
        }
        std::sort(groups.begin(), groups.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
        if (groups.size() >= 2)
        {
            local = groups[0].second;
            for (size_t g = 1; g < groups.size(); ++g) { extra.push_back(groups[g].second); extra_owner.push_back(owner[i]); }
        }
    }
    // per body: its bind 0, its cell binds, then the groups HandleConvexIsland split off them -- the order of the one-body call
    uint32_t at = 0, nc = 0;
    compound_off[0] = 0;
    auto emit = [&](const std::set<int>& s) { for (int p : s) compound_piece[at++] = p; compound_off[++nc] = at; };
    for (uint32_t b = 0; b < nb; ++b)
    {
        if (body_compound_off) body_compound_off[b] = nc;
        for (size_t i = 0; i < bind.size(); ++i) if (owner[i] == b) emit(bind[i]);
        for (size_t i = 0; i < extra.size(); ++i) if (extra_owner[i] == b) emit(extra[i]);
    }
    if (body_compound_off) body_compound_off[nb] = nc;
    *n_compounds = nc;
    return SURTR_OK;
}

extern "C" int surtr_event_regroup(surtr_ctx* ctx, int partial, uint32_t n_sphere, const float* sphere_points, const float origin[3], float radius,
                                   uint32_t* n_pieces_out, uint32_t* n_compounds, uint32_t* compound_off, int32_t* compound_piece)
{
    return regroup_event(ctx, partial, n_sphere, sphere_points, origin, radius, n_pieces_out, n_compounds, compound_off, compound_piece, nullptr);
}

extern "C" int surtr_event_regroup_bodies(surtr_ctx* ctx, int partial, uint32_t n_sphere, const float* sphere_points, const float origin[3], float radius,
                                          uint32_t* n_pieces_out, uint32_t* n_compounds, uint32_t* compound_off, int32_t* compound_piece,
                                          uint32_t* n_bodies, uint32_t* body_compound_off)
{
    if (!ctx || !n_bodies) return SURTR_E_INVALID;
    *n_bodies = (uint32_t)std::max<size_t>(ctx->scene_event_compound.size(), 1);
    return regroup_event(ctx, partial, n_sphere, sphere_points, origin, radius, n_pieces_out, n_compounds, compound_off, compound_piece, body_compound_off);
}

extern "C" int surtr_event_regroup_impacts(surtr_ctx* ctx, int partial, uint32_t n_impacts, const uint32_t* sphere_off, const float* sphere_points,
                                           const float* origins, const float* radii, uint32_t* n_pieces_out, uint32_t* n_compounds, uint32_t* compound_off,
                                           int32_t* compound_piece, uint32_t* n_bodies, uint32_t* body_compound_off)
{
    if (!ctx || !n_bodies || !n_impacts) return SURTR_E_INVALID;
    // the last event must be surtr_scene_fracture_impacts' over as many impacts: their target lists say which body is whose
    if (!ctx->have_event || ctx->scene_event_compound.empty() || ctx->scene_event_impacts.size() != (size_t)n_impacts + 1 ||
        ctx->scene_event_impacts.back() != ctx->scene_event_compound.size())
        return SURTR_E_STATE;
    *n_bodies = (uint32_t)ctx->scene_event_compound.size();
    if (!partial) return regroup_event(ctx, 0, 0, nullptr, nullptr, 0.f, n_pieces_out, n_compounds, compound_off, compound_piece, body_compound_off);
    const int rc = spheres_valid(n_impacts, sphere_off, origins, radii, sphere_points != nullptr);
    if (rc) return rc;
    const ImpactSpheres imp{n_impacts, sphere_off, origins, radii};
    return regroup_event(ctx, 1, sphere_off[n_impacts], sphere_points, origins, radii[0], n_pieces_out, n_compounds, compound_off, compound_piece, body_compound_off, &imp);
}

// The same with a flag per impact: the bodies of an impact with partial[i] == 0 are tested against no sphere (a "no sphere" entry of
// the table, for which k_rg_faces writes 0) and so see no MergeOutOfImpact; their cloud range may be empty.
extern "C" int surtr_event_regroup_impacts_partial(surtr_ctx* ctx, const uint8_t* partial, uint32_t n_impacts, const uint32_t* sphere_off, const float* sphere_points,
                                                   const float* origins, const float* radii, uint32_t* n_pieces_out, uint32_t* n_compounds,
                                                   uint32_t* compound_off, int32_t* compound_piece, uint32_t* n_bodies, uint32_t* body_compound_off)
{
    if (!ctx || !n_bodies || !n_impacts || !partial) return SURTR_E_INVALID;
    if (!ctx->have_event || ctx->scene_event_compound.empty() || ctx->scene_event_impacts.size() != (size_t)n_impacts + 1 ||
        ctx->scene_event_impacts.back() != ctx->scene_event_compound.size())
        return SURTR_E_STATE;
    *n_bodies = (uint32_t)ctx->scene_event_compound.size();
    if (std::find_if(partial, partial + n_impacts, [](uint8_t f) { return f != 0; }) == partial + n_impacts)      // no sphere at all
        return regroup_event(ctx, 0, 0, nullptr, nullptr, 0.f, n_pieces_out, n_compounds, compound_off, compound_piece, body_compound_off);
    const int rc = spheres_valid(n_impacts, sphere_off, origins, radii, sphere_points != nullptr);
    if (rc) return rc;
    const ImpactSpheres imp{n_impacts, sphere_off, origins, radii, partial};
    return regroup_event(ctx, 1, sphere_off[n_impacts], sphere_points, origins, radii[0], n_pieces_out, n_compounds, compound_off, compound_piece, body_compound_off, &imp);
}

// ---- the out-of-sphere mask of the pieces a click is about to break (k_scene_outside) ----
// The listed compounds' pieces, in the order given, each compound in resident order; SURTR_E_CAPACITY for a Convex k_scene_outside
// has no room for.  Nothing has been enqueued when an error is returned.
static int outside_list(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, std::vector<uint32_t>& list)
{
    if (!ctx || !n_targets || !compounds) return SURTR_E_INVALID;
    if (!ctx->n_pieces || ctx->scene_off.size() < 2 || ctx->scene_off.back() != ctx->n_pieces) return SURTR_E_STATE;
    list.clear();
    for (uint32_t t = 0; t < n_targets; ++t)
    {
        if ((size_t)compounds[t] + 1 >= ctx->scene_off.size()) return SURTR_E_INVALID;
        for (uint32_t p = ctx->scene_off[compounds[t]]; p < ctx->scene_off[compounds[t] + 1]; ++p)
        {
            if (ctx->h_vo[1][p + 1] - ctx->h_vo[1][p] > RG_MAXH || ctx->h_ho[1][p + 1] - ctx->h_ho[1][p] > RG_MAXH)
            {
                ctx->err = "surtr_scene_outside: a Convex of more than " + std::to_string(RG_MAXH) + " half-edges";
                return SURTR_E_CAPACITY;
            }
            list.push_back(p);
        }
    }
    return SURTR_OK;
}

// Enqueues the list's upload and the kernel on the context's stream.  The list goes through a buffer the context keeps, which grows
// (an allocation, and a free of the smaller one, which waits for the device) only when a call lists more pieces than any before it.
// Its source is pageable host memory: the runtime has staged such a copy when hipMemcpyAsync returns, as for the tables of
// surtr_scene_commit and scene_sync_device, so the caller's vector may go at once.
static int outside_enqueue(surtr_ctx* ctx, const std::vector<uint32_t>& list, uint32_t n_sphere, const float* dev_sphere_points, const float origin[3],
                           float radius, uint8_t* dev_outside)
{
    const uint32_t n = (uint32_t)list.size();
    (void)hipSetDevice(ctx->device);
    const int rc = ctx->d_outside_list.grow(ctx, n, (size_t)n + n / 4 + 64);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ctx->d_outside_list.p, list.data(), (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
    const PieceSet& C = ctx->cset;
    hipLaunchKernelGGL(k_scene_outside, dim3(n), dim3(SURTR_LANES), 0, ctx->stream, n, (const uint32_t*)ctx->d_outside_list.p, (const float*)C.pos.p,
                       (const uint32_t*)C.loff.p, (const int32_t*)C.nbr.p, (const uint32_t*)C.vo.p, n_sphere, dev_sphere_points, origin[0], origin[1], origin[2],
                       radius, dev_outside);
    HIPCHK(hipGetLastError());
    return SURTR_OK;
}

extern "C" int surtr_scene_outside_dev(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, uint32_t n_sphere, const float* dev_sphere_points,
                                       const float origin[3], float radius, uint8_t* dev_outside, size_t capacity_bytes)
{
    if (!ctx || !origin || !dev_outside || (n_sphere && !dev_sphere_points)) return SURTR_E_INVALID;
    std::vector<uint32_t> list;
    const int rc = outside_list(ctx, n_targets, compounds, list);
    if (rc) return rc;
    if (capacity_bytes < list.size()) return SURTR_E_CAPACITY;
    return outside_enqueue(ctx, list, n_sphere, dev_sphere_points, origin, radius, dev_outside);
}

// The host half of surtr_scene_outside and surtr_scene_outside_impacts, once the list is laid out and the capacity checked: the cloud goes
// up, `enqueue(dev cloud, dev mask)` runs the kernel, the n bytes come down; synchronises (the temporaries are freed when it returns).
template <class Enqueue>
static int outside_host(surtr_ctx* ctx, uint32_t n_sphere, const float* sphere_points, uint32_t n, uint8_t* outside, Enqueue enqueue)
{
    (void)hipSetDevice(ctx->device);
    DevBuf<float> d_sph; DevBuf<uint8_t> d_out;
    if (d_sph.grow(ctx, 3 * (size_t)n_sphere + 3) || d_out.grow(ctx, std::max<size_t>(n, 4))) return SURTR_E_HIP;
    if (n_sphere) HIPCHK(hipMemcpyAsync(d_sph.p, sphere_points, (size_t)n_sphere * 12, hipMemcpyHostToDevice, ctx->stream));
    const int rc = enqueue(d_sph.p, d_out.p);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(outside, d_out.p, n, hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SURTR_OK;
}

extern "C" int surtr_scene_outside(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, uint32_t n_sphere, const float* sphere_points,
                                   const float origin[3], float radius, uint32_t cap, uint32_t* n, uint8_t* outside)
{
    if (!ctx || !n || !origin || (n_sphere && !sphere_points)) return SURTR_E_INVALID;
    std::vector<uint32_t> list;
    const int rc = outside_list(ctx, n_targets, compounds, list);
    if (rc) return rc;
    *n = (uint32_t)list.size();
    if (!outside) return SURTR_OK;
    if (cap < *n) return SURTR_E_CAPACITY;
    return outside_host(ctx, n_sphere, sphere_points, *n, outside,
                        [&](const float* d_sph, uint8_t* d_out) { return outside_enqueue(ctx, list, n_sphere, d_sph, origin, radius, d_out); });
}

// ---- the same mask for the impacts of one frame, a sphere per piece (k_scene_outside_impacts) ----
// Checks everything and lays out the staged words: list[n] | impact of every listed piece [n] | ImpSphere[n_impacts].  Nothing has been
// enqueued when an error is returned.
static int outside_impacts_stage(surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* target_off, const uint32_t* compounds, const uint32_t* sphere_off,
                                 const float* origins, const float* radii, bool have_points, uint32_t* n_out)
{
    if (!ctx || !n_impacts || !sphere_off || !origins || !radii) return SURTR_E_INVALID;
    if (!ctx->n_pieces || ctx->scene_off.size() < 2 || ctx->scene_off.back() != ctx->n_pieces) return SURTR_E_STATE;
    int rc = impacts_valid(ctx, n_impacts, target_off, compounds);
    if (rc) return rc;
    if ((rc = spheres_valid(n_impacts, sphere_off, origins, radii, have_points)) != SURTR_OK) return rc;
    std::vector<uint32_t> list, imp, one;
    for (uint32_t i = 0; i < n_impacts; ++i)
    {
        rc = outside_list(ctx, target_off[i + 1] - target_off[i], compounds + target_off[i], one);
        if (rc) return rc;
        list.insert(list.end(), one.begin(), one.end()); imp.insert(imp.end(), one.size(), i);
    }
    static_assert(sizeof(ImpSphere) == 32, "the sphere table is staged as eight words per impact");
    const size_t n = list.size(), at_tab = (2 * n + 3) & ~(size_t)3;      // (the table 16-byte aligned)
    std::vector<uint32_t>& H = ctx->h_outside_stage;
    H.assign(at_tab + 8 * (size_t)n_impacts, 0u);
    memcpy(H.data(), list.data(), n * 4); memcpy(H.data() + n, imp.data(), n * 4);
    std::vector<ImpSphere> tab(n_impacts);
    fill_spheres(tab.data(), n_impacts, sphere_off, origins, radii);
    memcpy(H.data() + at_tab, tab.data(), tab.size() * sizeof(ImpSphere));
    *n_out = (uint32_t)n;
    return SURTR_OK;
}

// One copy of the staged words (the context's vector: pageable memory has left its source when hipMemcpyAsync returns) and one launch.
static int outside_impacts_enqueue(surtr_ctx* ctx, uint32_t n, const float* dev_sphere_points, uint8_t* dev_outside)
{
    const std::vector<uint32_t>& H = ctx->h_outside_stage;
    (void)hipSetDevice(ctx->device);
    const int rc = ctx->d_outside_list.grow(ctx, H.size(), H.size() + H.size() / 4 + 64);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(ctx->d_outside_list.p, H.data(), H.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    const uint32_t* d = ctx->d_outside_list.p; const size_t at_tab = (2 * (size_t)n + 3) & ~(size_t)3;
    const PieceSet& C = ctx->cset;
    hipLaunchKernelGGL(k_scene_outside_impacts, dim3(n), dim3(SURTR_LANES), 0, ctx->stream, n, d, d + n, (const ImpSphere*)(d + at_tab), (const float*)C.pos.p,
                       (const uint32_t*)C.loff.p, (const int32_t*)C.nbr.p, (const uint32_t*)C.vo.p, dev_sphere_points, dev_outside);
    HIPCHK(hipGetLastError());
    return SURTR_OK;
}

extern "C" int surtr_scene_outside_impacts_dev(surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* target_off, const uint32_t* compounds, const uint32_t* sphere_off,
                                               const float* dev_sphere_points, const float* origins, const float* radii, uint8_t* dev_outside,
                                               size_t capacity_bytes)
{
    if (!ctx || !dev_outside) return SURTR_E_INVALID;
    uint32_t n = 0;
    const int rc = outside_impacts_stage(ctx, n_impacts, target_off, compounds, sphere_off, origins, radii, dev_sphere_points != nullptr, &n);
    if (rc) return rc;
    if (capacity_bytes < n) return SURTR_E_CAPACITY;
    return outside_impacts_enqueue(ctx, n, dev_sphere_points, dev_outside);
}

extern "C" int surtr_scene_outside_impacts(surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* target_off, const uint32_t* compounds, const uint32_t* sphere_off,
                                           const float* sphere_points, const float* origins, const float* radii, uint32_t cap, uint32_t* n, uint8_t* outside)
{
    if (!ctx || !n) return SURTR_E_INVALID;
    const int rc = outside_impacts_stage(ctx, n_impacts, target_off, compounds, sphere_off, origins, radii, sphere_points != nullptr, n);
    if (rc) return rc;
    if (!outside) return SURTR_OK;
    if (cap < *n) return SURTR_E_CAPACITY;
    return outside_host(ctx, sphere_off[n_impacts], sphere_points, *n, outside,
                        [&](const float* d_sph, uint8_t* d_out) { return outside_impacts_enqueue(ctx, *n, d_sph, d_out); });
}
