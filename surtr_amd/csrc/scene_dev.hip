// scene_dev.hip -- the resident pieces as a scene of several bodies (FractureStorage::CompoundVec) and the bookkeeping of
// ExecuteFractureRoutine (Src/Surtr.cpp:1829-1883) on the device, so that pick -> fracture -> commit -> pick never leaves HBM.
//
//   surtr_scene_set_compounds / _get_compounds   compound c = resident pieces [compound_off[c], compound_off[c + 1])
//   surtr_scene_transform_compound                Poly::Transform of one compound's pieces (:1846-1851)
//   surtr_scene_set_poses / _get_poses / _apply_pose   a rigid pose per compound (WorldMatrix, :347-352), kept on the host next to the
//                                                 table; the posed queries (query_dev.hip) read it, apply_pose bakes it in
//   surtr_scene_fracture_event(_async)            the event over the pieces of one compound
//   surtr_scene_apply_poses / _fracture_bodies(_async)   the same for every body a click hits at once: one bake, one event whose pair
//                                                 list is target-major (the mask of surtr_scene_outside, regroup_dev.hip)
//   surtr_scene_fracture_impacts(_async)          the same for the impacts of one frame, each with its own sphere and its own instance
//                                                 of the pattern (surtr_place_cells_impacts): the pair list is impact-major
//   surtr_scene_fragments(_async)                 the resident pieces of some compounds as the current fragments (InitCompound, :2499-2529):
//                                                 the device twin of surtr_load_fragments, one chunked copy kernel into the event arena
//   surtr_scene_commit                            erase the event's compound(s), push back what they broke into (:1856-1875): one
//                                                 gather kernel from the old pieces and the event arena into spare buffers, then a swap
// The layout of the new pieces is laid out on the host from the small tables (piece offsets, fragment records), as
// surtr_pieces_from_event does; no solid leaves HBM.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <functional>
#include <utility>

#include "surtr_ctx.h"

using namespace pieces;
using scene::IDENTITY; using scene::rigid_pose; using scene::SolidsIn;

namespace {

// What piece p of the new scene is made from, per set s (0 = Mesh, 1 = Convex): src[p] >= 0 an old resident piece, -(f + 1)
// fragment f (or staged piece f of an append); sv / sh its first vertex / ring entry in its source (the old set, or the arena / the
// staged set), dv / dh in the new set (n + 1 entries: the last is the total).  The device copy of scene::Layout.
struct GatherTab { const int32_t* src; const uint32_t* sv[2]; const uint32_t* sh[2]; const uint32_t* dv[2]; const uint32_t* dh[2]; };
struct SolidsOut { float* pos; uint32_t* loff; int32_t* nbr; };

// One workgroup per (new piece, set): positions and rings are copied, ring offsets rebased; the last piece writes the closing
// sentinel.  Plain stores to disjoint ranges, no atomics.
__global__ __launch_bounds__(SURTR_WG) void k_scene_gather(uint32_t n, GatherTab T, SolidsIn other0, SolidsIn other1, SolidsIn old0, SolidsIn old1, SolidsOut new0, SolidsOut new1)
{
    const uint32_t p = blockIdx.x >> 1, set = blockIdx.x & 1u;
    if (p >= n) return;
    const bool frag = T.src[p] < 0;
    const SolidsIn O = frag ? (set ? other1 : other0) : (set ? old1 : old0); const SolidsOut D = set ? new1 : new0;
    const float* spos = O.pos; const uint32_t* sloff = O.loff; const int32_t* snbr = O.nbr;
    const uint32_t sv = T.sv[set][p], sh = T.sh[set][p], dv = T.dv[set][p], dh = T.dh[set][p];
    const uint32_t nv = T.dv[set][p + 1] - dv, nh = T.dh[set][p + 1] - dh;
    for (uint32_t i = threadIdx.x; i < 3u * nv; i += group_size()) D.pos[3 * (size_t)dv + i] = spos[3 * (size_t)sv + i];
    for (uint32_t v = threadIdx.x; v < nv; v += group_size()) D.loff[dv + v] = dh + (sloff[sv + v] - sh);
    for (uint32_t e = threadIdx.x; e < nh; e += group_size()) D.nbr[dh + e] = snbr[sh + e];
    if (p + 1u == n && threadIdx.x == 0) D.loff[dv + nv] = dh + nh;
}

// ---- surtr_scene_fragments: resident pieces -> event arena.  The host cuts the copy into chunks of at most FRAG_SPAN words, so that a
// body of 50 000 vertices is spread over as many workgroups as thousands of small pieces beside it.  Pieces that follow each other in
// the resident set follow each other in the arena too, so a run of them is ONE range per array whatever the pieces' sizes: the chunks
// know nothing of pieces.  Every array is copied as 32-bit words (positions keep their bits); `add` rebases the ring offsets.  The
// host starts every run at an arena slot congruent to its source modulo 4, and every chunk but a run's first at a source multiple of
// 4: source and destination are 16-byte aligned together, and all but a head and a tail of up to 3 words moves as 128-bit words.
enum : uint32_t { FC_POS = 0, FC_NBR = 1, FC_LOFF = 2, FC_LLEN = 3, FC_ORDER = 4, FC_SET1 = 16 };
#define FRAG_SPAN 4096u
struct alignas(16) FragChunk { uint32_t kind, n, add, pad; unsigned long long src, dst; };      // kind = FC_* (| FC_SET1: from the Convex set)
struct alignas(16) Words4 { uint32_t w[4]; };
struct PieceWords { const uint32_t* pos; const uint32_t* nbr; const uint32_t* loff; const uint32_t* llen; };

// One workgroup per chunk.  FC_ORDER chunks fill the size-class lists of the fragment table: fragment dst + i goes to slot[src + i].
// Plain stores to disjoint ranges; no atomics, no LDS.
__global__ __launch_bounds__(SURTR_WG) void k_frags_from_pieces(uint32_t n_chunks, const FragChunk* __restrict__ chunks, const uint32_t* __restrict__ slot,
                                                                PieceWords S0, PieceWords S1, Arena A, uint32_t* __restrict__ forder)
{
    if (blockIdx.x >= n_chunks) return;
    const FragChunk C = chunks[blockIdx.x];
    const uint32_t kind = C.kind & 15u, n = C.n;
    if (kind == FC_ORDER)
    {
        for (uint32_t i = threadIdx.x; i < n; i += group_size()) forder[slot[C.src + i]] = (uint32_t)C.dst + i;
        return;
    }
    const PieceWords S = (C.kind & FC_SET1) ? S1 : S0;
    const uint32_t* s = kind == FC_POS ? S.pos : kind == FC_NBR ? S.nbr : kind == FC_LOFF ? S.loff : S.llen;
    uint32_t* d = kind == FC_POS ? (uint32_t*)A.pos : kind == FC_NBR ? (uint32_t*)A.nbr : kind == FC_LOFF ? A.loff : A.llen;
    s += C.src; d += C.dst;
    const uint32_t add = C.add;
    if ((C.src ^ C.dst) & 3ull)      // (never with the host's layout: the two are not aligned together, word by word)
    {
        for (uint32_t i = threadIdx.x; i < n; i += group_size()) d[i] = s[i] + add;
        return;
    }
    const uint32_t lead = (4u - (uint32_t)(C.src & 3ull)) & 3u, head = lead < n ? lead : n, n4 = (n - head) >> 2, tail = head + 4u * n4;
    for (uint32_t i = threadIdx.x; i < head; i += group_size()) d[i] = s[i] + add;
    const Words4* s4 = (const Words4*)(s + head); Words4* d4 = (Words4*)(d + head);
    for (uint32_t i = threadIdx.x; i < n4; i += group_size())
    {
        Words4 w = s4[i];
        w.w[0] += add; w.w[1] += add; w.w[2] += add; w.w[3] += add;
        d4[i] = w;
    }
    for (uint32_t i = tail + threadIdx.x; i < n; i += group_size()) d[i] = s[i] + add;
}

bool valid_table(uint32_t n_compounds, const uint32_t* off, uint32_t n_pieces)
{
    if (!n_compounds || !off || off[0] != 0u || off[n_compounds] != n_pieces) return false;
    for (uint32_t c = 0; c < n_compounds; ++c) if (off[c + 1] <= off[c]) return false;
    return true;
}

// The event of every scene entrance.  Impact i owns compounds[target_off[i] .. target_off[i + 1]), all checked by the caller; the
// one-compound and the bodies entrance are one "impact" over the plain placement.  The pairs are impact-major, then target-major in
// the order given, then cell-major over the target's pieces, as surtr_fracture_event takes them: every target's fragments come out as
// the event of that target alone gives them.  `outside` holds one byte per piece of the listed compounds in that order and is spread
// over all resident pieces.  instance_cells (surtr_scene_fracture_impacts): impact i's cells are those of its own instance of the
// pattern, i * n_cells + c (after surtr_place_cells_patterns: imp_cell_base[i] + c), and the event reads the instance planes.
int scene_event(surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* target_off, const uint32_t* compounds, uint32_t cell_begin, uint32_t cell_end,
                const uint8_t* outside, uint32_t flags, bool instance_cells)
{
    const uint32_t n_targets = target_off[n_impacts];
    // the cells of impact i: [cell_begin, cell_end) of its instance, or of the plain placement; after surtr_place_cells_patterns every
    // cell of its instance, which has as many as its own pattern
    const bool library = instance_cells && ctx->imp_library;
    auto first_cell = [&](uint32_t i) { return library ? ctx->imp_cell_base[i] : (instance_cells ? i * ctx->n_cells : 0u) + cell_begin; };
    auto cell_count = [&](uint32_t i) { return library ? ctx->imp_cell_base[i + 1] - ctx->imp_cell_base[i] : cell_end - cell_begin; };
    uint64_t n_pairs = 0;
    for (uint32_t i = 0; i < n_impacts; ++i)
    {
        uint64_t total = 0;
        for (uint32_t t = target_off[i]; t < target_off[i + 1]; ++t) total += ctx->scene_off[compounds[t] + 1] - ctx->scene_off[compounds[t]];
        n_pairs += (uint64_t)cell_count(i) * total;
    }
    if (n_pairs > 0xFFFFFFFFull) return SURTR_E_INVALID;
    std::vector<uint32_t> cell, piece;
    cell.reserve((size_t)n_pairs); piece.reserve((size_t)n_pairs);
    std::vector<uint8_t> mask;
    if (outside) mask.assign(ctx->n_pieces, 0);
    size_t at = 0;
    for (uint32_t i = 0; i < n_impacts; ++i)
        for (uint32_t t = target_off[i]; t < target_off[i + 1]; ++t)
        {
            const uint32_t p0 = ctx->scene_off[compounds[t]], m = ctx->scene_off[compounds[t] + 1] - p0, c0 = first_cell(i), nc = cell_count(i);
            for (uint32_t c = 0; c < nc; ++c)
                for (uint32_t q = 0; q < m; ++q) { cell.push_back(c0 + c); piece.push_back(p0 + q); }
            if (outside) memcpy(mask.data() + p0, outside + at, m);
            at += m;
        }
    const std::vector<uint32_t> targets(compounds, compounds + n_targets), offs(target_off, target_off + n_impacts + 1);      // (launch_event clears the context's)
    int rc;
    if (instance_cells)
    {
        ImpactPlanesScope instance_planes(ctx);
        rc = surtr_event_pairs_masked(ctx, (uint32_t)cell.size(), cell.data(), piece.data(), outside ? mask.data() : nullptr, flags);
    }
    else rc = surtr_event_pairs_masked(ctx, (uint32_t)cell.size(), cell.data(), piece.data(), outside ? mask.data() : nullptr, flags);
    if (rc) return rc;
    ctx->scene_event_compound = targets;
    if (instance_cells) ctx->scene_event_impacts = offs;
    return SURTR_OK;
}

} // namespace

namespace scene {

const float IDENTITY[16] = {1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};

// Rigid: finite, last row exactly (0, 0, 0, 1), max |A^T A - I| <= 1e-4, det A > 0; in double from the floats.
bool rigid_pose(const float* W)
{
    for (int i = 0; i < 16; ++i) if (!(std::fabs(W[i]) <= 3.4028235e38f)) return false;
    if (W[12] != 0.f || W[13] != 0.f || W[14] != 0.f || W[15] != 1.f) return false;
    double A[3][3];
    for (int r = 0; r < 3; ++r) for (int k = 0; k < 3; ++k) A[r][k] = (double)W[4 * r + k];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
        {
            const double g = A[0][i] * A[0][j] + A[1][i] * A[1][j] + A[2][i] * A[2][j] - (i == j ? 1.0 : 0.0);
            if (!(std::fabs(g) <= 1e-4)) return false;
        }
    const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) - A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                       A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
    return det > 0.0;
}

int regather(surtr_ctx* ctx, const Layout& L, const SolidsIn other[2], std::vector<float>&& pose, std::chrono::steady_clock::time_point* gathered)
{
    hipStream_t st = ctx->stream;
    const std::vector<int32_t>& src = L.src;
    const std::vector<uint32_t>* sv = L.sv; const std::vector<uint32_t>* sh = L.sh; const std::vector<uint32_t>* dv = L.dv; const std::vector<uint32_t>* dh = L.dh;
    const uint32_t n = (uint32_t)src.size();
    // ---- spare buffers, tables, gather
    for (int s = 0; s < 2; ++s)
    {
        auto& B = ctx->spare[s];
        if (grow_pieces(ctx, B.pos, 3 * (size_t)dv[s][n] + 3) || grow_pieces(ctx, B.loff, (size_t)dv[s][n] + 1) || grow_pieces(ctx, B.nbr, (size_t)dh[s][n] + 1) ||
            grow_pieces(ctx, B.vo, n + 1))
            return SURTR_E_HIP;
    }
    if (grow_pieces(ctx, ctx->d_commit_src, n) || grow_pieces(ctx, ctx->d_commit_tab, (size_t)8 * (n + 1))) return SURTR_E_HIP;
    if (!ctx->d_upload_err) { if (ctx->d_upload_err.grow(ctx, 4)) return SURTR_E_HIP; ++ctx->upload_allocs; }
    HIPCHK(hipMemsetAsync(ctx->d_upload_err, 0, 4, st));
    uint32_t* d = ctx->d_commit_tab; const size_t w = (size_t)n + 1;
    GatherTab T{ctx->d_commit_src, {d, d + w}, {d + 2 * w, d + 3 * w}, {d + 4 * w, d + 5 * w}, {d + 6 * w, d + 7 * w}};
    HIPCHK(hipMemcpyAsync(ctx->d_commit_src, src.data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
    for (int s = 0; s < 2; ++s)
    {
        HIPCHK(hipMemcpyAsync((void*)T.sv[s], sv[s].data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync((void*)T.sh[s], sh[s].data(), (size_t)n * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync((void*)T.dv[s], dv[s].data(), w * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync((void*)T.dh[s], dh[s].data(), w * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(ctx->spare[s].vo, dv[s].data(), w * 4, hipMemcpyHostToDevice, st));
    }
    PieceSet& M = ctx->mset; PieceSet& C = ctx->cset;
    hipLaunchKernelGGL(k_scene_gather, dim3(2 * n), dim3(SURTR_WG), 0, st, n, T, other[0], other[1], SolidsIn{M.pos, M.loff, M.nbr}, SolidsIn{C.pos, C.loff, C.nbr},
                       SolidsOut{ctx->spare[0].pos, ctx->spare[0].loff, ctx->spare[0].nbr}, SolidsOut{ctx->spare[1].pos, ctx->spare[1].loff, ctx->spare[1].nbr});
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));      // (the old buffers may be freed below)
    if (gathered) *gathered = std::chrono::steady_clock::now();
    // ---- the gathered solids become the resident ones; the buffers they came from are the next gather's spare ones and get the
    //      same room now, so that a scene of steady size commits (or is edited) without an allocation from the second time on
    for (int s = 0; s < 2; ++s)
    {
        PieceSet& S = s ? C : M; auto& B = ctx->spare[s];
        std::swap(S.pos, B.pos); std::swap(S.loff, B.loff); std::swap(S.nbr, B.nbr); std::swap(S.vo, B.vo);
        if (grow_pieces(ctx, B.pos, 3 * (size_t)dv[s][n] + 3) || grow_pieces(ctx, B.loff, (size_t)dv[s][n] + 1) || grow_pieces(ctx, B.nbr, (size_t)dh[s][n] + 1) ||
            grow_pieces(ctx, B.vo, n + 1))
            return SURTR_E_HIP;
    }
    const std::vector<uint32_t> bo[2] = {sphere_offsets(n, dv[0].data()), sphere_offsets(n, dv[1].data())};
    for (int s = 0; s < 2; ++s)
    {
        PieceSet& S = s ? C : M;
        int rc = reserve_set(ctx, S, n, dv[s][n], dh[s][n], bo[s][n]);
        if (rc) return rc;
        rc = derive_set(ctx, S, n, dv[s][n], bo[s], false);
        if (rc) return rc;
    }
    set_piece_stats(ctx, n, dv[0].data(), dh[0].data(), dv[1].data(), dh[1].data());      // (resets the table and the poses)
    ctx->scene_off = L.table;
    ctx->scene_pose = std::move(pose); ctx->scene_dev_stale = true;
    return SURTR_OK;
}

} // namespace scene

extern "C" {

int surtr_scene_set_poses(surtr_ctx* ctx, uint32_t n_compounds, const float* world)
{
    if (!ctx || !world) return SURTR_E_INVALID;
    if (!ctx->n_pieces) return SURTR_E_STATE;
    if ((size_t)n_compounds + 1 != ctx->scene_off.size()) return SURTR_E_INVALID;
    for (uint32_t c = 0; c < n_compounds; ++c) if (!rigid_pose(world + 16 * (size_t)c)) return SURTR_E_INVALID;
    ctx->scene_pose.assign(world, world + 16 * (size_t)n_compounds);
    ctx->scene_dev_stale = true;
    return SURTR_OK;
}

int surtr_scene_get_poses(surtr_ctx* ctx, uint32_t cap, uint32_t* n_compounds, float* world)
{
    if (!ctx || !n_compounds) return SURTR_E_INVALID;
    if (!ctx->n_pieces) return SURTR_E_STATE;
    const uint32_t nc = (uint32_t)ctx->scene_off.size() - 1u;
    *n_compounds = nc;
    if (!world) return SURTR_OK;
    if (cap < nc) return SURTR_E_CAPACITY;
    if (ctx->scene_pose.empty()) for (uint32_t c = 0; c < nc; ++c) memcpy(world + 16 * (size_t)c, IDENTITY, 64);
    else memcpy(world, ctx->scene_pose.data(), (size_t)64 * nc);
    return SURTR_OK;
}

int surtr_scene_apply_pose(surtr_ctx* ctx, uint32_t compound)
{
    if (!ctx) return SURTR_E_INVALID;
    if (!ctx->n_pieces) return SURTR_E_STATE;
    if (compound + 1u >= ctx->scene_off.size()) return SURTR_E_INVALID;
    if (ctx->scene_pose.empty() || memcmp(ctx->scene_pose.data() + 16 * (size_t)compound, IDENTITY, 64) == 0) return SURTR_OK;
    const uint32_t n = ctx->scene_off[compound + 1] - ctx->scene_off[compound];
    std::vector<float> w((size_t)16 * n);
    for (uint32_t k = 0; k < n; ++k) memcpy(w.data() + 16 * (size_t)k, ctx->scene_pose.data() + 16 * (size_t)compound, 64);
    const int rc = transform_range(ctx, ctx->scene_off[compound], n, w.data());
    if (rc) return rc;
    memcpy(ctx->scene_pose.data() + 16 * (size_t)compound, IDENTITY, 64);
    ctx->scene_dev_stale = true;
    return SURTR_OK;
}

int surtr_scene_apply_poses(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds)
{
    if (!ctx || (n_targets && !compounds)) return SURTR_E_INVALID;
    if (!ctx->n_pieces) return SURTR_E_STATE;
    for (uint32_t t = 0; t < n_targets; ++t) if ((size_t)compounds[t] + 1 >= ctx->scene_off.size()) return SURTR_E_INVALID;
    // the compounds whose pose is not bit for bit the identity, each once (a compound named twice is baked once, as two calls of
    // surtr_scene_apply_pose would)
    std::vector<uint32_t> moved, p0, np; std::vector<float> w;
    for (uint32_t t = 0; t < n_targets && !ctx->scene_pose.empty(); ++t)
    {
        const uint32_t c = compounds[t];
        const float* W = ctx->scene_pose.data() + 16 * (size_t)c;
        if (memcmp(W, IDENTITY, 64) == 0 || std::find(moved.begin(), moved.end(), c) != moved.end()) continue;
        moved.push_back(c); p0.push_back(ctx->scene_off[c]); np.push_back(ctx->scene_off[c + 1] - ctx->scene_off[c]);
        for (uint32_t k = 0; k < np.back(); ++k) w.insert(w.end(), W, W + 16);
    }
    if (moved.empty()) return SURTR_OK;      // (nothing at all: a pending event stays committable)
    const int rc = transform_ranges(ctx, (uint32_t)moved.size(), p0.data(), np.data(), w.data());
    if (rc) return rc;
    for (uint32_t c : moved) memcpy(ctx->scene_pose.data() + 16 * (size_t)c, IDENTITY, 64);
    ctx->scene_dev_stale = true;
    return SURTR_OK;
}

int surtr_scene_set_compounds(surtr_ctx* ctx, uint32_t n_compounds, const uint32_t* compound_off)
{
    if (!ctx) return SURTR_E_INVALID;
    if (!ctx->n_pieces) return SURTR_E_STATE;
    if (!valid_table(n_compounds, compound_off, ctx->n_pieces)) return SURTR_E_INVALID;
    ctx->scene_off.assign(compound_off, compound_off + n_compounds + 1);
    ctx->scene_event_compound.clear();   // (an event's compound numbers belong to the table they were given in)
    scene_reset_poses(ctx);              // (and so does a pose)
    return SURTR_OK;
}

int surtr_scene_get_compounds(surtr_ctx* ctx, uint32_t cap, uint32_t* n_compounds, uint32_t* compound_off)
{
    if (!ctx || !n_compounds) return SURTR_E_INVALID;
    if (!ctx->n_pieces) return SURTR_E_STATE;
    *n_compounds = (uint32_t)ctx->scene_off.size() - 1u;
    if (!compound_off) return SURTR_OK;
    if (cap < ctx->scene_off.size()) return SURTR_E_CAPACITY;
    memcpy(compound_off, ctx->scene_off.data(), ctx->scene_off.size() * 4);
    return SURTR_OK;
}

int surtr_scene_transform_compound(surtr_ctx* ctx, uint32_t compound, uint32_t n, const float* world)
{
    if (!ctx || !world) return SURTR_E_INVALID;
    if (!ctx->n_pieces) return SURTR_E_STATE;
    if (compound + 1u >= ctx->scene_off.size() || n != ctx->scene_off[compound + 1] - ctx->scene_off[compound]) return SURTR_E_INVALID;
    return transform_range(ctx, ctx->scene_off[compound], n, world);
}

int surtr_scene_fracture_event_async(surtr_ctx* ctx, uint32_t compound, uint32_t cell_begin, uint32_t cell_end, const uint8_t* outside, uint32_t flags)
{
    if (!ctx) return SURTR_E_INVALID;
    if (!ctx->n_pieces || !ctx->planes_ready) return SURTR_E_STATE;
    if ((size_t)compound + 1 >= ctx->scene_off.size() || cell_end > ctx->n_cells || cell_begin > cell_end) return SURTR_E_INVALID;
    const uint32_t one[2] = {0u, 1u};
    return scene_event(ctx, 1, one, &compound, cell_begin, cell_end, outside, flags, false);
}

int surtr_scene_fracture_event(surtr_ctx* ctx, uint32_t compound, uint32_t cell_begin, uint32_t cell_end, const uint8_t* outside, uint32_t flags,
                               surtr_counts* counts)
{
    return event_sync_counts(ctx, surtr_scene_fracture_event_async(ctx, compound, cell_begin, cell_end, outside, flags), counts);
}

int surtr_scene_fracture_bodies_async(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, uint32_t cell_begin, uint32_t cell_end,
                                      const uint8_t* outside, uint32_t flags)
{
    if (!ctx) return SURTR_E_INVALID;
    if (!ctx->n_pieces || !ctx->planes_ready) return SURTR_E_STATE;
    if (!n_targets || !compounds || cell_end > ctx->n_cells || cell_begin > cell_end) return SURTR_E_INVALID;
    for (uint32_t t = 0; t < n_targets; ++t)
        if ((size_t)compounds[t] + 1 >= ctx->scene_off.size() || (t && compounds[t] >= compounds[t - 1])) return SURTR_E_INVALID;      // strictly descending
    const uint32_t one[2] = {0u, n_targets};
    return scene_event(ctx, 1, one, compounds, cell_begin, cell_end, outside, flags, false);
}

int surtr_scene_fracture_bodies(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, uint32_t cell_begin, uint32_t cell_end,
                                const uint8_t* outside, uint32_t flags, surtr_counts* counts)
{
    return event_sync_counts(ctx, surtr_scene_fracture_bodies_async(ctx, n_targets, compounds, cell_begin, cell_end, outside, flags), counts);
}

int surtr_scene_fracture_impacts_async(surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* target_off, const uint32_t* compounds, uint32_t cell_begin,
                                       uint32_t cell_end, const uint8_t* outside, uint32_t flags)
{
    if (!ctx || !n_impacts) return SURTR_E_INVALID;
    if (!ctx->n_pieces || !ctx->n_impacts_placed || ctx->n_impacts_placed != n_impacts) return SURTR_E_STATE;
    const int rc = impacts_valid(ctx, n_impacts, target_off, compounds);
    if (rc) return rc;
    // (after surtr_place_cells_patterns the instances differ in their cells: all of them, or nothing)
    if (ctx->imp_library ? cell_begin != 0u || cell_end != SURTR_CELLS_ALL : cell_end > ctx->n_cells || cell_begin > cell_end) return SURTR_E_INVALID;
    return scene_event(ctx, n_impacts, target_off, compounds, cell_begin, cell_end, outside, flags, true);
}

int surtr_scene_fracture_impacts(surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* target_off, const uint32_t* compounds, uint32_t cell_begin,
                                 uint32_t cell_end, const uint8_t* outside, uint32_t flags, surtr_counts* counts)
{
    return event_sync_counts(ctx, surtr_scene_fracture_impacts_async(ctx, n_impacts, target_off, compounds, cell_begin, cell_end, outside, flags), counts);
}

int surtr_scene_fragments_async(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, int render_convex, uint32_t flags)
{
    if (!ctx) return SURTR_E_INVALID;
    if (!ctx->n_pieces || ctx->scene_off.size() < 2) return SURTR_E_STATE;
    if ((flags & ~(uint32_t)SURTR_EVT_RENDER) || (compounds && !n_targets)) return SURTR_E_INVALID;
    const uint32_t nc = (uint32_t)ctx->scene_off.size() - 1u;
    if (!compounds) n_targets = nc;
    // ---- everything is checked, laid out and grown before anything is enqueued
    uint64_t n64 = 0;
    {
        std::vector<uint8_t> seen(nc, 0);
        for (uint32_t t = 0; t < n_targets; ++t)
        {
            const uint32_t c = compounds ? compounds[t] : t;
            if (c >= nc || seen[c]) return SURTR_E_INVALID;
            seen[c] = 1; n64 += ctx->scene_off[c + 1] - ctx->scene_off[c];
        }
    }
    if (n64 == 0) return SURTR_E_INVALID;
    if (n64 > 0x7FFFFFFFull) return SURTR_E_CAPACITY;      // (more than any fragment table holds: ensure_arena)
    const uint32_t n = (uint32_t)n64;
    (void)hipSetDevice(ctx->device);
    // The staged words: FragRec[n] | cursors[CUR_STATS_WORDS] | surtr_counts (padded to 12 words) | slot[n] | chunks.  The first three go
    // to d_frags, the arena's cursors and d_counts; the last two are the kernel's own tables.
    constexpr size_t FR_W = sizeof(FragRec) / 4, CH_W = sizeof(FragChunk) / 4, CNT_W = 12;
    static_assert(sizeof(FragRec) % 4 == 0 && sizeof(surtr_counts) <= CNT_W * 4 && sizeof(FragChunk) == 32, "staging layout");
    const size_t at_cur = FR_W * n, at_cnt = at_cur + CUR_STATS_WORDS, at_slot = (at_cnt + CNT_W + 3) & ~(size_t)3, at_chunk = (at_slot + n + 3) & ~(size_t)3;
    std::vector<uint32_t>& H = ctx->h_frag_stage;
    H.assign(at_chunk, 0u);
    std::vector<FragChunk> chunks;
    auto cut = [&](uint32_t kind, uint64_t src, uint64_t dst, uint64_t count, uint32_t add) {
        while (count)
        {
            const uint32_t take = (uint32_t)std::min<uint64_t>(count, FRAG_SPAN - (src & 3u));      // the next chunk starts at a multiple of 4
            chunks.push_back(FragChunk{kind, take, add, 0u, src, dst});
            src += take; dst += take; count -= take;
        }
    };
    uint32_t vmax = 0, hmax = 0, cvmax = 0, chmax = 0;
    uint64_t vcur = 0, hcur = 0, slotV[2] = {0, 0}, slotH[2] = {0, 0};
    for (int slot = 0; slot < 2; ++slot)      // the Mesh slots of all fragments first, then the Convex slots, as surtr_load_fragments lays them out
    {
        const int set = (slot || render_convex) ? 1 : 0;
        const std::vector<uint32_t>& vo = ctx->h_vo[set]; const std::vector<uint32_t>& ho = ctx->h_ho[set];
        const uint32_t from = set ? FC_SET1 : 0u;
        const uint64_t v0 = vcur, h0 = hcur;
        uint32_t k = 0, prev = 0xFFFFFFFFu;
        uint64_t run_sv = 0, run_sh = 0, run_dv = 0, run_dh = 0, run_nv = 0, run_nh = 0;
        auto close_run = [&]() {
            if (!run_nv) return;
            cut(FC_POS | from, 3 * run_sv, 3 * run_dv, 3 * run_nv, 0u); cut(FC_NBR | from, run_sh, run_dh, run_nh, 0u);
            cut(FC_LOFF | from, run_sv, run_dv, run_nv, (uint32_t)(run_dh - run_sh)); cut(FC_LLEN | from, run_sv, run_dv, run_nv, 0u);
            run_nv = run_nh = 0;
        };
        for (uint32_t t = 0; t < n_targets; ++t)
        {
            const uint32_t c = compounds ? compounds[t] : t;
            for (uint32_t p = ctx->scene_off[c]; p < ctx->scene_off[c + 1]; ++p, ++k)
            {
                const uint32_t sv = vo[p], nv = vo[p + 1] - sv, sh = ho[p], nh = ho[p + 1] - sh;
                if (p != prev + 1u || prev == 0xFFFFFFFFu)      // a new run: its arena slots congruent to the source's modulo 4
                {
                    close_run();
                    vcur += (sv - vcur) & 3u; hcur += (sh - hcur) & 3u;
                    run_sv = sv; run_sh = sh; run_dv = vcur; run_dh = hcur;
                }
                prev = p;
                FragRec r; memset(&r, 0, sizeof(r));
                memcpy(&r, H.data() + FR_W * k, sizeof(r));
                if (slot == 0)
                {
                    r.cell = (int32_t)c; r.piece = (int32_t)p; r.island = 0;
                    r.mv_off = (uint32_t)vcur; r.mv_n = nv; r.mh_off = (uint32_t)hcur; r.mh_n = nh;
                    vmax = std::max(vmax, nv); hmax = std::max(hmax, nh);
                    uint32_t cls = 0; while ((nv >> (cls + 1u)) != 0u && cls < 15u) ++cls;      // size classes of k_frag_table
                    H[at_slot + k] = cls;      // (the slot itself once the arena, and with it the lists' stride, is known)
                }
                else
                {
                    r.cv_off = (uint32_t)vcur; r.cv_n = nv; r.ch_off = (uint32_t)hcur; r.ch_n = nh;
                    cvmax = std::max(cvmax, nv); chmax = std::max(chmax, nh);
                }
                memcpy(H.data() + FR_W * k, &r, sizeof(r));
                vcur += nv; hcur += nh; run_nv += nv; run_nh += nh;
            }
        }
        close_run();
        slotV[slot] = vcur - v0; slotH[slot] = hcur - h0;
    }
    if (vcur > 0xFFFFFFF0ull || hcur > 0xFFFFFFF0ull) return SURTR_E_CAPACITY;
    cut(FC_ORDER, 0, 0, n, 0u);
    int rc = frags_reserve(ctx, n, vmax, hmax, cvmax, chmax, slotV[0], slotV[1], slotH[0], slotH[1]);
    if (rc) return rc;
    if (n > ctx->cap_frags || vcur > ctx->arena.capV || hcur > ctx->arena.capH) return SURTR_E_CAPACITY;
    if ((rc = ctx->d_frag_tab.grow(ctx, (size_t)n + CH_W * chunks.size() + 4, ((size_t)n + CH_W * chunks.size()) * 5 / 4 + 64)) != SURTR_OK) return rc;
    for (uint32_t k = 0; k < n; ++k)
    {
        const uint32_t cls = H[at_slot + k];
        H[at_slot + k] = cls * ctx->cap_frags + H[at_cur + CUR_CLS_FRAG + cls]++;
    }
    H[at_cur + CUR_V] = (uint32_t)vcur; H[at_cur + CUR_H] = (uint32_t)hcur;
    surtr_counts c; memset(&c, 0, sizeof(c)); c.n_frag = n; c.n_pairs = n;
    memcpy(H.data() + at_cnt, &c, sizeof(c));
    H.resize(at_chunk + CH_W * chunks.size());
    memcpy(H.data() + at_chunk, chunks.data(), chunks.size() * sizeof(FragChunk));
    // ---- enqueue.  (The staging vector is the context's: pageable memory has left its source when hipMemcpyAsync returns, and the
    //      vector lives until the next call refills it, as the tables of scene_sync_device do.)
    hipStream_t st = ctx->stream;
    ctx->have_event = false; ctx->scene_event_compound.clear();
    uint32_t* d_slot = ctx->d_frag_tab; const size_t dev_chunk = ((size_t)n + 3) & ~(size_t)3;      // (16-byte aligned chunk records)
    HIPCHK(hipMemcpyAsync(ctx->d_frags, H.data(), (size_t)n * sizeof(FragRec), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->arena.cursors, H.data() + at_cur, CUR_STATS_WORDS * 4, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(ctx->d_counts, H.data() + at_cnt, sizeof(c), hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_slot, H.data() + at_slot, (H.size() - at_slot) * 4, hipMemcpyHostToDevice, st));
    static_assert(sizeof(float) == 4 && sizeof(int32_t) == 4, "the solids are copied as 32-bit words");
    PieceSet& M = ctx->mset; PieceSet& C = ctx->cset;
    const PieceWords S0{(const uint32_t*)M.pos.p, (const uint32_t*)M.nbr.p, M.loff.p, M.llen.p}, S1{(const uint32_t*)C.pos.p, (const uint32_t*)C.nbr.p, C.loff.p, C.llen.p};
    PROF_BEGIN(12);
    hipLaunchKernelGGL(k_frags_from_pieces, dim3((uint32_t)chunks.size()), dim3(SURTR_WG), 0, st, (uint32_t)chunks.size(),
                       (const FragChunk*)(d_slot + dev_chunk), (const uint32_t*)d_slot, S0, S1, ctx->arena, ctx->d_forder.p);
    PROF_END(12);
    HIPCHK(hipGetLastError());
    rc = frags_present(ctx, (flags & SURTR_EVT_RENDER) != 0u, render_convex);
    if (rc) ctx->have_event = false;
    return rc;
}

int surtr_scene_fragments(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, int render_convex, uint32_t flags, surtr_counts* counts)
{
    return event_sync_counts(ctx, surtr_scene_fragments_async(ctx, n_targets, compounds, render_convex, flags), counts);
}

int surtr_scene_commit(surtr_ctx* ctx, uint32_t n_compounds, const uint32_t* compound_off, const int32_t* compound_piece, uint32_t* n_pieces_out,
                       uint32_t* first_new_compound, uint32_t* n_new_compounds, int32_t* src_out)
{
    if (!ctx || !compound_off || (n_compounds && compound_off[n_compounds] && !compound_piece)) return SURTR_E_INVALID;
    if (!ctx->n_pieces || !ctx->have_event || !ctx->frags_of_pieces || ctx->scene_event_compound.empty() ||
        (size_t)*std::max_element(ctx->scene_event_compound.begin(), ctx->scene_event_compound.end()) + 1 >= ctx->scene_off.size())
        return SURTR_E_STATE;
    (void)hipSetDevice(ctx->device);
    Timer timer(ctx);
    const auto clock0 = std::chrono::steady_clock::now();
    surtr_counts c;
    if (surtr_event_counts(ctx, &c) != SURTR_OK) return SURTR_E_STATE;      // the event failed: nothing to commit
    // ---- everything is checked and laid out before anything is written
    const uint32_t np = ctx->n_pieces;
    // strictly descending; after surtr_scene_fracture_impacts inside an impact only: sorted here, for the poses below (the layout
    // reads is_target and the order of the returned compounds, neither of which asks for an order of the targets)
    std::vector<uint32_t> targets = ctx->scene_event_compound;
    std::sort(targets.begin(), targets.end(), std::greater<uint32_t>());
    std::vector<uint8_t> is_target(ctx->scene_off.size() - 1, 0);
    for (uint32_t t : targets) is_target[t] = 1;
    std::vector<uint32_t> skipped;      // of every target, ascending: surtr_event_regroup's numbers
    for (uint32_t k = 0; k + 1 < ctx->scene_off.size() && ctx->last_outside.size() == np; ++k)
        for (uint32_t p = ctx->scene_off[k]; is_target[k] && p < ctx->scene_off[k + 1]; ++p) if (ctx->last_outside[p]) skipped.push_back(p);
    const uint32_t n_skip = (uint32_t)skipped.size(), n_in = n_skip + c.n_frag;
    if (compound_off[0] != 0u || compound_off[n_compounds] != n_in) return SURTR_E_INVALID;
    {
        std::vector<uint8_t> seen(n_in, 0);
        for (uint32_t k = 0; k < n_compounds; ++k)
        {
            if (compound_off[k + 1] < compound_off[k] || compound_off[k + 1] > n_in) return SURTR_E_INVALID;
            for (uint32_t i = compound_off[k]; i < compound_off[k + 1]; ++i)
            {
                const int32_t q = compound_piece[i];
                if (q < 0 || (uint32_t)q >= n_in || seen[q]) return SURTR_E_INVALID;
                seen[q] = 1;
            }
        }
    }
    std::vector<FragRec> fr(c.n_frag); std::vector<uint32_t> fstat(c.n_frag);
    if (c.n_frag)
    {
        HIPCHK(hipMemcpy(fr.data(), ctx->d_frags, (size_t)c.n_frag * sizeof(FragRec), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(fstat.data(), ctx->d_frag_status, (size_t)c.n_frag * 4, hipMemcpyDeviceToHost));
    }
    scene::Layout L;
    // the pieces of every other compound first, in their old order: a compound moves down by the number of targets below it
    for (uint32_t k = 0; k + 1 < ctx->scene_off.size(); ++k)
    {
        if (is_target[k]) continue;
        for (uint32_t p = ctx->scene_off[k]; p < ctx->scene_off[k + 1]; ++p) L.push_old(ctx, p);
        L.table.push_back((uint32_t)L.src.size());
    }
    const uint32_t first_new = (uint32_t)L.table.size() - 1u;
    // then the members of every returned compound: skipped pieces as they stand, fragments from the arena with the Convex the
    // context holds.  A fragment that is no solid, or a flagged one, is left out; a compound left without pieces is not created.
    for (uint32_t k = 0; k < n_compounds; ++k)
    {
        for (uint32_t i = compound_off[k]; i < compound_off[k + 1]; ++i)
        {
            const uint32_t q = (uint32_t)compound_piece[i];
            if (q < n_skip) { L.push_old(ctx, skipped[q]); continue; }
            const uint32_t f = q - n_skip;
            if (fr[f].mv_n < 4 || fr[f].cv_n < 4 || fstat[f] != 0u) continue;
            L.push_other(f, 0, fr[f].mv_off, fr[f].mv_n, fr[f].mh_off, fr[f].mh_n);
            L.push_other(f, 1, fr[f].cv_off, fr[f].cv_n, fr[f].ch_off, fr[f].ch_n);
        }
        L.close_compound();
    }
    const uint32_t n = (uint32_t)L.src.size();
    if (n == 0) return SURTR_E_INVALID;      // (a scene without a piece: as surtr_pieces_from_event refuses to keep nothing)
    // the poses of the surviving compounds move down with them; what the event made is in world space already (InitCompound(compound, false))
    std::vector<float> pose = ctx->scene_pose;
    if (!pose.empty())
    {
        for (uint32_t target : targets) pose.erase(pose.begin() + 16 * (size_t)target, pose.begin() + 16 * (size_t)(target + 1u));      // (highest first)
        for (size_t k = first_new; k + 1 < L.table.size(); ++k) pose.insert(pose.end(), IDENTITY, IDENTITY + 16);
    }
    const SolidsIn arena[2] = {{ctx->arena.pos, ctx->arena.loff, ctx->arena.nbr}, {ctx->arena.pos, ctx->arena.loff, ctx->arena.nbr}};
    auto clock1 = clock0;
    {
        const int rc = scene::regather(ctx, L, arena, std::move(pose), &clock1);
        if (rc) return rc;
    }
    const std::vector<int32_t>& src = L.src; const std::vector<uint32_t>& table = L.table;
    ctx->have_event = true;       // the event's fragments are still in the arena, as after surtr_pieces_from_event
    ctx->frags_of_pieces = false; // (but the pieces they came from have moved)
    if (n_pieces_out) *n_pieces_out = n;
    if (first_new_compound) *first_new_compound = first_new;
    if (n_new_compounds) *n_new_compounds = (uint32_t)table.size() - 1u - first_new;
    if (src_out) memcpy(src_out, src.data(), (size_t)n * 4);
    const int rc = finish_upload(ctx, n, false);      // (synchronises: the derived data is there)
    ctx->commit_ms[0] = std::chrono::duration<float, std::milli>(clock1 - clock0).count();
    ctx->commit_ms[1] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - clock1).count();
    return rc;
}

int surtr_scene_commit_times(surtr_ctx* ctx, float* gather_ms, float* derive_ms)
{
    if (!ctx) return SURTR_E_INVALID;
    if (gather_ms) *gather_ms = ctx->commit_ms[0];
    if (derive_ms) *derive_ms = ctx->commit_ms[1];
    return SURTR_OK;
}

} // extern "C"
