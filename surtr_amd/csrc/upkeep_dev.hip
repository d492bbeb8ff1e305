// upkeep_dev.hip -- what a frame loop with a rigid-body solver needs of the resident scene besides the fracture cycle:
//
//   surtr_scene_bounds(_dev)   the world-space box of every body (and piece) from the resident positions and the poses, every frame:
//                              k_bounds_pieces (one workgroup per piece), then k_bounds_bodies (one wave per body over its pieces)
//   surtr_scene_remove         erase bodies: the kept pieces are gathered into the commit's spare buffers and swapped in
//   surtr_scene_append         push_back bodies from host arrays: staged, vetted as an upload, gathered behind the old pieces
//   surtr_scene_cull           mark the light bodies and those outside a keep box on the device (k_cull_mark), remove them
// The edits lay the new set out with scene::Layout and make it with scene::regather (scene_dev.hip), as surtr_scene_commit does: no
// solid leaves HBM, and the derived data of the whole scene is rebuilt.
#include <cmath>
#include <cstring>

#include "surtr_ctx.h"

using namespace pieces;

namespace {

#define BOUNDS_MAX 3.4028235e38f

struct BoundsIn { const float* pos; const uint32_t* vo; const uint32_t* piece_comp; const float* pose; uint32_t n; };      // pose: 16 floats per compound, or null

// min / max of two partial boxes and the "not finite" flag across the lanes of a wave: lane 0 ends with the wave's
__device__ __forceinline__ void wave_box(float lo[3], float hi[3], uint32_t& flag, uint32_t& count)
{
    for (int d = SURTR_LANES / 2; d >= 1; d >>= 1)
    {
        for (int c = 0; c < 3; ++c)
        {
            const float ol = __shfl_down(lo[c], d, SURTR_LANES), oh = __shfl_down(hi[c], d, SURTR_LANES);
            lo[c] = ol < lo[c] ? ol : lo[c]; hi[c] = oh > hi[c] ? oh : hi[c];
        }
        flag |= __shfl_down(flag, d, SURTR_LANES);
        count += __shfl_down(count, d, SURTR_LANES);
    }
}

// Stage 1: the box of every piece under its body's pose.  One workgroup per piece; its threads stride over the piece's vertices
// (coalesced 12-byte positions), a wave reduction, the waves' partial boxes through LDS, one plain 32-byte store.  The pose is read
// once per thread from 64 bytes every thread of the workgroup shares; a pose that is bit for bit the identity transforms nothing,
// as surtr_scene_apply_pose rewrites nothing then (an infinite coordinate stays infinite instead of turning into inf * 0).
__global__ __launch_bounds__(SURTR_WG) void k_bounds_pieces(BoundsIn B, surtr_bounds* __restrict__ out)
{
    __shared__ float part[SURTR_NWAVE][6];
    __shared__ uint32_t partf[SURTR_NWAVE];
    const uint32_t p = blockIdx.x;
    if (p >= B.n) return;
    const uint32_t a = B.vo[p], b = B.vo[p + 1];
    float W[16];
    bool posed = false;
    if (B.pose)
    {
        const float* src = B.pose + 16 * (size_t)B.piece_comp[p];
        for (int k = 0; k < 16; ++k)
        {
            W[k] = src[k];
            posed = posed || __float_as_uint(W[k]) != (k % 5 == 0 ? 0x3F800000u : 0u);
        }
    }
    float lo[3] = {BOUNDS_MAX, BOUNDS_MAX, BOUNDS_MAX}, hi[3] = {-BOUNDS_MAX, -BOUNDS_MAX, -BOUNDS_MAX};
    uint32_t flag = 0, count = 0;
    for (uint32_t v = a + threadIdx.x; v < b; v += group_size())
    {
        float x[3] = {B.pos[3 * (size_t)v], B.pos[3 * (size_t)v + 1], B.pos[3 * (size_t)v + 2]};
        if (posed) transform_coord(W, x[0], x[1], x[2], x);
        for (int c = 0; c < 3; ++c)
        {
            if (fabsf(x[c]) <= BOUNDS_MAX) { lo[c] = x[c] < lo[c] ? x[c] : lo[c]; hi[c] = x[c] > hi[c] ? x[c] : hi[c]; }
            else flag = SURTR_BOUNDS_NONFINITE;
        }
    }
    wave_box(lo, hi, flag, count);
    if (lane_id() == 0) { for (int c = 0; c < 3; ++c) { part[wave_id()][c] = lo[c]; part[wave_id()][3 + c] = hi[c]; } partf[wave_id()] = flag; }
    __syncthreads();
    if (threadIdx.x == 0)
    {
        for (uint32_t w = 1; w < group_waves(); ++w)
        {
            for (int c = 0; c < 3; ++c)
            {
                lo[c] = part[w][c] < lo[c] ? part[w][c] : lo[c];
                hi[c] = part[w][3 + c] > hi[c] ? part[w][3 + c] : hi[c];
            }
            flag |= partf[w];
        }
        surtr_bounds r;
        for (int c = 0; c < 3; ++c) { r.lo[c] = lo[c]; r.hi[c] = hi[c]; }
        r.n_vertices = b - a; r.status = flag;
        out[p] = r;
    }
}

// Stage 2: the box of every body from its pieces' records, which lie next to each other.  One wave per body (four bodies per
// workgroup); its lanes stride over the records, a wave reduction, lane 0 stores.  No LDS, no barrier.
__global__ __launch_bounds__(SURTR_WG) void k_bounds_bodies(uint32_t n_comp, const uint32_t* __restrict__ comp_off, const surtr_bounds* __restrict__ piece,
                                                            surtr_bounds* __restrict__ out)
{
    const uint32_t c = blockIdx.x * group_waves() + wave_id();
    if (c >= n_comp) return;
    const uint32_t p0 = comp_off[c], p1 = comp_off[c + 1];
    float lo[3] = {BOUNDS_MAX, BOUNDS_MAX, BOUNDS_MAX}, hi[3] = {-BOUNDS_MAX, -BOUNDS_MAX, -BOUNDS_MAX};
    uint32_t flag = 0, count = 0;
    for (uint32_t p = p0 + lane_id(); p < p1; p += SURTR_LANES)
    {
        const surtr_bounds r = piece[p];
        for (int k = 0; k < 3; ++k) { lo[k] = r.lo[k] < lo[k] ? r.lo[k] : lo[k]; hi[k] = r.hi[k] > hi[k] ? r.hi[k] : hi[k]; }
        flag |= r.status; count += r.n_vertices;
    }
    wave_box(lo, hi, flag, count);
    if (lane_id() == 0)
    {
        surtr_bounds r;
        for (int k = 0; k < 3; ++k) { r.lo[k] = lo[k]; r.hi[k] = hi[k]; }
        r.n_vertices = count; r.status = flag;
        out[c] = r;
    }
}

// surtr_scene_cull: one lane per body reads its mass record and its bounds and writes its reason byte.
struct CullBox { float lo[3], hi[3]; uint32_t on; };
__global__ void k_cull_mark(uint32_t n_comp, const surtr_mass* __restrict__ mass, const surtr_bounds* __restrict__ box, float min_mass, CullBox keep,
                            uint8_t* __restrict__ reason)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_comp) return;
    uint32_t r = 0;
    if (mass[c].status == 0u && mass[c].mass <= (double)min_mass) r |= SURTR_CULL_LIGHT;
    if (keep.on && box[c].status == 0u)
    {
        bool apart = false;
        for (int k = 0; k < 3; ++k) apart = apart || box[c].hi[k] < keep.lo[k] || box[c].lo[k] > keep.hi[k];
        if (apart) r |= SURTR_CULL_OUTSIDE;
    }
    reason[c] = (uint8_t)r;
}

// The float poses on the device, behind scene_sync_device's refresh of the tables (which raises scene_posef_stale).  -> null when the
// scene has no pose table: every pose is the identity.
int sync_posef(surtr_ctx* ctx, const float** out)
{
    *out = nullptr;
    if (ctx->scene_pose.empty()) return SURTR_OK;
    if (ctx->scene_posef_stale || !ctx->d_posef)
    {
        std::vector<float>& P = ctx->h_posef_stage;      // (pageable: it has left the vector when hipMemcpyAsync returns, as in scene_sync_device)
        P = ctx->scene_pose;
        const int rc = ctx->d_posef.grow(ctx, P.size(), P.size() + P.size() / 4);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(ctx->d_posef.p, P.data(), P.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        ctx->scene_posef_stale = false;
    }
    *out = ctx->d_posef.p;
    return SURTR_OK;
}

// What every edit leaves behind once scene::regather has installed the new set (set_piece_stats has forgotten the event).
int finish_edit(surtr_ctx* ctx, uint32_t n, bool had_event)
{
    ctx->have_event = had_event;      // the last event's fragments are still in the arena, as after a commit
    ctx->frags_of_pieces = false;     // (but the pieces have moved: no commit, no mask)
    ctx->last_outside.clear(); ctx->scene_event_compound.clear(); ctx->scene_event_impacts.clear();
    return finish_upload(ctx, n, false);      // (synchronises: the derived data is there)
}

} // namespace

extern "C" {

int surtr_scene_bounds_dev(surtr_ctx* ctx, int set, void* dev_body, size_t body_cap_bytes, void* dev_piece_or_null, size_t piece_cap_bytes)
{
    if (!ctx || !dev_body || (set != 0 && set != 1)) return SURTR_E_INVALID;
    const PieceSet& P = set ? ctx->cset : ctx->mset;
    if (!P.pos || !P.vo || ctx->n_pieces == 0 || ctx->scene_off.size() < 2) return SURTR_E_STATE;
    const uint32_t nc = (uint32_t)ctx->scene_off.size() - 1u, n = ctx->n_pieces;
    if ((size_t)nc * sizeof(surtr_bounds) > body_cap_bytes || (dev_piece_or_null && (size_t)n * sizeof(surtr_bounds) > piece_cap_bytes)) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    SceneDev sc;
    int rc = scene_sync_device(ctx, &sc);
    if (rc) return rc;
    const float* posef = nullptr;
    if ((rc = sync_posef(ctx, &posef)) != SURTR_OK) return rc;
    surtr_bounds* piece = (surtr_bounds*)dev_piece_or_null;
    if (!piece)
    {
        if ((rc = ctx->d_bounds_piece.grow(ctx, n, (size_t)n + n / 4 + 64)) != SURTR_OK) return rc;
        piece = ctx->d_bounds_piece.p;
    }
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_bounds_pieces, dim3(n), dim3(SURTR_WG), 0, st, BoundsIn{P.pos, P.vo, sc.piece_comp, posef, n}, piece);
    hipLaunchKernelGGL(k_bounds_bodies, dim3((nc + SURTR_NWAVE - 1u) / SURTR_NWAVE), dim3(SURTR_WG), 0, st, nc, sc.comp_off, (const surtr_bounds*)piece,
                       (surtr_bounds*)dev_body);
    HIPCHK(hipGetLastError());
    return SURTR_OK;
}

int surtr_scene_bounds(surtr_ctx* ctx, int set, uint32_t* n, surtr_bounds* out)
{
    if (!ctx || !n || (set != 0 && set != 1)) return SURTR_E_INVALID;
    const PieceSet& P = set ? ctx->cset : ctx->mset;
    if (!P.pos || !P.vo || ctx->n_pieces == 0 || ctx->scene_off.size() < 2) return SURTR_E_STATE;
    const uint32_t nc = (uint32_t)ctx->scene_off.size() - 1u;
    if (out && *n < nc) { *n = nc; return SURTR_E_CAPACITY; }
    *n = nc;
    if (!out) return SURTR_OK;
    DevBuf<surtr_bounds> d;
    int rc = d.grow(ctx, nc);
    if (rc == SURTR_OK) rc = surtr_scene_bounds_dev(ctx, set, d.p, (size_t)nc * sizeof(surtr_bounds), nullptr, 0);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, d.p, (size_t)nc * sizeof(surtr_bounds), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return SURTR_OK;
}

int surtr_scene_remove(surtr_ctx* ctx, uint32_t n_remove, const uint32_t* compounds, uint32_t* n_pieces_out, int32_t* src_out)
{
    if (!ctx || (n_remove && !compounds)) return SURTR_E_INVALID;
    if (!ctx->n_pieces || ctx->scene_off.size() < 2) return SURTR_E_STATE;
    const uint32_t nc = (uint32_t)ctx->scene_off.size() - 1u;
    std::vector<uint8_t> gone(nc, 0);
    for (uint32_t k = 0; k < n_remove; ++k)
    {
        if (compounds[k] >= nc || gone[compounds[k]]) return SURTR_E_INVALID;
        gone[compounds[k]] = 1;
    }
    if (n_remove >= nc) return SURTR_E_INVALID;      // (a scene without a body: as a commit that keeps nothing)
    if (n_remove == 0)                               // (nothing to erase: nothing moves, nothing is forgotten)
    {
        if (n_pieces_out) *n_pieces_out = ctx->n_pieces;
        for (uint32_t p = 0; src_out && p < ctx->n_pieces; ++p) src_out[p] = (int32_t)p;
        return SURTR_OK;
    }
    (void)hipSetDevice(ctx->device);
    Timer timer(ctx);
    scene::Layout L;
    std::vector<float> pose;
    for (uint32_t c = 0; c < nc; ++c)
    {
        if (gone[c]) continue;
        for (uint32_t p = ctx->scene_off[c]; p < ctx->scene_off[c + 1]; ++p) L.push_old(ctx, p);
        L.table.push_back((uint32_t)L.src.size());
        if (!ctx->scene_pose.empty()) pose.insert(pose.end(), ctx->scene_pose.begin() + 16 * (size_t)c, ctx->scene_pose.begin() + 16 * (size_t)(c + 1u));
    }
    const uint32_t n = (uint32_t)L.src.size();
    const bool had_event = ctx->have_event;
    const scene::SolidsIn none[2] = {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}};      // (every piece is an old one)
    const int rc = scene::regather(ctx, L, none, std::move(pose), nullptr);
    if (rc) return rc;
    if (n_pieces_out) *n_pieces_out = n;
    if (src_out) memcpy(src_out, L.src.data(), (size_t)n * 4);
    return finish_edit(ctx, n, had_event);
}

int surtr_scene_append(surtr_ctx* ctx, uint32_t n_bodies, const uint32_t* body_piece_off, const uint32_t* mvo, const float* mpos, const uint32_t* moff,
                       const int32_t* mnbr, const uint32_t* cvo, const float* cpos, const uint32_t* coff, const int32_t* cnbr, const float* world,
                       uint32_t* first_new_compound)
{
    if (!ctx || !n_bodies || !body_piece_off || !mvo || !mpos || !moff || !mnbr || !cvo || !cpos || !coff || !cnbr) return SURTR_E_INVALID;
    if (!ctx->n_pieces || ctx->scene_off.size() < 2) return SURTR_E_STATE;
    if (body_piece_off[0] != 0u) return SURTR_E_INVALID;
    for (uint32_t b = 0; b < n_bodies; ++b) if (body_piece_off[b + 1] <= body_piece_off[b]) return SURTR_E_INVALID;
    const uint32_t m = body_piece_off[n_bodies], np = ctx->n_pieces, nc = (uint32_t)ctx->scene_off.size() - 1u;
    if ((uint64_t)np + m > 0x7FFFFFFFull) return SURTR_E_CAPACITY;
    for (uint32_t b = 0; world && b < n_bodies; ++b) if (!scene::rigid_pose(world + 16 * (size_t)b)) return SURTR_E_INVALID;
    // ---- the host checks of surtr_upload_pieces
    std::vector<uint32_t> ho[2];
    if (host_offsets(m, mvo, moff, ho[0]) || host_offsets(m, cvo, coff, ho[1])) return SURTR_E_INVALID;
    for (int s = 0; s < 2; ++s)
        if ((uint64_t)ctx->h_vo[s][np] + (s ? cvo : mvo)[m] > 0xFFFFFFF0ull || (uint64_t)ctx->h_ho[s][np] + ho[s][m] > 0xFFFFFFF0ull) return SURTR_E_CAPACITY;
    (void)hipSetDevice(ctx->device);
    Timer timer(ctx);
    hipStream_t st = ctx->stream;
    // ---- staged as they came (offsets from 0 per set) and vetted there: the scene is not touched before the links have passed
    if (!ctx->d_upload_err) { if (ctx->d_upload_err.grow(ctx, 4)) return SURTR_E_HIP; ++ctx->upload_allocs; }
    HIPCHK(hipMemsetAsync(ctx->d_upload_err, 0, 4, st));
    scene::SolidsIn staged[2];
    for (int s = 0; s < 2; ++s)
    {
        auto& G = ctx->stage[s];
        const uint32_t* vo = s ? cvo : mvo; const float* pos = s ? cpos : mpos; const uint32_t* off = s ? coff : moff; const int32_t* nbr = s ? cnbr : mnbr;
        const uint32_t V = vo[m], H = off[V];
        if (grow_pieces(ctx, G.pos, 3 * (size_t)V + 3) || grow_pieces(ctx, G.loff, (size_t)V + 1) || grow_pieces(ctx, G.llen, V) || grow_pieces(ctx, G.nbr, (size_t)H + 1) ||
            grow_pieces(ctx, G.vo, m + 1) || grow_pieces(ctx, G.dup, m + 1))
            return SURTR_E_HIP;
        HIPCHK(hipMemcpyAsync(G.pos, pos, (size_t)V * 12, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(G.loff, off, (size_t)(V + 1) * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(G.nbr, nbr, (size_t)H * 4, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(G.vo, vo, (size_t)(m + 1) * 4, hipMemcpyHostToDevice, st));
        const int rc = vet_solids(ctx, m, V, H, G.vo, G.loff, G.nbr, G.llen, G.dup);
        if (rc) return rc;
        staged[s] = scene::SolidsIn{G.pos, G.loff, G.nbr};
    }
    uint32_t err = 0;
    HIPCHK(hipMemcpyAsync(&err, ctx->d_upload_err, 4, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (err) return (int)err;
    // ---- every old piece where it is, the new ones behind them
    scene::Layout L;
    for (uint32_t c = 0; c < nc; ++c)
    {
        for (uint32_t p = ctx->scene_off[c]; p < ctx->scene_off[c + 1]; ++p) L.push_old(ctx, p);
        L.table.push_back((uint32_t)L.src.size());
    }
    for (uint32_t b = 0; b < n_bodies; ++b)
    {
        for (uint32_t k = body_piece_off[b]; k < body_piece_off[b + 1]; ++k)
        {
            L.push_other(k, 0, mvo[k], mvo[k + 1] - mvo[k], ho[0][k], ho[0][k + 1] - ho[0][k]);
            L.push_other(k, 1, cvo[k], cvo[k + 1] - cvo[k], ho[1][k], ho[1][k + 1] - ho[1][k]);
        }
        L.table.push_back((uint32_t)L.src.size());
    }
    // the pose table is made only when a pose arrives that is not bit for bit the identity
    std::vector<float> pose = ctx->scene_pose;
    bool moved = false;
    for (uint32_t b = 0; world && b < n_bodies; ++b) moved = moved || memcmp(world + 16 * (size_t)b, scene::IDENTITY, 64) != 0;
    if (pose.empty() && moved) for (uint32_t c = 0; c < nc; ++c) pose.insert(pose.end(), scene::IDENTITY, scene::IDENTITY + 16);
    if (!pose.empty())
        for (uint32_t b = 0; b < n_bodies; ++b) { const float* W = world ? world + 16 * (size_t)b : scene::IDENTITY; pose.insert(pose.end(), W, W + 16); }
    const uint32_t n = (uint32_t)L.src.size();
    const bool had_event = ctx->have_event;
    const int rc = scene::regather(ctx, L, staged, std::move(pose), nullptr);
    if (rc) return rc;
    if (first_new_compound) *first_new_compound = nc;
    return finish_edit(ctx, n, had_event);
}

int surtr_scene_cull(surtr_ctx* ctx, int set, float density, float min_mass, const float* keep_box, int apply, uint32_t* n_compounds, uint8_t* reason,
                     uint32_t* n_removed)
{
    if (!ctx || !n_compounds || (set != 0 && set != 1)) return SURTR_E_INVALID;
    if (!ctx->n_pieces || ctx->scene_off.size() < 2) return SURTR_E_STATE;
    for (int k = 0; keep_box && k < 6; ++k) if (keep_box[k] != keep_box[k]) return SURTR_E_INVALID;
    const uint32_t nc = (uint32_t)ctx->scene_off.size() - 1u;
    if (reason && *n_compounds < nc) { *n_compounds = nc; return SURTR_E_CAPACITY; }
    *n_compounds = nc;
    if (n_removed) *n_removed = 0;
    if (!reason) return SURTR_OK;
    (void)hipSetDevice(ctx->device);
    // mass records | bounds | reason bytes, in one buffer of the context
    const size_t at_box = (size_t)nc * sizeof(surtr_mass), at_reason = at_box + (size_t)nc * sizeof(surtr_bounds);
    int rc = ctx->d_cull.grow(ctx, at_reason + nc, at_reason + nc + (at_reason + nc) / 4);
    if (rc) return rc;
    char* d = ctx->d_cull.p;
    if ((rc = surtr_scene_mass_dev(ctx, set, density, d, at_box)) != SURTR_OK) return rc;
    if ((rc = surtr_scene_bounds_dev(ctx, 1, d + at_box, (size_t)nc * sizeof(surtr_bounds), nullptr, 0)) != SURTR_OK) return rc;
    CullBox keep;
    memset(&keep, 0, sizeof(keep));
    if (keep_box) { for (int k = 0; k < 3; ++k) { keep.lo[k] = keep_box[k]; keep.hi[k] = keep_box[3 + k]; } keep.on = 1u; }
    hipStream_t st = ctx->stream;
    hipLaunchKernelGGL(k_cull_mark, dim3((nc + 255) / 256), dim3(256), 0, st, nc, (const surtr_mass*)d, (const surtr_bounds*)(d + at_box), min_mass, keep,
                       (uint8_t*)(d + at_reason));
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(reason, d + at_reason, nc, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (!apply) return SURTR_OK;
    std::vector<uint32_t> marked;
    for (uint32_t c = 0; c < nc; ++c) if (reason[c]) marked.push_back(c);
    if (marked.empty()) return SURTR_OK;
    if (marked.size() == nc) return SURTR_E_INVALID;      // (nothing is removed; the reasons say why)
    rc = surtr_scene_remove(ctx, (uint32_t)marked.size(), marked.data(), nullptr, nullptr);
    if (rc == SURTR_OK && n_removed) *n_removed = (uint32_t)marked.size();
    return rc;
}

} // extern "C"
