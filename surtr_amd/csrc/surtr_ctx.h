// surtr_ctx.h -- records shared by the translation units of libsurtr_hip.so: what the kernels of one event leave in HBM
// (PairRec, FragRec, Arena), the resident pieces, the scratch pools, and the host-side context behind the C ABI.
#pragma once
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../include/surtr_hip.h"
#include "clip_core.h"

using namespace surtr;

// ------------------------------------------------------------------ records
struct PairRec
{
    uint32_t cv_off, cv_n, ch_off, ch_n;   // clipped Convex in the arena
    uint32_t mv_off, mv_n, mh_off, mh_n;   // clipped Mesh (all islands, island-major)
    uint32_t ni, isl_off;                  // islands and where their (nv, nh) records start
    uint32_t status;
    // reduced Mesh left in HBM by k_prep_pairs: img_fmt = IMG_*, offset in 16-byte units, vertices, ring entries,
    // position slots reserved (>= the capacity of the topology that will clip it: positions are then used in place)
    uint32_t img_fmt, img_off, img_n, img_h, img_pc;
    // 1: the clip of the Convex ended in an inconsistent solid (degenerate input, where the reference produces an invalid
    // polyhedron and carries on).  The pair goes on like the reference's: if nothing is left of the Mesh it yields no fragment
    // and the event is fine; a fragment that would carry the invalid Convex fails the event with SURTR_E_TOPOLOGY.
    uint32_t cv_bad;
};

enum { IMG_NONE = 0,      // no image: k_clip_pairs runs the pre-pass itself
       IMG_NARROW = 1,    // 16-bit image, loads straight into the LDS topology
       IMG_WIDE = 2,      // the reduced solid does not fit the LDS topology: k_clip_pairs goes to global scratch directly
       IMG_EMPTY = 3,     // nothing of the Mesh is left
       IMG_REC = 4 };     // the band as sorted 16-byte records + positions (prep_sorted.h): the record clipper streams it as it is

// Byte offsets of the sections of one image (all 16-byte aligned): hist/zhist/nzero (F words each), the keep mask
// (one word per 64 input vertices), then the reduced solid in the LDS layout, then its positions.
struct ImgLayout { uint32_t hist, zhist, nzero, mask, loff, llen, comp, ring, pos, total; };
__host__ __device__ static inline ImgLayout img_layout(uint32_t F, uint32_t nbV, uint32_t n, uint32_t hsum, uint32_t posCap = 0)
{
    auto up = [](uint32_t b) { return (b + 15u) & ~15u; };
    ImgLayout L;
    L.hist = 0; L.zhist = up(4u * F); L.nzero = L.zhist + up(4u * F); L.mask = L.nzero + up(4u * F); L.loff = L.mask + up(8u * nbV);
    L.llen = L.loff + up(2u * n); L.comp = L.llen + up(n); L.ring = L.comp + up(n); L.pos = L.ring + up(2u * hsum);
    L.total = L.pos + up(12u * (n > posCap ? n : posCap));      // positions last: room for the cut points of the clip
    return L;
}

struct ImgArena { char* base; uint32_t cap16; };      // capacity in 16-byte units; cursor = Arena::cursors[CUR_IMG]

// Per-workgroup scratch of k_prep_pairs: work lists of the pre-pass and (for very large solids) its masks.
struct PrepPool { char* base; size_t per_wg; uint32_t VMAX; };
static size_t prep_bytes_per_wg(uint32_t VMAX)
{
    auto r = [](size_t b) { return (b + 255) & ~(size_t)255; };
    return 2 * r((size_t)VMAX * 4) + r((size_t)(VMAX / SURTR_SB + 2) * 4) + 2 * r((size_t)(VMAX / SURTR_LANES + 2) * 8) +
           2 * r((size_t)VMAX + 64) +     // + first clipping planes of the undecided groups' vertices / by band index (prep_sorted.h)
           2 * r((size_t)VMAX * 4) +      // + kept list, face-walk list
           r((size_t)VMAX * 2 + 64);      // + sorted id by band index (record emit)
}

struct FragRec
{
    int32_t cell, piece, island;
    uint32_t mv_off, mv_n, mh_off, mh_n;
    uint32_t cv_off, cv_n, ch_off, ch_n;
    uint32_t idx_off, idx_n;
    // output bases (filled by k_out_scan)
    uint32_t o_mv, o_mh, o_cv, o_ch, o_idx;
};

struct Arena
{
    float* pos; uint32_t* loff; uint32_t* llen; int32_t* nbr; uint32_t* idx;
    uint2* isl;
    uint32_t capV, capH, capI, capIsl;
    uint32_t* cursors;   // the event's device counters: CUR_COUNT words, slot map below
};

// The slot map of Arena::cursors: every word the kernels of an event coordinate through.  k_event_init clears all of them at the
// start of an event ("cleared" below names only what clears a slot besides that).  surtr_queue_stats copies the first
// CUR_STATS_WORDS out, and include/surtr_hip.h publishes some of them by number: those are pinned under the enumeration.
enum : uint32_t
{
    // arena cursors (every kernel that parks a solid adds what it takes; k_out_scan and surtr_queue_stats read them)
    CUR_V = 0,              // vertices.  W: arena_take, sc_park, wc_park.  surtr_load_fragments sets it
    CUR_H = 1,              // ring entries.  W: the same
    CUR_I = 2,              // triangle indices.  W: k_faces; R: k_out_scan.  Cleared by launch_faces
    CUR_ISL = 3,            // island records.  W: arena_take, wc_park
    // work-queue tickets (atomicAdd by lane 0 of a workgroup: the value is the ticket)
    CUR_Q_CLIP = 4,         // k_clip_pairs / _wave / _main over the clip table's regular classes
    CUR_STATUS = 5,         // W: atomicMax of the event's SURTR_E_* by any kernel; R: k_out_scan -> surtr_counts::status
    CUR_Q_REFIT = 6,        // k_refit / k_refit_n over the fragment table.  Cleared by surtr_event_refit
    CUR_Q_FACES = 7,        // k_faces (first tier) over the fragment table.  Cleared by launch_faces
    CUR_Q_CONVEX = 8,       // k_clip_convex over the pairs
    CUR_Q_PREP = 9,         // k_prep_pairs* over the pre-pass table (or the pairs themselves: front_par)
    CUR_IMG = 10,           // image arena, 16-byte units.  W: k_prep_pairs*
    CUR_Q_BIG = 11,         // k_clip_pairs_big / _wave_big over clip classes 15..14
    CUR_Q_HALF = 12,        // k_clip_pairs_half over half classes 6..1
    CUR_Q_RETRY = 13,       // the retry launch of k_clip_pairs over the half table's retry list
    CUR_FLAGGED_FRAGS = 14, // W: k_refit*, k_faces; R: k_out_scan (n_failed = 14 + 15).  Cleared by launch_faces unless a refit flagged
    CUR_FLAGGED_PAIRS = 15, // W: pair_failed; R: k_out_scan
    // per-class counts, 16 classes each (a ticket walks them from the heaviest class down)
    CUR_CLS_CLIP = 16,      // base.  W: k_prep_pairs* (enqueue); R: every Mesh clip kernel's take_pair
    CUR_CLS_FRAG = 32,      // base.  W: k_frag_table, surtr_load_fragments; R: frag_of_ticket (k_refit*, k_faces)
    CUR_CLS_PREP = 48,      // base.  W: k_clip_convex; R: k_prep_pairs*
    CUR_CLS_HALF = 64,      // base.  W: k_prep_pairs* (enqueue_half); R: k_clip_pairs_half
    CUR_RETRY_N = CUR_CLS_HALF,   // the half table's class 0 = retry list.  W: clip_pair_general<HALF>; R: the retry launch
    // diagnostics of the Convex chain (W: convex_chain via ChainCaller; R: surtr_queue_stats)
    CUR_CVX_RESUMED = 78,   // k_clip_convex: general clips resumed from a later plane
    CUR_REFIT_RESUMED = 79, // k_refit*: the same
    CUR_CVX_TOOK = 80,      // k_clip_convex: Convexes small_clip took; + 1 (81): handed on, or started on the literal clipper
    CUR_REFIT_TOOK = 82,    // k_refit*: the same; + 1 (83): handed on
    CUR_BIG_QUOTA = 84,     // W/R: k_prep_pairs*, large bands admitted to k_clip_pairs_big so far
    CUR_FACES2_N = 85,      // second-tier faces list, fragments pushed.  W: k_faces first tier; R: second tier.  Cleared by launch_faces
    CUR_Q_FACES2 = 86,      // ... its ticket (directly behind CUR_FACES2_N: launch_faces clears both with one fill)
    CUR_CVX_GAVE_UP = 87,   // give-up list of k_clip_convex_lean, pairs pushed.  W: the lean kernel; R: k_clip_convex as its second tier
    // diagnostics (W: as said; R: surtr_queue_stats)
    CUR_REC_TOOK = 88,      // clip_pairs_wave_body: pairs the record clipper finished
    CUR_REC_HANDED = 89,    // ... handed on to the general clipper
    CUR_LIT_TOO_LARGE = 90, // literal_run: solids too large for the literal clipper
    CUR_REC_IMAGES = 91,    // k_prep_pairs*: bands left as record images
    CUR_SORTED_SEL = 92,    // k_prep_pairs*: pairs that took the sorted selection
    CUR_REC_SPENT = 93,     // clip_pairs_wave_body: record images given up on (redone from the piece)
    CUR_CATCH_CLIPPED = 94, // k_clip_pairs_catch: pairs it clipped
    CUR_UNREFITTED = 95,    // k_refit_n: fragments left un-refitted and flagged SURTR_E_CAPACITY
    CUR_WC_WHY = 96,        // base of the record clipper's why[site] block (wave_clip.h: WC_WHY_WORDS words)
    CUR_Q_CONVEX2 = 125,    // ticket of k_clip_convex as second tier, over the give-up list
    CUR_STATS_WORDS = 128,  // what surtr_queue_stats copies out (and surtr_load_fragments writes)
    // hand-over from k_clip_pairs_main to k_clip_pairs_catch (surtr_handover_stats copies the CUR_HO_WORDS words out)
    CUR_HO_PUSHED = 146,    // W: main, one per pair pushed to hlist; R: polling catcher, sweep
    CUR_HO_STARTED = 147,   // W: main, one per workgroup on entry; R: polling catcher ("is it running beside me")
    CUR_HO_SIGNED_OFF = 148,// W: main, one per workgroup after its last hand-over; R: polling catcher
    CUR_HO_POLL_SLOT = 149, // W/R: catcher, hlist slot each polling workgroup waits on
    CUR_Q_CATCH = 150,      // ticket of the catcher's own classes (clip classes 13..12)
    CUR_Q_SWEEP = 151,      // ticket of the sweep launch over the pushed slots
    CUR_HO_WORDS = 6,
    CUR_COUNT = 256
};
static_assert(CUR_V == 0 && CUR_H == 1 && CUR_I == 2 && CUR_ISL == 3 && CUR_STATUS == 5 && CUR_CLS_CLIP == 16 && CUR_CLS_FRAG == 32 &&
              CUR_CLS_PREP == 48 && CUR_CLS_HALF == 64 && CUR_REC_TOOK == 88 && CUR_REC_HANDED == 89 && CUR_LIT_TOO_LARGE == 90 &&
              CUR_UNREFITTED == 95 && CUR_WC_WHY == 96, "include/surtr_hip.h publishes these slots of surtr_queue_stats by number");
static_assert(CUR_STATS_WORDS <= CUR_COUNT && CUR_Q_SWEEP + 1 == CUR_HO_PUSHED + CUR_HO_WORDS && CUR_HO_PUSHED + CUR_HO_WORDS <= CUR_COUNT &&
              CUR_Q_FACES2 == CUR_FACES2_N + 1, "slot map");

struct alignas(16) SRow { uint32_t w[4]; };

struct Pieces
{
    const float* mpos; const uint32_t* mloff; const uint32_t* mllen; const int32_t* mnbr; const uint32_t* mvo; const uint8_t* mtri; const float* mrad;
    const uint32_t* mperm; const float4* mposr_s; const float4* mbsph; const uint32_t* mbo;
    const float* cpos; const uint32_t* cloff; const uint32_t* cllen; const int32_t* cnbr; const uint32_t* cvo; const uint8_t* ctri; const float* crad;
    const uint32_t* cperm; const float4* cposr_s; const float4* cbsph; const uint32_t* cbo;
    uint32_t n;
    // per piece: 1 = some ring of the solid lists a neighbour twice (a sliver with coincident vertices).  Face walks on such a
    // solid need not close, and where the reference's bounded walk stops then depends on its vertex count of the moment: these
    // solids take the literal clipper (literal_clip.h) from the start.
    const uint8_t* mdup; const uint8_t* cdup;
    // the Mesh rings once more in SORTED space (round 4, pieces_dev.hip): sorted slot i (global over the set) has the 16-byte row
    // mrow_s[i] = eight 16-bit words: header (ring length 0..7 | 0x80: some incident face is no triangle | 0x40: more than seven
    // neighbours, not listed), then the neighbours as piece-local SORTED indices (pieces of up to 65 535 vertices; 0xFFFF: none).
    // One aligned load gives the pre-pass of k_prep_pairs a vertex's whole ring; it looks the first clipping plane of a
    // neighbour up by that index.  miperm: sorted index of every vertex.
    // mbsph2 / mbsph3: one sphere per 8 / 64 of the SURTR_SB-vertex spheres (mbo2 / mbo3: first such sphere of every piece)
    const SRow* mrow_s; const uint32_t* miperm;
    const float4* mbsph2; const uint32_t* mbo2; const float4* mbsph3; const uint32_t* mbo3;
};

struct ScratchPool
{
    char* base; size_t per_wg;
    uint32_t CV, CH, VMAX;
};

// Per-workgroup global scratch: positions of the reduced solid (both variants), the wide (32-bit)
// topology used when a solid does not fit the LDS one, three u32 work arrays, scan blocks, pre-pass masks.
struct Scratch
{
    float* pos;
    uint32_t* g_loff; uint32_t* g_llen; int8_t* g_comp; uint32_t* g_ring;
    uint32_t* g_succ; uint32_t* g_pred; uint32_t* g_pcnt;
    uint32_t* aux0; uint32_t* aux1; uint32_t* aux2; uint32_t* aux3;
    int8_t* g_gcomp;       // explicit classification of a plane some live vertex lies in (both variants)
    uint2* blk;
    unsigned long long* gmask; uint2* gblk;
    float* t_pos; uint32_t* t_loff; uint32_t* t_llen; int8_t* t_comp; uint32_t* t_ring;   // squeeze() staging
    uint32_t CV, CH;
};

__device__ static Scratch carve(const ScratchPool& P, uint32_t wg)
{
    Scratch S;
    char* p = P.base + (size_t)wg * P.per_wg;
    auto take = [&](size_t bytes) { char* r = p; p += (bytes + 255) & ~(size_t)255; return r; };
    S.pos = (float*)take((size_t)P.CV * 12);
    S.g_loff = (uint32_t*)take((size_t)P.CV * 4);
    S.g_llen = (uint32_t*)take((size_t)P.CV * 4);
    S.g_comp = (int8_t*)take((size_t)P.CV);
    S.g_ring = (uint32_t*)take((size_t)P.CH * 4);
    S.g_succ = (uint32_t*)take((size_t)P.CV * 4);
    S.g_pred = (uint32_t*)take((size_t)P.CV * 4);
    S.g_pcnt = (uint32_t*)take((size_t)P.CV * 4);
    // (aux0 and aux2 are also the pre-pass's work lists -- prepass_select's needy, up to one entry per vertex of the INPUT, and und,
    //  one per SURTR_SB of them -- filled before anything is known to fit: they have room for the largest piece even where
    //  surtr_set_scratch makes CV smaller.  Sized by CV alone, a longer needy list ran on into aux1 .. aux3 of the same slice, where
    //  nothing shows it, then into und, which the same loop reads, and the masks.  und gets VMAX entries too: more than it needs.)
    const size_t AV = P.CV > P.VMAX ? P.CV : P.VMAX;
    S.aux0 = (uint32_t*)take(AV * 4);
    S.aux1 = (uint32_t*)take((size_t)P.CV * 4);
    S.aux2 = (uint32_t*)take(AV * 4);
    S.aux3 = (uint32_t*)take((size_t)P.CV * 4);
    S.g_gcomp = (int8_t*)take((size_t)P.CV);
    S.blk = (uint2*)take((size_t)(P.CV / SURTR_LANES + 4) * 8);
    S.gmask = (unsigned long long*)take((size_t)(P.VMAX / SURTR_LANES + 2) * 8);
    S.gblk = (uint2*)take((size_t)(P.VMAX / SURTR_LANES + 2) * 8);
    S.t_pos = (float*)take((size_t)P.CV * 12); S.t_loff = (uint32_t*)take((size_t)P.CV * 4); S.t_llen = (uint32_t*)take((size_t)P.CV * 4);
    S.t_comp = (int8_t*)take((size_t)P.CV); S.t_ring = (uint32_t*)take((size_t)P.CH * 4);
    S.CV = P.CV; S.CH = P.CH;
    return S;
}

static size_t scratch_bytes_per_wg(uint32_t CV, uint32_t CH, uint32_t VMAX)
{
    auto r = [](size_t b) { return (b + 255) & ~(size_t)255; };
    return 2 * r((size_t)CV * 12) + 9 * r((size_t)CV * 4) + 2 * r((size_t)std::max(CV, VMAX) * 4) + 3 * r((size_t)CV) + 2 * r((size_t)CH * 4) + r((size_t)(CV / SURTR_LANES + 4) * 8) +
           2 * r((size_t)(VMAX / SURTR_LANES + 2) * 8);
}

struct FaceScratch
{
    int32_t* base; size_t per_wg; uint32_t HF;   // HF = max half-edges of one fragment
};

struct surtr_ctx;

// Device memory owned by the context or by one call: grow-only, move-only, freed when destroyed.  grow() frees the old
// block before it allocates the new one (the peak is the larger of the two, not their sum) and records the capacity only
// once the allocation has succeeded: after a failure the buffer is empty and ctx->err says why.
template <class T>
struct DevBuf
{
    T* p = nullptr;
    size_t cap = 0;      // elements of T
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; } return *this; }
    ~DevBuf() { reset(); }
    void reset() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    operator T*() const { return p; }
    // at least `need` elements; a smaller buffer is replaced by one of `alloc` (>= need; 0: need) elements
    int grow(surtr_ctx* ctx, size_t need, size_t alloc = 0);
};

// One set of resident solids (all Mesh solids, or all Convex solids, of the pieces) in a grow-only pool.
struct PieceSet
{
    DevBuf<float> pos; DevBuf<uint32_t> loff, llen; DevBuf<int32_t> nbr; DevBuf<uint32_t> vo; DevBuf<uint8_t> tri; DevBuf<float> rad;
    DevBuf<uint32_t> perm; DevBuf<float4> posr_s, bsph; DevBuf<uint32_t> bo;
    DevBuf<float> box; DevBuf<unsigned long long> key, key2; DevBuf<uint32_t> val;    // Morton sort
    DevBuf<uint8_t> dup;       // per piece: a ring lists a neighbour twice
    // rings in sorted space + two coarser sphere levels (see Pieces)
    DevBuf<uint32_t> iperm; DevBuf<SRow> row_s;
    DevBuf<float4> bsph2; DevBuf<uint32_t> bo2; DevBuf<float4> bsph3; DevBuf<uint32_t> bo3;
};

// Device buffers of surtr_build_cells (cells_dev.hip): seeds, per-cell slots, and the compact cell arrays.
struct CellBuffers
{
    DevBuf<double> seeds; DevBuf<uint32_t> goff; DevBuf<char> slots; DevBuf<uint32_t> cfo, cvo;
    DevBuf<int32_t> gen; DevBuf<uint32_t> fvo; DevBuf<double> verts; DevBuf<uint32_t> heads;
    uint32_t n = 0, nf = 0, nfv = 0;
};

// Half-size LDS topology of k_clip_pairs_half (capacities; the kernel is in surtr_hip.hip).
#define SURTR_LVS (SURTR_LV / 2u)
#define SURTR_LHS ((SURTR_LH * 11u / 24u) & ~7u)
// It takes solids of up to half its capacity: thin bands can double under the cuts (measured on BASELINE configs[3]: a
// fifth of the pairs admitted with 20 % room outgrew it), and a retry costs the pair twice.
#ifndef SURTR_HALF_ROOM
#define SURTR_HALF_ROOM 2u       // (tests build with 1 to make pairs outgrow it)
#endif
__host__ __device__ static inline bool fits_half(uint32_t n, uint32_t h, uint32_t capVs) { return SURTR_HALF_ROOM * n <= capVs && SURTR_HALF_ROOM * h <= SURTR_LHS; }
static inline bool surtr_fits_half(uint32_t n, uint32_t h) { return fits_half(n, h, SURTR_LVS); }

struct surtr_ctx
{
    int device = 0;
    bool frags_of_pieces = false;      // the current fragments are an event's over the resident pieces (k_refit may look at the piece a Convex came from)
    // what the CUs can hold (surtr_create); max_wg* below are those, cut down to what the scratch of the current pieces leaves room for
    uint32_t hw_wg = 512, hw_wg_faces = 1024, hw_wg_prep = 1792, hw_wg_big = 48, budget_vmax = 0xFFFFFFFFu, budget_hmax = 0xFFFFFFFFu;
    uint32_t max_wg = 512, max_wg_faces = 1024, max_wg_small = 2048, max_wg_lean = 3072, max_wg_prep = 1792, max_wg_half = 1024;
    DevBuf<uint32_t> d_hlist;                               // hand-over list of the split arrangement (k_clip_pairs_main -> k_clip_pairs_catch)
    uint32_t vmin = 0;                                      // smallest Mesh of the resident pieces
    ScratchPool pool_half{}; uint32_t n_wg_half = 0; DevBuf<char> pool_half_buf;     // k_clip_pairs_half: scratch for the half-size LDS topology only
    // Light pairs go to k_clip_pairs_half only when they are most of the event (small pieces: refracture).  Beside a
    // full k_clip_pairs a third kernel costs more than it gains (configs[3]: +0.2 ms even when its workgroups exit at
    // once), and what a large piece leaves of itself in a cell is seldom small enough.  Decided per upload from the piece sizes.
    bool half_on = false;
    PrepPool prep{nullptr, 0, 0}; uint32_t n_wg_prep = 0; DevBuf<char> prep_buf;
    ImgArena img{nullptr, 0}; DevBuf<char> img_buf;
    DevBuf<uint32_t> d_order;        // 64 x the pairs it has room for: class tables of 16 each (clip order, pre-pass order, half clip order, spare)
    DevBuf<uint32_t> d_forder;       // fragments by size class, 16 x cap_frags
    bool wave_big = false;           // the large bands through k_clip_pairs_wave_big (one workgroup per CU) instead of k_clip_pairs_big
    uint32_t n_wg_big = 48;          // workgroups of k_clip_pairs_big
    hipStream_t stream2 = nullptr;   // k_clip_pairs runs here, beside k_clip_pairs_big on the caller's stream
    hipStream_t stream3 = nullptr;   // k_clip_pairs_half (+ the retry launch) beside both
    hipEvent_t ev_prep = nullptr, ev_big = nullptr, ev_half = nullptr, ev_cvx = nullptr;
    uint32_t events_in_flight = 1;      // surtr_set_events_in_flight: contexts the host keeps busy on this GPU at once
    hipStream_t stream = nullptr;
    std::string err;
    // pieces
    uint32_t n_pieces = 0, vmax = 0, hmax = 0, cvmax = 0, chmax = 0;
    CellBuffers cells;               // surtr_build_cells
    PieceSet mset, cset;             // the resident pieces: Mesh and Convex solids + what the pre-pass derives from them (pieces_dev.hip)
    DevBuf<uint32_t> d_upload_err;
    DevBuf<float> d_group_xf;        // surtr_place_cells_in_pieces: per-group scale / shift
    DevBuf<float> d_world;           // surtr_transform_pieces: the world matrices
    DevBuf<char> sort_tmp;           // radix-sort scratch of the Morton sort
    DevBuf<uint32_t> d_from;         // surtr_pieces_from_event: fragment list and offsets
    DevBuf<uint32_t> d_qstatus; uint32_t qstatus_n = 0;   // query_dev.hip: per-piece status of the last ray cast / overlap
    float upload_ms = 0.f; uint32_t upload_allocs = 0;   // surtr_upload_stats
    // the scene (scene_dev.hip): compound c owns resident pieces [scene_off[c], scene_off[c + 1]); every call that replaces the
    // pieces leaves one compound holding all of them (set_piece_stats)
    std::vector<uint32_t> scene_off;
    std::vector<uint32_t> h_vo[2], h_ho[2];              // vertex / ring-entry offsets of the resident pieces (0 = Mesh, 1 = Convex), host copies
    // the compounds the last event ran over, strictly descending (surtr_scene_fracture_event: one; surtr_scene_fracture_bodies: the
    // click's targets); empty: none, or committed
    std::vector<uint32_t> scene_event_compound;
    // after surtr_scene_fracture_impacts: scene_event_compound holds the targets impact after impact (descending inside an impact
    // only), and impact i owns entries [scene_event_impacts[i], scene_event_impacts[i + 1]); empty after any other event
    std::vector<uint32_t> scene_event_impacts;
    DevBuf<uint32_t> d_outside_list;                     // surtr_scene_outside(_dev): the pieces it was asked about
    std::vector<uint32_t> h_outside_stage;               // surtr_scene_outside_impacts(_dev): list, impact of every piece, sphere table
    // per-body poses (surtr_scene_set_poses): 16 floats per compound, x' = A x + b as surtr_transform_pieces takes them; empty: every
    // pose is the identity.  The device copy (scene_sync_device below) is made by the first query after the poses or the table change.
    std::vector<float> scene_pose;
    bool scene_dev_stale = true;
    std::vector<double> h_pose_stage; std::vector<uint32_t> h_comp_stage;      // what the last upload was made from
    DevBuf<double> d_pose;               // per compound: A^T row-major (9), b (3)
    DevBuf<uint32_t> d_piece_comp;       // per resident piece: its compound; then the compound table (n_compounds + 1 offsets)
    struct { DevBuf<float> pos; DevBuf<uint32_t> loff; DevBuf<int32_t> nbr; DevBuf<uint32_t> vo; } spare[2];   // surtr_scene_commit gathers into these, then swaps
    DevBuf<int32_t> d_commit_src; DevBuf<uint32_t> d_commit_tab;      // its gather tables
    // scene upkeep (upkeep_dev.hip).  The float poses as surtr_scene_bounds reads them, 16 floats per compound, brought up to date
    // after scene_sync_device has refreshed the tables (which raises scene_posef_stale); empty scene_pose: no copy, every pose the identity
    DevBuf<float> d_posef; bool scene_posef_stale = true; std::vector<float> h_posef_stage;
    DevBuf<surtr_bounds> d_bounds_piece;                 // surtr_scene_bounds_dev without a piece buffer of the caller's: the per-piece records
    DevBuf<char> d_cull;                                 // surtr_scene_cull: mass records, bounds and reason bytes of every compound
    // surtr_scene_contacts(_dev) (contact_dev.hip): the body records its broad phase reads (the piece records go to d_bounds_piece), and
    // -- only under surtr_set_profiling -- the five events between its phases (made on first use, destroyed with the context)
    DevBuf<surtr_bounds> d_bounds_body;
    struct ContactEvents { hipEvent_t e[5] = {}; bool valid = false; ~ContactEvents() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); } } contact_ev;
    // surtr_scene_append: the new pieces as the host gave them (offsets from 0 per set), vetted here by k_piece_check before the scene is touched
    struct { DevBuf<float> pos; DevBuf<uint32_t> loff, llen, vo; DevBuf<int32_t> nbr; DevBuf<uint8_t> dup; } stage[2];
    // surtr_scene_fragments: the tables it lays out on the host (fragment records, cursors, counts, size-class slots, chunk table), kept
    // between calls so that the _async form leaves nothing behind that goes out of scope; the device copy of the last two
    std::vector<uint32_t> h_frag_stage; DevBuf<uint32_t> d_frag_tab;
    float commit_ms[2] = {0.f, 0.f};                     // host time of the last commit up to the end of the gather / from there to its end (surtr_scene_commit_times)
    uint32_t regroup_rounds = 0;                         // label rounds of the last surtr_event_regroup (one launch)
    uint64_t tot_mv = 0, tot_mh = 0;
    // cells
    uint32_t n_cells = 0, n_faces = 0;
    DevBuf<uint32_t> d_cvx_giveup;      // k_clip_convex_lean: the pairs it left to k_clip_convex (one word per pair of the event)
    DevBuf<uint32_t> d_pair_order; uint32_t pair_order_begin = 0, pair_order_count = 0;   // k_clip_convex: pairs by plane count
    bool pair_order_is_list = false;
    DevBuf<float> d_v012; DevBuf<float4> d_planes; DevBuf<uint32_t> d_plane_off;
    std::vector<uint32_t> h_plane_off;
    bool planes_ready = false;
    // surtr_place_cells_impacts: n_impacts_placed instances of the pattern, instance i's cell c at i * n_cells + c, in tables of their
    // own (the plain placement keeps d_planes); 0: none, or the pattern has been replaced since
    uint32_t n_impacts_placed = 0;
    DevBuf<float4> d_planes_imp; DevBuf<uint32_t> d_plane_off_imp; DevBuf<float> d_imp_xf;
    std::vector<uint32_t> h_plane_off_imp; std::vector<float> h_imp_xf;
    // ... or surtr_place_cells_patterns (imp_library): instance i is a stored pattern of its own, in the same tables.  After either
    // placement instance i owns global cells [imp_cell_base[i], imp_cell_base[i + 1]) and the tables hold imp_faces planes.
    bool imp_library = false; std::vector<uint32_t> imp_cell_base; uint32_t imp_faces = 0;
    DevBuf<uint32_t> d_imp_tab; std::vector<uint32_t> h_imp_tab;      // k_place_cells_patterns: face prefix [n + 1], library face base [n]
    // the pattern library (surtr_pattern_store): v012 and face offsets (each pattern's from 0) of every stored pattern, one after the
    // other in two grow-only buffers; lib[k]: where pattern k lies.  h_lib_off: the offsets once more, for the host's plane counts.
    struct LibPattern { uint32_t n_cells, n_faces, face_base, off_base; };
    std::vector<LibPattern> lib;
    DevBuf<uint32_t> d_lib_v012 /* floats, kept as words */, d_lib_off; std::vector<uint32_t> h_lib_off;
    uint32_t lib_faces = 0;      // faces stored so far (h_lib_off.size(): offset words)
    // scratch + arena
    uint32_t user_cv = 0, user_ch = 0;
    uint64_t user_av = 0, user_ah = 0, user_ai = 0;
    // (the kernels' views -- pool, fs, arena, ... -- and the sizes beside them describe what their buffers hold: ensure_scratch and
    //  ensure_arena set them once every buffer of the group exists, and clear them when they free the group)
    ScratchPool pool{}; uint32_t n_wg = 0; DevBuf<char> pool_buf;
    ScratchPool pool_small{}; uint32_t n_wg_small = 0; DevBuf<char> pool_small_buf;      // one-wave kernels (Convex clip, refit)
    FaceScratch fs{}; DevBuf<int32_t> fs_buf; DevBuf<uint2> d_blk; uint32_t blk_per_wg = 0, n_wg_faces_alloc = 0;
    // second tier of k_faces scratch (pieces of more than SURTR_FACES_TIER half-edges): a few workgroups with room for a fragment
    // as large as the largest piece; the first launch hands them the fragments that do not fit its own (d_face_list)
    FaceScratch fs_big{}; DevBuf<int32_t> fs_big_buf; DevBuf<uint2> d_blk_big; uint32_t blk_per_wg_big = 0, n_wg_faces_big = 0;
    DevBuf<uint32_t> d_face_list;
    Arena arena{};
    struct { DevBuf<float> pos; DevBuf<uint32_t> loff, llen, idx, cursors; DevBuf<int32_t> nbr; DevBuf<uint2> isl; } arena_buf;
    DevBuf<PairRec> d_pairs;
    DevBuf<FragRec> d_frags; uint32_t cap_frags = 0;
    DevBuf<uint32_t> d_frag_status;      // per fragment: SURTR_OK or why it has no triangles (u32[cap_frags])
    DevBuf<uint2> d_scanblk;
    DevBuf<surtr_counts> d_counts;
    DevBuf<uint32_t> d_face_group;       // surtr_place_cells_groups: group of every pattern face
    DevBuf<uint8_t> d_outside;
    std::vector<uint8_t> last_outside;       // the `outside` mask of the last event (empty: none), for surtr_event_regroup
    DevBuf<uint2> d_pair_list;
    uint32_t refit_limit = 4;            // FractureArgs::RefittingPointLimit (surtr_set_refit_point_limit): above 4, k_refit_n refits
    DevBuf<uint32_t> d_hull_ws;          // k_refit_n: gain and "processed" mark of every arena vertex (2 x capV words)
    uint32_t shade_lds_limit = 0;        // surtr_set_shade_tier: half-edges of a fragment k_sh_faces keeps in LDS (0: SURTR_SHADE_LH)
    float color[3] = {0.25f, 0.25f, 0.25f};      // VertexNormalColor::Color written by k_pack (Inc/Poly.h:68 default)
    surtr_counts last{}; bool last_current = false;     // `last` holds the counts of the event in the arena
    bool have_event = false; uint32_t last_flags = 0;
    // fragments and pairs of the last event over these pieces whose counts were read back (0: none yet), see plan_event
    uint32_t frag_hint = 0, frag_hint_pairs = 0, event_pairs = 0;
    // staging for downloads
    DevBuf<char> d_blob;
    // per-kernel timing with HIP events on the work stream (surtr_set_profiling)
    bool profiling = false;
    // history of the Mesh clip kernel (slot 0: k_clip_pairs, slot 11: k_clip_pairs_wave) over the last events, read without a
    // synchronisation in between (surtr_kernel_history): what a caller with several events in flight averages over
    hipEvent_t hev[16][2] = {}; uint32_t hcount = 0; int hslot[16] = {};
    hipEvent_t ev[32] = {};     // begin/end per kernel slot 0..15
    bool ev_valid[16] = {};
};

#define PROF_BEGIN_ON(i, strm) do { if (ctx->profiling) { (void)hipEventRecord(ctx->ev[2 * (i)], strm); } } while (0)
#define PROF_END_ON(i, strm) do { if (ctx->profiling) { (void)hipEventRecord(ctx->ev[2 * (i) + 1], strm); ctx->ev_valid[i] = true; } } while (0)
// the same into the history ring (only where a kernel was really launched)
#define PROF_HIST_BEGIN(i, strm) do { if (ctx->profiling && ctx->hev[0][0]) { (void)hipEventRecord(ctx->hev[ctx->hcount % 16u][0], strm); } } while (0)
#define PROF_HIST_END(i, strm) do { if (ctx->profiling && ctx->hev[0][0]) { (void)hipEventRecord(ctx->hev[ctx->hcount % 16u][1], strm); ctx->hslot[ctx->hcount % 16u] = (i); ++ctx->hcount; } } while (0)
#define PROF_BEGIN(i) PROF_BEGIN_ON(i, st)
#define PROF_END(i) PROF_END_ON(i, st)

#define HIPCHK(call)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) { ctx->err = std::string(#call) + ": " + hipGetErrorString(e_); return SURTR_E_HIP; } \
    } while (0)

template <class T>
int DevBuf<T>::grow(surtr_ctx* ctx, size_t need, size_t alloc)
{
    if (p && cap >= need) return SURTR_OK;
    reset();
    const size_t n = std::max(need, alloc);
    const hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
    if (e != hipSuccess)
    {
        p = nullptr;
        (void)hipGetLastError();      // (the runtime keeps the failure as its last error: a later launch check is not to report it again)
        ctx->err = "device allocation of " + std::to_string(n * sizeof(T)) + " bytes: " + hipGetErrorString(e);
        return SURTR_E_HIP;
    }
    cap = n;
    return SURTR_OK;
}

// The resident pieces' host side (pieces_dev.hip), shared with scene_dev.hip.
namespace pieces {
// The buffers of the pieces keep a little room, so that slightly larger pieces fit too; surtr_upload_stats counts their allocations.
template <class T>
int grow_pieces(surtr_ctx* ctx, DevBuf<T>& b, size_t need)
{
    const size_t cap0 = b.cap;
    const int rc = b.grow(ctx, need, std::max<size_t>(need + need / 4, 64));
    if (rc == SURTR_OK && b.cap != cap0) ++ctx->upload_allocs;
    return rc;
}
struct Timer
{
    surtr_ctx* ctx; std::chrono::steady_clock::time_point t0;
    explicit Timer(surtr_ctx* c) : ctx(c), t0(std::chrono::steady_clock::now()) { c->upload_allocs = 0; }
    ~Timer() { ctx->upload_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
};
int reserve_set(surtr_ctx* ctx, PieceSet& S, uint32_t n, uint32_t V, uint32_t H, uint32_t NB);
int derive_set(surtr_ctx* ctx, PieceSet& S, uint32_t n, uint32_t V, const std::vector<uint32_t>& bo_h, bool check, uint32_t H = 0xFFFFFFFFu);
std::vector<uint32_t> sphere_offsets(uint32_t n, const uint32_t* vo);
int host_offsets(uint32_t n, const uint32_t* vo, const uint32_t* off, std::vector<uint32_t>& ho);
int vet_solids(surtr_ctx* ctx, uint32_t n, uint32_t V, uint32_t H, const uint32_t* vo, const uint32_t* loff, const int32_t* nbr, uint32_t* llen, uint8_t* dup);
void set_piece_stats(surtr_ctx* ctx, uint32_t n, const uint32_t* mvo, const uint32_t* mho, const uint32_t* cvo, const uint32_t* cho);
int finish_upload(surtr_ctx* ctx, uint32_t n, bool check);
// Poly::Transform of resident pieces [p0, p0 + n) by world[16 * (p - p0) ..], the derived data again; the other pieces keep their bits
int transform_range(surtr_ctx* ctx, uint32_t p0, uint32_t n, const float* world);
// the same for several disjoint ranges [p0[r], p0[r] + n[r]), world holding the matrices of range 0's pieces, then range 1's, ...:
// one k_transform per range and set, the derived data once per set
int transform_ranges(surtr_ctx* ctx, uint32_t n_ranges, const uint32_t* p0, const uint32_t* n, const float* world);
}
// Poly::Transform of one position (Src/Poly.cpp:580-585): XMVector3TransformCoord(Position, XMMatrixTranspose(matrix)) with
// XMVector3TransformCoord (DirectXMath, not in the reference tree): r = z*M.r[2] + M.r[3]; r = y*M.r[1] + r; r = x*M.r[0] + r;
// result = r.xyz / r.w -- with M = the transpose, M.r[k][c] = W[4*c + k].  k_transform (pieces_dev.hip) writes it, the bounds of
// surtr_scene_bounds (upkeep_dev.hip) take min / max of it: one function, so that the two agree bit for bit.
__host__ __device__ static inline void transform_coord(const float* W, float x, float y, float z, float out[3])
{
    float r[4];
    for (int c = 0; c < 4; ++c)
    {
        float t = z * W[4 * c + 2] + W[4 * c + 3];
        t = y * W[4 * c + 1] + t;
        r[c] = x * W[4 * c] + t;
    }
    out[0] = r[0] / r[3]; out[1] = r[1] / r[3]; out[2] = r[2] / r[3];
}

// The scene's tables as the posed queries (query_dev.hip) and surtr_scene_mass (mass_dev.hip) read them on the device.  Fields only:
// every translation unit that needs them brings them up to date itself, on the context's stream, when the host's have changed.
struct SceneDev { const double* pose; const uint32_t* piece_comp; const uint32_t* comp_off; uint32_t n_comp; };
static inline void scene_reset_poses(surtr_ctx* ctx) { ctx->scene_pose.clear(); ctx->scene_dev_stale = true; }
static inline int scene_sync_device(surtr_ctx* ctx, SceneDev* out)
{
    if (ctx->scene_off.size() < 2 || ctx->scene_off.back() != ctx->n_pieces) return SURTR_E_STATE;
    const uint32_t nc = (uint32_t)ctx->scene_off.size() - 1u, np = ctx->n_pieces;
    if (ctx->scene_dev_stale || !ctx->d_pose || !ctx->d_piece_comp)
    {
        // (refilling the staging vectors is safe although the copies below are "async": they are pageable memory, and a pageable
        //  host-to-device copy has left its source before hipMemcpyAsync returns, as for the tables of surtr_scene_commit)
        std::vector<double>& P = ctx->h_pose_stage; std::vector<uint32_t>& C = ctx->h_comp_stage;
        P.assign((size_t)12 * nc, 0.0); C.resize((size_t)np + nc + 1u);
        for (uint32_t c = 0; c < nc; ++c)
        {
            double* m = P.data() + (size_t)12 * c;
            if (ctx->scene_pose.empty()) { m[0] = m[4] = m[8] = 1.0; }
            else
            {
                const float* W = ctx->scene_pose.data() + (size_t)16 * c;
                for (int r = 0; r < 3; ++r) { for (int k = 0; k < 3; ++k) m[3 * r + k] = (double)W[4 * k + r]; m[9 + r] = (double)W[4 * r + 3]; }
            }
            for (uint32_t p = ctx->scene_off[c]; p < ctx->scene_off[c + 1]; ++p) C[p] = c;
        }
        for (uint32_t c = 0; c <= nc; ++c) C[(size_t)np + c] = ctx->scene_off[c];
        int rc = ctx->d_pose.grow(ctx, P.size(), P.size() + P.size() / 4);
        if (rc == SURTR_OK) rc = ctx->d_piece_comp.grow(ctx, C.size(), C.size() + C.size() / 4);
        if (rc) return rc;
        HIPCHK(hipMemcpyAsync(ctx->d_pose.p, P.data(), P.size() * 8, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(hipMemcpyAsync(ctx->d_piece_comp.p, C.data(), C.size() * 4, hipMemcpyHostToDevice, ctx->stream));
        ctx->scene_dev_stale = false;
        ctx->scene_posef_stale = true;      // (the float poses of surtr_scene_bounds follow on their first use)
    }
    *out = SceneDev{ctx->d_pose.p, ctx->d_piece_comp.p, ctx->d_piece_comp.p + np, nc};
    return SURTR_OK;
}

// A new resident set laid out on the host from the small tables, and the one gather that makes it (scene_dev.hip): shared by
// surtr_scene_commit and the scene edits (upkeep_dev.hip).  Piece p of the new set comes from src[p] >= 0, an old resident piece, or
// from -(k + 1), solid k of the call's other source (the event arena for the commit, the staged pieces for an append); sv / sh: its
// first vertex / ring entry there, dv / dh in the new set (n + 1 entries: the last is the total); table: the new compound table.
namespace scene {
struct SolidsIn { const float* pos; const uint32_t* loff; const int32_t* nbr; };
struct Layout
{
    std::vector<int32_t> src;
    std::vector<uint32_t> sv[2], sh[2], dv[2] = {{0u}, {0u}}, dh[2] = {{0u}, {0u}}, table{0u};
    void push_old(const surtr_ctx* ctx, uint32_t p)
    {
        src.push_back((int32_t)p);
        for (int s = 0; s < 2; ++s)
        {
            sv[s].push_back(ctx->h_vo[s][p]); sh[s].push_back(ctx->h_ho[s][p]);
            dv[s].push_back(dv[s].back() + (ctx->h_vo[s][p + 1] - ctx->h_vo[s][p])); dh[s].push_back(dh[s].back() + (ctx->h_ho[s][p + 1] - ctx->h_ho[s][p]));
        }
    }
    void push_other(uint32_t k, int s, uint32_t v0, uint32_t nv, uint32_t h0, uint32_t nh)      // (once per set; src once)
    {
        if (s == 0) src.push_back(-(int32_t)(k + 1u));
        sv[s].push_back(v0); sh[s].push_back(h0); dv[s].push_back(dv[s].back() + nv); dh[s].push_back(dh[s].back() + nh);
    }
    void close_compound() { if (src.size() != table.back()) table.push_back((uint32_t)src.size()); }
};
// Gathers L into the spare buffers (other[s]: where the src < 0 pieces of set s lie), swaps them in, rebuilds the derived data of the
// whole scene and installs the table and `pose` (empty: every pose the identity).  Synchronises after the gather (*gathered: when)
// but not after the derived data: the caller ends with finish_upload.  Nothing of the scene is touched before the swap.
int regather(surtr_ctx* ctx, const Layout& L, const SolidsIn other[2], std::vector<float>&& pose, std::chrono::steady_clock::time_point* gathered);
extern const float IDENTITY[16];
bool rigid_pose(const float* W);
}

// an event over an explicit pair list with an `outside` mask over all resident pieces (surtr_hip.hip); NULL: no mask
int surtr_event_pairs_masked(surtr_ctx* ctx, uint32_t n_pairs, const uint32_t* pair_cell, const uint32_t* pair_piece, const uint8_t* outside, uint32_t flags);
// The synchronous twin of an _async event call: given what the _async call returned, reads the counts back (surtr_event_counts: one
// small copy and a synchronisation of the context's stream).
static inline int event_sync_counts(surtr_ctx* ctx, int rc_async, surtr_counts* counts)
{
    if (rc_async) return rc_async;
    surtr_counts c{};
    const int rc = surtr_event_counts(ctx, &c);
    if (counts) *counts = c;
    return rc;
}

// Room for n loaded fragments of MV + CV vertices and MH + CH ring entries (Mesh + Convex slots), the largest of them vmax / hmax
// (Mesh slot) and cvmax / chmax (Convex slot): the context's maxima are raised, then scratch, one-wave scratch and arena get the bounds
// of surtr_load_fragments (room for a refit and a triangulation of them).  Nothing is enqueued.  (surtr_hip.hip)
int frags_reserve(surtr_ctx* ctx, uint32_t n, uint32_t vmax, uint32_t hmax, uint32_t cvmax, uint32_t chmax, uint64_t MV, uint64_t CV, uint64_t MH, uint64_t CH);
// The fragments whose records, solids, cursors and counts have been enqueued on the context's stream become the current ones: status
// words cleared, k_faces when `render` (the fan when is_convex), k_out_scan.  No synchronisation.  (surtr_hip.hip)
int frags_present(surtr_ctx* ctx, bool render, int is_convex);

// placement of cell groups with per-group scale / shift already in device memory (surtr_hip.hip)
extern "C" int surtr_place_cells_groups_dev(surtr_ctx* ctx, uint32_t n_groups, const uint32_t* group_cell_off, const float* d_scale3, const float* d_shift3);

// ---- several impacts in one event (surtr_place_cells_impacts, surtr_scene_outside_impacts, surtr_scene_fracture_impacts,
//      surtr_event_regroup_impacts) ----
// One impact's sphere as the kernels read it: origin, radius, and its points [cloud_begin, cloud_begin + cloud_n) of the cloud.
// no_sphere (surtr_event_regroup_impacts_partial): the impact is not partial, k_rg_faces tests none of its pieces and writes 0 for them.
struct alignas(16) ImpSphere { float ox, oy, oz, radius; uint32_t cloud_begin, cloud_n, no_sphere, pad1; };
// The target lists of a call: impact i owns compounds[target_off[i] .. target_off[i + 1]).  K >= 1, no impact without a target, every
// compound in range and named once over all impacts, strictly descending inside an impact.  Anything else: SURTR_E_INVALID.
static inline int impacts_valid(const surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* target_off, const uint32_t* compounds)
{
    if (!n_impacts || !target_off || !compounds || target_off[0] != 0u) return SURTR_E_INVALID;
    std::vector<uint8_t> seen(ctx->scene_off.empty() ? 0 : ctx->scene_off.size() - 1, 0);
    for (uint32_t i = 0; i < n_impacts; ++i)
    {
        if (target_off[i + 1] <= target_off[i]) return SURTR_E_INVALID;
        for (uint32_t t = target_off[i]; t < target_off[i + 1]; ++t)
        {
            const uint32_t c = compounds[t];
            if (c >= seen.size() || seen[c] || (t > target_off[i] && c >= compounds[t - 1])) return SURTR_E_INVALID;
            seen[c] = 1;
        }
    }
    return SURTR_OK;
}
// The spheres of a call: impact i's origin, radius and points [sphere_off[i], sphere_off[i + 1]) of one cloud.  sphere_off starts at 0
// and does not decrease; the cloud may be missing only when it is empty.  Anything else: SURTR_E_INVALID.
static inline int spheres_valid(uint32_t n_impacts, const uint32_t* sphere_off, const float* origins, const float* radii, bool have_points)
{
    if (!sphere_off || !origins || !radii || sphere_off[0] != 0u) return SURTR_E_INVALID;
    for (uint32_t i = 0; i < n_impacts; ++i) if (sphere_off[i + 1] < sphere_off[i]) return SURTR_E_INVALID;
    return sphere_off[n_impacts] && !have_points ? SURTR_E_INVALID : SURTR_OK;
}
static inline void fill_spheres(ImpSphere* tab, uint32_t n_impacts, const uint32_t* sphere_off, const float* origins, const float* radii,
                                const uint8_t* partial = nullptr)
{
    for (uint32_t i = 0; i < n_impacts; ++i)
        tab[i] = ImpSphere{origins[3 * i], origins[3 * i + 1], origins[3 * i + 2], radii[i], sphere_off[i], sphere_off[i + 1] - sphere_off[i],
                           partial && !partial[i] ? 1u : 0u, 0u};
}
// While one of these lives the event's kernels read the instance planes of surtr_place_cells_impacts or surtr_place_cells_patterns, and
// n_cells is the number of cells of all instances: the plain placement's tables are swapped out and come back, untouched, when it goes.
struct ImpactPlanesScope
{
    surtr_ctx* ctx; bool ready; uint32_t n_cells;
    void flip() { std::swap(ctx->d_planes, ctx->d_planes_imp); std::swap(ctx->d_plane_off, ctx->d_plane_off_imp); std::swap(ctx->h_plane_off, ctx->h_plane_off_imp); }
    explicit ImpactPlanesScope(surtr_ctx* c) : ctx(c), ready(c->planes_ready), n_cells(c->n_cells) { flip(); ctx->n_cells = ctx->imp_cell_base.back(); ctx->planes_ready = true; }
    ~ImpactPlanesScope() { flip(); ctx->n_cells = n_cells; ctx->planes_ready = ready; }
    ImpactPlanesScope(const ImpactPlanesScope&) = delete;
    ImpactPlanesScope& operator=(const ImpactPlanesScope&) = delete;
};
