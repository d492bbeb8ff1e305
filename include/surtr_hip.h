/* surtr_hip.h -- C ABI of the MI355X-native fracture engine (libsurtr_hip.so).
 *
 * The reference (W298/Surtr) has no FFI layer; its operator boundary for the
 * fracture-event path is the trio of std::function tasks
 *     m_fractureTask      Inc/Surtr.h:272, body Src/Surtr.cpp:1457-1504
 *     m_refittingTask     Inc/Surtr.h:271, body Src/Surtr.cpp:1449-1455
 *     m_initCompoundTask  Inc/Surtr.h:270, body Src/Surtr.cpp:1436-1447
 * fanned out by Surtr::ApplyFracture (Src/Surtr.cpp:2098-2149), Refitting
 * (2405-2413) and InitCompound (2499-2529).  The entry points below are what a
 * host shim that keeps those C++ signatures binds.
 *
 * Conventions
 *   - plain C types only; every array is a flat buffer with an explicit count;
 *   - a solid (Poly::Polyhedron, Inc/Poly.h:15-32) is CSR: pos f32[3*V],
 *     nbr_off u32[V+1], nbr i32[H] (neighbour rings, CCW seen from outside);
 *   - a set of solids shares one vertex numbering: vert_off u32[n+1] gives the
 *     vertex range of solid i, nbr_off is global over all vertices and the
 *     entries of nbr are indices local to their solid;
 *   - planes are float[4] = (nx,ny,nz,d); the kept side is n.x + d <= 0
 *     (Poly::ClipPolyhedron, Src/Poly.cpp:265-500);
 *   - errors are integer codes (the reference throws std::exception,
 *     Src/Poly.cpp:258, Src/VMACH.cpp:91); 0 is success;
 *   - one context per GPU; calls on a context are serialised by the caller;
 *     contexts are independent (thread-compatible, not thread-safe);
 *   - "dev" pointers are device (HBM) addresses, everything else is host memory.
 */
#ifndef SURTR_HIP_H
#define SURTR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct surtr_ctx surtr_ctx;

enum {
    SURTR_OK = 0,
    SURTR_E_INVALID = 1,   /* bad argument */
    SURTR_E_TOPOLOGY = 2,  /* asymmetric neighbour links / vertex of degree < 3 (Src/Poly.cpp:253-260) */
    SURTR_E_CAPACITY = 3,  /* a device arena or the caller's output buffer is too small */
    SURTR_E_HIP = 4,       /* HIP runtime error, see surtr_last_error */
    SURTR_E_STATE = 5,     /* call order violated (e.g. event before upload) */
    SURTR_E_NOGPU = 6      /* no HIP device: the engine has no CPU fallback */
};

/* Event flags. */
enum {
    SURTR_EVT_REFIT = 1,   /* run m_refittingTask on every fragment's Convex */
    SURTR_EVT_RENDER = 2   /* ExtractFaces + RenderPolyhedron(isConvex=false) of every Mesh */
};

/* Sizes of one event's result (all counts, not bytes). */
typedef struct surtr_counts {
    uint32_t n_frag;       /* non-empty (cell, piece, island) outputs */
    uint32_t mesh_verts, mesh_nbrs;
    uint32_t conv_verts, conv_nbrs;
    uint32_t n_idx;        /* triangle indices (render buffers) */
    uint32_t n_pairs;      /* (cell, piece) pairs processed */
    uint32_t status;       /* device-side status word, SURTR_OK or an error code */
    uint32_t n_failed;     /* THE DEGENERATE POLICY.  Where the reference leaves its own arrays -- a ring entry that names no vertex
                            * (out of range, a removal mark read as a vertex), a link to a clipped vertex renumbered through a stale
                            * or never-set ID (Src/Poly.cpp:484-493), an ExtractFaces walk that never ends (:100-118) -- nothing it
                            * does afterwards is emulated; the unit is FLAGGED and the event stays SURTR_OK.  n_failed counts the
                            * flags: a pair whose Mesh clip has no valid answer yields no fragment (surtr_pair_status names it); a
                            * fragment whose refit has no valid answer keeps its un-refitted Convex, one whose faces cannot be
                            * extracted has no triangles (frag_status names them).  Asked for one solid (surtr_clip_polyhedron,
                            * surtr_refit_solid, ...), the call returns SURTR_E_TOPOLOGY instead.
                            * AN ENGINE LIMIT is flagged the same way, with SURTR_E_CAPACITY in frag_status: a refit at a
                            * RefittingPointLimit above 4 (surtr_set_refit_point_limit) whose limited hull has more than 63 faces --
                            * two slab planes each, 127 planes per clip at most --, overflows the hull kernel's tables or has a
                            * coordinate beyond the range of its edge keys.  The fragment keeps its un-refitted Convex;
                            * surtr_queue_stats out[95] counts these apart. */
} surtr_counts;

/* Host-side view used by surtr_event_download: every pointer may be NULL to
 * skip that array; otherwise it must hold the size noted (from surtr_counts). */
typedef struct surtr_fragments {
    int32_t* frag_ids;          /* 3*n_frag: cell, piece, island (cell-major order, Src/Surtr.cpp:2133-2146) */
    uint32_t* mesh_vert_off;    /* n_frag+1 */
    float* mesh_pos;            /* 3*mesh_verts */
    uint32_t* mesh_nbr_off;     /* mesh_verts+1 (global over all fragments) */
    int32_t* mesh_nbr;          /* mesh_nbrs, fragment-local indices */
    uint32_t* conv_vert_off;    /* n_frag+1 */
    float* conv_pos;            /* 3*conv_verts */
    uint32_t* conv_nbr_off;     /* conv_verts+1 */
    int32_t* conv_nbr;          /* conv_nbrs */
    float* vnc;                 /* 9*mesh_verts: VertexNormalColor (Inc/Mesh.h:4-13) of every Mesh vertex */
    uint32_t* idx_off;          /* n_frag+1 */
    uint32_t* idx;              /* n_idx, fragment-local vertex indices (Src/Poly.cpp:708-713) */
    uint32_t* frag_status;      /* n_frag: SURTR_OK, or SURTR_E_TOPOLOGY for a fragment without triangles / with its Convex not refitted (see n_failed) */
} surtr_fragments;

/* ---- life cycle -------------------------------------------------------- */
int surtr_create(int device, surtr_ctx** out);
void surtr_destroy(surtr_ctx* ctx);
const char* surtr_strerror(int code);
const char* surtr_last_error(surtr_ctx* ctx);
/* Use this HIP stream (hipStream_t passed as void*) for all work; NULL = default stream. */
int surtr_set_stream(surtr_ctx* ctx, void* hip_stream);
/* The stream the context's kernels (surtr_event_pack_dev included) are launched on: a caller that consumes a device blob on
 * another stream orders the two with an event recorded here. */
int surtr_get_stream(surtr_ctx* ctx, void** hip_stream);
/* How many contexts the host keeps busy on this GPU at once (default 1).  It changes no result, only which kernels an event of a
 * few hundred pairs takes: alone on the GPU such an event is shortest with the arrangement that puts the most threads on every pair
 * (the wide pre-pass, one workgroup of the general clipper per pair); with other events beside it the lean arrangement (the regular
 * pre-pass, the record clipper + catcher) leaves them the room and the steps come faster (a 512-cell block of configs[3], four
 * contexts: 0.65 -> 0.55 ms per step; one at a time 1.29 -> 1.37 ms).  The reference has no counterpart (one event at a time,
 * Src/Surtr.cpp:178-254). */
int surtr_set_events_in_flight(surtr_ctx* ctx, uint32_t n);
/* Diagnostic: the plan an event of n_pairs pairs (pair_list != 0: given as a pair list, otherwise a cell range) with `flags` gets
 * from this context now -- which kernels and how many workgroups of each -- with the environment overrides as they stand.  No
 * launch, no synchronisation; SURTR_E_STATE before the context's first event (the plan reads the capacities an event's launch
 * sets).  out[0] n_pairs, [1] the events-in-flight hint, [2] bits: 1 record clipper, 2 split arrangement (main + catcher), 4
 * half-size kernel, 8 Convex clip beside the pre-pass, 16 refit beside faces, 32 lean Convex kernel + second tier, 64 the queue
 * kernels' grids are those of several events in flight, 128 pairs in cell order; [3] pre-pass kernel (0 none, 1 regular, 2 sorted,
 * 3 wide); the grids: [4] Mesh clip, [5] k_clip_convex alone, [6] k_clip_convex_lean, [7] its second tier, [8] pre-pass,
 * [9] k_clip_pairs_big, [10] half-size kernel, [11] its retry, [12] catcher, [13] the catcher's sweep, [14] polling catcher
 * workgroups, [15] refit, [16] k_faces, [17] its second tier (0: the context has none), [18] threads of a k_faces workgroup,
 * [19] the fragments the refit and k_faces grids were sized for, [20] threads of a pre-pass workgroup; the rest 0. */
int surtr_event_plan(surtr_ctx* ctx, uint32_t n_pairs, int pair_list, uint32_t flags, uint32_t out[32]);
/* Override the per-workgroup scratch capacities (vertices, neighbour entries); 0 = automatic. */
int surtr_set_scratch(surtr_ctx* ctx, uint32_t max_verts, uint32_t max_nbrs);
/* Override the result arena capacities (vertices, neighbour entries, indices); 0 = automatic. */
int surtr_set_arena(surtr_ctx* ctx, uint64_t verts, uint64_t nbrs, uint64_t idx);
/* WHAT THE TWO CALLS PROMISE.  Any capacity, however small, gives either the exact event -- bit for bit the one the automatic
 * capacities give -- or SURTR_E_CAPACITY, and nothing is written past a buffer either way.  An arena of exactly what the event
 * takes (surtr_queue_stats out[0..2] after an automatic run: the cursors' final values) succeeds; one entry fewer in any of the
 * three is refused.  Every take adds to its cursor before it compares, so the cursors of a refused event say what it would have
 * needed from the stages that ran.  A scratch smaller than a solid needs refuses the pairs that reach the global clipper with it
 * (SURTR_E_CAPACITY, never a topology flag); the literal clipper, which has nobody to hand on to, flags what does not fit it
 * (out[90]).  The pre-pass's work lists, filled before anything is known to fit, are sized by the largest piece, not by
 * max_verts.  After a refusal surtr_event_counts and surtr_event_download return SURTR_E_CAPACITY, surtr_event_pack_dev writes the
 * header alone, a resident scene is unchanged and its commit is SURTR_E_STATE; with the capacities set back (0 = automatic) the
 * same context gives the event again.  surtr_load_fragments and surtr_scene_fragments size the arena for what they load
 * whatever was set.  tests/test_capacity_limits.py checks this on the emulation: exact event or SURTR_E_CAPACITY on every route;
 * writes past the arena, the tables and the blobs through red zones; writes past a scratch slice only where they change the
 * event, at one probed threshold, and at the end of the pool's last slice (the module says what its zones cannot see). */

/* Per-kernel timing with HIP events recorded on the work stream (the reference's TIMER_* phase
 * timers, Inc/pch.h:122-141, Src/Surtr.cpp:1917-1941).  ms[i] = duration of the last launch of
 * 0 clip_pairs (Mesh), 1 frag_table, 2 refit, 3 faces, 4 out_scan, 5 pack, 6 clip_convex, 7 prep_pairs,
 * 8 clip_pairs_big (or _wave_big), 9 clip_pairs_half, 10 clip_pairs retry launch + the catcher's sweep,
 * 11 clip_pairs_wave (or _main), 13 clip_pairs_catch (the Mesh clip's kernels run side by side on the caller's and
 * two internal streams), 12 frags_from_pieces (surtr_scene_fragments), 14 hulls count + scan, 15 hulls emit + errors
 * (surtr_event_hulls_dev / surtr_pieces_hulls_dev); -1 where not run. */
int surtr_set_profiling(surtr_ctx* ctx, int on);
int surtr_kernel_times(surtr_ctx* ctx, float ms[16]);
/* The durations of the Mesh clip kernel (slot[k] = 0: k_clip_pairs, 11: k_clip_pairs_wave) over the last *n <= 16 events since
 * surtr_set_profiling(ctx, 1), oldest first, without a synchronisation between the events: what a caller that keeps several
 * events in flight (several contexts on several streams) averages for the kernel's launch duration under those conditions. */
int surtr_kernel_history(surtr_ctx* ctx, float ms[16], int slot[16], uint32_t* n);
/* Diagnostic: the device-side counters of the last event (synchronises the stream).  out[0..3] arena use (vertices, ring
 * entries, indices, islands), [5] status, [16+c] pairs of cost class c handed to k_clip_pairs(_big), [32+c] fragments of size
 * class c, [48+c] pairs of pre-pass class c, [64+c] pairs of class c handed to k_clip_pairs_half, [64] pairs that outgrew
 * its half-size LDS topology and were redone by k_clip_pairs, [88] / [89] pairs the record clipper took / handed on to the
 * general clipper ([96+r]: by rule r), [90] solids that were too large for the literal last-resort clipper (more than 32 ring
 * entries at a vertex, or more vertices than its scratch): their pair / fragment is flagged like one without a valid result in
 * the reference -- this counter is how to tell the engine's limit from the reference's undefined behaviour; [95] fragments a
 * refit at a RefittingPointLimit above 4 left un-refitted and flagged SURTR_E_CAPACITY (see n_failed); [80] / [81] Convexes of the
 * pairs the regular one-wave clipper took / handed on (or that started on the literal clipper), [87] pairs k_clip_convex_lean left
 * to k_clip_convex as its second tier (0 after an event that took the one-kernel arrangement). */
int surtr_queue_stats(surtr_ctx* ctx, uint32_t out[128]);
/* Diagnostic: the status of every pair of the last event (0, or the SURTR_E_* code that pair raised), in pair order
 * (cell-major for surtr_fracture_event, list order for surtr_fracture_pairs).  Works after an event that failed. */
int surtr_pair_status(surtr_ctx* ctx, uint32_t n_pairs, uint32_t* status);
/* A cost estimate per pair of the last event (band vertices its Mesh clip worked on + vertices it produced; small for a pair
 * whose Convex came out empty): what a sharded run balances its contiguous rank blocks with ("optional cost
 * balancing must not change output order"; the reference hands one task per cell to whichever pool thread is free,
 * Src/Surtr.cpp:2129-2131). */
int surtr_event_pair_costs(surtr_ctx* ctx, uint32_t n_pairs, uint32_t* cost);

/* ---- inputs ------------------------------------------------------------ */
/* Replaces compound.PieceVec (Inc/Surtr.h:113-134): n pieces, each a (Convex, Mesh)
 * pair of solids.  Copies host -> device once; validates neighbour symmetry
 * and degree >= 3 (SURTR_E_TOPOLOGY).  Ring offsets that decrease or point past the last ring entry are SURTR_E_INVALID, a ring
 * shorter than three or a link that names no vertex of its piece is SURTR_E_TOPOLOGY (the larger code when both occur), whatever
 * the values: the first kernel of the upload vets every offset before it reads a ring and every link before it follows it, and
 * the kernels that walk through links do nothing once it has found a fault.  A refused upload leaves no resident pieces and the
 * context usable. */
int surtr_upload_pieces(surtr_ctx* ctx, uint32_t n_pieces,
                        const uint32_t* mesh_vert_off, const float* mesh_pos,
                        const uint32_t* mesh_nbr_off, const int32_t* mesh_nbr,
                        const uint32_t* conv_vert_off, const float* conv_pos,
                        const uint32_t* conv_nbr_off, const int32_t* conv_nbr);

/* Replaces the std::vector<VMACH::Polygon3D> fracture pattern
 * (Src/Surtr.cpp:1806-1807): n_cells cells, cell c owns faces
 * [face_off[c], face_off[c+1]); v012 holds the first three vertices of every
 * face in pattern space (9 floats), which is all ConstructFacePlane reads
 * (Src/VMACH.cpp:302-310). */
int surtr_upload_pattern(surtr_ctx* ctx, uint32_t n_cells, const uint32_t* face_off, const float* v012);

/* Surtr::GenerateVoronoi(cellPointVec) (Src/Surtr.cpp:2003-2070, the voro++ call) on the device: the bounded Voronoi cells of
 * the seeds in the unit box, one diagram per group (group g owns seeds [group_seed_off[g], group_seed_off[g+1]); one group for
 * a plain pattern, one per first-level fragment for a refracture), installed as the context's fracture pattern exactly as
 * surtr_upload_pattern would (cell = seed, in seed order).  Same cells, face order and coordinates as surtr_voronoi_cells
 * (canonical cell: DESIGN.md section 5).  seeds: 3 doubles per seed. */
int surtr_build_cells(surtr_ctx* ctx, uint32_t n_groups, const uint32_t* group_seed_off, const double* seeds,
                      uint32_t* n_faces, uint32_t* n_face_verts);
/* The cells of the last surtr_build_cells in the layout of surtr_voronoi_cells (+ v012, 9 floats per face); NULL skips an array. */
int surtr_download_cells(surtr_ctx* ctx, uint32_t* cell_face_off, int32_t* face_gen, uint32_t* face_vert_off, double* verts, float* v012);

/* Polygon3D::Scale + Translate + ConstructFacePlane for every face, on the
 * device (Src/VMACH.cpp:506-534; per event at Src/Surtr.cpp:1891-1896). */
int surtr_place_cells(surtr_ctx* ctx, const float scale[3], const float translate[3]);
/* n_impacts >= 1 instances of the uploaded pattern in one launch, one per impact of a frame (surtr_scene_fracture_impacts): placed
 * cell i * n_cells + c is cell c under impact i's scale3[3i..] / translate3[3i..].  The kernel reads every face's v012 once; the
 * pattern is not uploaded again.  The planes of instance i are bit for bit those surtr_place_cells writes for that scale and
 * translate.  They live in tables of their own: the plain placement, and any event after it, are untouched.  Enqueued on the
 * context's stream; a buffer grows (which waits for the device) only when a call places more instances than any before it.
 * SURTR_E_INVALID: n_impacts == 0; SURTR_E_STATE: no pattern.  A new pattern (surtr_upload_pattern, surtr_build_cells,
 * surtr_upload_planes) forgets the instances. */
int surtr_place_cells_impacts(surtr_ctx* ctx, uint32_t n_impacts, const float* scale3, const float* translate3);
/* Diagnostic, for tests: the placed planes (4 floats each, face after face) of the plain placement (impacts == 0: n_faces planes) or
 * of surtr_place_cells_impacts / surtr_place_cells_patterns (impacts != 0: every instance's faces, instance-major).  Count-then-fill: planes == NULL returns *n only;
 * cap = the planes it has room for.  Synchronises the stream. */
int surtr_download_planes(surtr_ctx* ctx, int impacts, uint32_t cap, uint32_t* n, float* planes);

/* ---- the pattern library: several fracture patterns resident on the device ----
 * The reference keeps a partial and a general pattern for the whole session and picks one per event (Src/Surtr.cpp:1806-1807, 1887).
 * The library keeps any number of patterns (face offsets + v012) in device memory beside the installed one, so that a switch of
 * pattern is a device-to-device copy, and so that every impact of a frame can have a pattern of its own
 * (surtr_place_cells_patterns).  It belongs to its context.
 * surtr_pattern_store: copies the installed pattern into the library and returns its id; ids count from 0 in order of storing.
 *   Works after surtr_upload_pattern, surtr_build_cells and surtr_pattern_select alike.  SURTR_E_STATE: no pattern, or one given as
 *   planes (surtr_upload_planes: it has no v012 and cannot be placed).  SURTR_E_CAPACITY: more than 0x7FFFFFFF faces or offsets.
 *   The stored patterns share two grow-only buffers; a growth keeps the patterns already stored bit for bit.
 * surtr_pattern_count / surtr_pattern_info: how many are stored / the cells and faces of one (either pointer may be NULL).
 * surtr_pattern_clear: drops every stored pattern (ids start at 0 again) and forgets the instances of surtr_place_cells_patterns;
 *   the installed pattern, the plain placement and the instances of surtr_place_cells_impacts stay.
 * surtr_pattern_select: installs stored pattern id as the context's pattern, device to device, without a host array.  Afterwards
 *   the context is in the state surtr_upload_pattern of the same arrays leaves: no plain placement, no placed instances, the pair
 *   order forgotten, the cell arrays of the last surtr_build_cells untouched; every later call gives bit-identical results.
 * An unknown id is SURTR_E_INVALID; a failed allocation is SURTR_E_HIP with the reason in surtr_last_error.  After any error the
 * library, the installed pattern and the placements are as they were.
 * The device: every copy is enqueued on the context's stream, behind an event in flight and before any later placement; none of
 * these calls synchronises.  Only a growth waits for the device, when it frees the smaller block: surtr_pattern_store when the
 * library has to grow, surtr_pattern_select when the selected pattern is larger than any the context has held.  count, info and
 * clear touch no device memory. */
#define SURTR_CELLS_ALL 0xFFFFFFFFu
int surtr_pattern_store(surtr_ctx* ctx, uint32_t* id);
int surtr_pattern_count(surtr_ctx* ctx, uint32_t* n);
int surtr_pattern_info(surtr_ctx* ctx, uint32_t id, uint32_t* n_cells, uint32_t* n_faces);
int surtr_pattern_clear(surtr_ctx* ctx);
int surtr_pattern_select(surtr_ctx* ctx, uint32_t id);
/* surtr_place_cells_impacts with a stored pattern per impact, in one launch (k_place_cells_patterns): instance i is stored pattern
 * pattern_id[i] under scale3[3i..] / translate3[3i..].  Ids may repeat and come in any order.  Instance i owns the global cells
 * [cell_base[i], cell_base[i + 1]), cell_base being the prefix sum of its pattern's n_cells, and its planes follow instance i - 1's;
 * they are bit for bit what surtr_pattern_select(pattern_id[i]) + surtr_place_cells writes.  The instances share the tables of
 * surtr_place_cells_impacts: the newer of the two placements replaces the older.  The installed pattern and the plain placement are
 * untouched.  SURTR_E_INVALID: n_impacts == 0 or an id that is not stored; SURTR_E_CAPACITY: more than 0x7FFFFFFF faces or cells
 * over all instances.  A new installed pattern (upload, build, select) or surtr_pattern_clear forgets the instances.
 * The event over them: surtr_scene_fracture_impacts(_async) with cell_begin = 0, cell_end = SURTR_CELLS_ALL takes every cell of every
 * instance (any other range: SURTR_E_INVALID; after surtr_place_cells_impacts SURTR_CELLS_ALL is SURTR_E_INVALID as before).
 * frag_ids carry the global cell number; cell - cell_base[i] is the pattern's own cell. */
int surtr_place_cells_patterns(surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* pattern_id, const float* scale3, const float* translate3);
/* cell_base of the placed instances, after either placement (surtr_place_cells_impacts: i * n_cells).  Count-then-fill: *n =
 * n_impacts + 1; cell_base == NULL returns *n only.  SURTR_E_STATE: no instances. */
int surtr_placed_cells(surtr_ctx* ctx, uint32_t cap, uint32_t* n, uint32_t* cell_base);

/* Alternative to pattern+place: give the cell planes directly. */
int surtr_upload_planes(surtr_ctx* ctx, uint32_t n_cells, const uint32_t* plane_off, const float* planes);

/* ---- the event --------------------------------------------------------- */
/* ApplyFracture over cells [cell_begin, cell_end) x all pieces on device-resident
 * inputs: clip Convex, clip Mesh, split islands, then (flags) refit and
 * triangulate.  `outside` (n_pieces bytes, may be NULL) marks pieces skipped as
 * in Src/Surtr.cpp:1463-1464.  Results stay on the device; counts are returned.
 * Synchronises the stream once to read the counts. */
int surtr_fracture_event(surtr_ctx* ctx, uint32_t cell_begin, uint32_t cell_end,
                         const uint8_t* outside, uint32_t flags, surtr_counts* counts);

/* Same, but does not synchronise or read anything back: for timing loops.
 * The counts of the last event are fetched with surtr_event_counts. */
int surtr_fracture_event_async(surtr_ctx* ctx, uint32_t cell_begin, uint32_t cell_end,
                               const uint8_t* outside, uint32_t flags);
int surtr_event_counts(surtr_ctx* ctx, surtr_counts* counts);

/* Recursive refracture (BASELINE configs[4]): an explicit list of (cell, piece) pairs, processed and output in
 * list order (e.g. fragment-major: every first-level fragment with its own cells).  Same pipeline and result
 * layout as surtr_fracture_event; frag_ids carry the listed cell / piece numbers. */
int surtr_fracture_pairs_async(surtr_ctx* ctx, uint32_t n_pairs, const uint32_t* pair_cell, const uint32_t* pair_piece,
                               uint32_t flags);
/* surtr_place_cells with one (scale, translate) per group of consecutive cells: group g owns cells
 * [group_cell_off[g], group_cell_off[g+1]); scale3 / translate3 hold 3 floats per group. */
int surtr_place_cells_groups(surtr_ctx* ctx, uint32_t n_groups, const uint32_t* group_cell_off, const float* scale3,
                             const float* translate3);

/* The same with group g placed over the bounding box of resident piece g's Mesh (scale = its extent, translate = its centre,
 * Src/Surtr.cpp:1799-1803 applied per piece): the boxes are taken on the device, nothing is read back.  n_groups must equal the
 * number of resident pieces (a recursive refracture after surtr_pieces_from_event + surtr_build_cells). */
int surtr_place_cells_in_pieces(surtr_ctx* ctx, uint32_t n_groups, const uint32_t* group_cell_off);

/* Bytes of the packed device blob holding the last event's fragments. */
size_t surtr_event_blob_bytes(const surtr_counts* counts);
/* Packs the last event's fragments into one contiguous device buffer (for an
 * all-gather over RCCL or a single D2H copy).  Layout: see DESIGN.md.  A buffer that is too small, or an event that was refused
 * (its status word is not SURTR_OK: an arena or a scratch too small), gets the header alone: zero counts, n_pairs and the status. */
int surtr_event_pack_dev(surtr_ctx* ctx, void* dev_blob, size_t capacity_bytes);
/* Splits a host copy of a blob into the arrays of surtr_fragments. */
int surtr_blob_unpack_host(const void* host_blob, size_t bytes, surtr_counts* counts, surtr_fragments* out);
/* Convenience: pack + copy to host + unpack into caller arrays. */
int surtr_event_download(surtr_ctx* ctx, surtr_fragments* out);

/* ---- single-solid operators (the Poly / Kdop API surface) -------------- */
/* Poly::ClipPolyhedron(polyhedron, planes) for one solid, Src/Poly.cpp:556-566.
 * Count-then-fill: call with out_* NULL to get sizes. */
int surtr_clip_polyhedron(surtr_ctx* ctx, uint32_t nv, const float* pos, const uint32_t* nbr_off, const int32_t* nbr,
                          uint32_t n_planes, const float* planes,
                          uint32_t* out_nv, uint32_t* out_nh, float* out_pos, uint32_t* out_nbr_off, int32_t* out_nbr);

/* The three per-Piece tasks for ONE solid (what m_refittingTask and m_initCompoundTask do to a Piece, Inc/Surtr.h:270-271),
 * run by the same kernels as the event.  They use the event arena: the fragments of the last event are gone afterwards.
 *
 * m_refittingTask (Src/Surtr.cpp:1449-1455): ConvexHull(mesh points, min(n, RefittingPointLimit)) -> Kdop::Calc(mesh) ->
 * ClipWithPolyhedron(convex), with the limit of surtr_set_refit_point_limit (4 by default).  Count-then-fill like
 * surtr_clip_polyhedron.  SURTR_E_CAPACITY: the hull is beyond the engine's limits (see n_failed). */
int surtr_refit_solid(surtr_ctx* ctx, uint32_t mesh_nv, const float* mesh_pos, const uint32_t* mesh_nbr_off, const int32_t* mesh_nbr,
                      uint32_t conv_nv, const float* conv_pos, const uint32_t* conv_nbr_off, const int32_t* conv_nbr,
                      uint32_t* out_nv, uint32_t* out_nh, float* out_pos, uint32_t* out_nbr_off, int32_t* out_nbr);
/* Poly::ExtractFaces (Src/Poly.cpp:89-126): face loops in visiting order, face f = face_idx[face_off[f] .. face_off[f+1]).
 * Count-then-fill: NULL arrays return n_faces / n_face_idx only.  SURTR_E_TOPOLOGY where the reference's walk never ends. */
int surtr_extract_faces(surtr_ctx* ctx, uint32_t nv, const float* pos, const uint32_t* nbr_off, const int32_t* nbr,
                        uint32_t* n_faces, uint32_t* n_face_idx, uint32_t* face_off, int32_t* face_idx);
/* Poly::ExtractFaces + Poly::RenderPolyhedron (Src/Poly.cpp:681-714): vnc = 9 floats per vertex (VertexNormalColor with
 * `color`, NULL = 0.25), idx = triangle indices; is_convex selects the fan (:696-706) or EarClipping (:707-713).
 * Count-then-fill: idx NULL returns n_idx. */
int surtr_triangulate(surtr_ctx* ctx, uint32_t nv, const float* pos, const uint32_t* nbr_off, const int32_t* nbr, int is_convex,
                      const float color[3], float* vnc, uint32_t* n_idx, uint32_t* idx);

/* Presents n host pieces as the fragments of an event (fragment k = Mesh k + Convex k, ids = frag_ids[3k..] or
 * (k, 0, 0) when NULL), so that surtr_event_refit / surtr_event_triangulate / surtr_event_download /
 * surtr_pieces_from_event work on solids that did not come out of surtr_fracture_event.  The `outside` mask of an earlier
 * event is dropped: surtr_event_regroup after this call regroups these n fragments alone (bind 0 starts empty).
 * Its device twin, for pieces that are resident already, is surtr_scene_fragments (below): nothing leaves HBM there. */
int surtr_load_fragments(surtr_ctx* ctx, uint32_t n,
                         const uint32_t* mesh_vert_off, const float* mesh_pos, const uint32_t* mesh_nbr_off, const int32_t* mesh_nbr,
                         const uint32_t* conv_vert_off, const float* conv_pos, const uint32_t* conv_nbr_off, const int32_t* conv_nbr,
                         const int32_t* frag_ids);
/* m_initCompoundTask's triangulation (Src/Surtr.cpp:1436-1447) of every Mesh of the current fragments; is_convex as above. */
int surtr_event_triangulate(surtr_ctx* ctx, int is_convex);

/* ---- device-resident pieces -------------------------------------------- */
/* Poly::Transform (Src/Poly.cpp:580-585) of piece i's Convex and Mesh by world[16*i .. 16*i+16) -- the row-major XMMATRIX of
 * m_structuredBufferData[i].WorldMatrix, transposed before use as the reference does -- on the resident copies
 * (ExecuteFractureRoutine's pre-transform, Src/Surtr.cpp:1846-1851).  No host round trip. */
int surtr_transform_pieces(surtr_ctx* ctx, uint32_t n_pieces, const float* world);
/* The fragments of the last event become the resident pieces (recursive refracture without leaving HBM): fragment k is kept
 * when keep[k] != 0; keep == NULL keeps every fragment that is a solid (at least four vertices in Mesh and Convex; a Convex the
 * refit clipped away yields nothing in the reference either, Src/Surtr.cpp:1466-1468).  Kept fragments become pieces 0, 1, ...
 * in fragment order; n_pieces returns their number. */
int surtr_pieces_from_event(surtr_ctx* ctx, const uint8_t* keep, uint32_t* n_pieces);
/* Reads resident piece `piece` back (set 0 = Mesh, 1 = Convex): count-then-fill like surtr_clip_polyhedron.  For tests and for
 * Poly::Transform of a single host polyhedron; the event path never needs it. */
int surtr_download_piece(surtr_ctx* ctx, uint32_t piece, int set, uint32_t* out_nv, uint32_t* out_nh, float* out_pos,
                         uint32_t* out_nbr_off, int32_t* out_nbr);
/* Diagnostic: one array of the data every upload, transform, surtr_pieces_from_event and surtr_scene_commit derives from the
 * resident pieces for the pre-pass (pieces_dev.hip: derive_set), read back as it stands (set 0 = Mesh, 1 = Convex).  V = vertices of
 * the set, n = pieces; arrays over vertices are in piece order, sorted ones (perm, posr_s, row_s) in Morton order inside each piece.
 * Count-then-fill: *bytes is the size of the array; out == NULL returns it only; SURTR_E_CAPACITY when capacity_bytes is smaller.
 * SURTR_E_STATE without resident pieces (SURTR_DERIVED_BUILD needs none).  Synchronises the context's stream; launches nothing and
 * changes nothing.  For tests: the event path never calls it. */
enum {
    SURTR_DERIVED_LLEN = 0,    /* uint32[V]   ring length */
    SURTR_DERIVED_TRI = 1,     /* uint8[V]    1: every face through the vertex is a triangle */
    SURTR_DERIVED_RAD = 2,     /* float[V]    radius of a ball around the vertex that holds every vertex of its faces */
    SURTR_DERIVED_BOX = 3,     /* float[6n]   lo xyz, hi xyz of every piece */
    SURTR_DERIVED_PERM = 4,    /* uint32[V]   piece-local vertex of sorted slot i */
    SURTR_DERIVED_POSR_S = 5,  /* float[4V]   position and ball radius of sorted slot i */
    SURTR_DERIVED_BSPH = 6,    /* float[4 * spheres]  centre, radius: one per build[0] sorted vertices of a piece */
    SURTR_DERIVED_BSPH2 = 7,   /*             one per build[1] spheres of the level below, per piece */
    SURTR_DERIVED_BSPH3 = 8,
    SURTR_DERIVED_IPERM = 9,   /* uint32[V]   sorted slot of piece-local vertex v */
    SURTR_DERIVED_ROW_S = 10,  /* uint16[8V]  header, then up to seven ring entries as sorted slots, 0xFFFF padding */
    SURTR_DERIVED_DUP = 11,    /* uint8[n]    1: some ring of the piece lists a vertex twice */
    SURTR_DERIVED_BO = 12,     /* uint32[n+1] first sphere of every piece at level 1 */
    SURTR_DERIVED_BO2 = 13,    /*             ... level 2 */
    SURTR_DERIVED_BO3 = 14,    /*             ... level 3 */
    SURTR_DERIVED_BUILD = 15,  /* uint32[2]   what the library was built with: vertices per level-1 sphere, spheres per coarser sphere */
    SURTR_DERIVED_COUNT = 16
};
int surtr_pieces_derived(surtr_ctx* ctx, int set, int which, void* out, size_t capacity_bytes, size_t* bytes);
/* Host time of the last surtr_upload_pieces / surtr_pieces_from_event / surtr_transform_pieces / surtr_scene_commit call, in milliseconds,
 * and how many device allocations it made (0 in steady state: the piece buffers are pooled). */
int surtr_upload_stats(surtr_ctx* ctx, float* ms, uint32_t* n_alloc);
/* Diagnostic: the hand-over words of the last event's split Mesh clip (k_clip_pairs_main hands the pairs it cannot finish to
 * k_clip_pairs_catch on another stream; a sweep launch behind both takes what nobody polled for).  Synchronises the context's
 * three streams.  out[0] pairs handed on (pushed), [1] / [2] workgroups of the main kernel that started / signed off (both equal
 * its grid, min(pairs, out[6]), after an event that took the split arrangement; 0 after one that did not), [3] hand-over slots
 * claimed by polling catcher workgroups, [4] the catcher's cursor over its own classes (13..12), [5] the sweep's cursor,
 * [6] the workgroups the last event's clip kernels could use, [7] the hand-over list's capacity (pairs + 4 096). */
int surtr_handover_stats(surtr_ctx* ctx, uint32_t out[8]);
/* Diagnostic: what the last surtr_event_regroup of the context that filled its arrays counted (zeros before the first).  Host
 * values the call had read back anyway: no launch, no copy, no synchronisation.  out[0] pieces, [1] faces of three points or more,
 * [2] points of those faces, [3] touching pairs of faces found (one per pair of FACES, both orders of a pair of pieces included;
 * may exceed [4] when the call returned SURTR_E_CAPACITY), [4] room for them (16 * faces + 1024), [5] rounds of the label
 * propagation including the last, which changes nothing (1 when no pair touched), [6] fragments moved to compound 0 by
 * ConvexOutOfSphere, [7] 0. */
int surtr_regroup_stats(surtr_ctx* ctx, uint32_t out[8]);
/* Diagnostic: the order in which k_clip_convex takes the pairs of the last surtr_fracture_event (pairs of the cells with the most
 * planes first; the order of surtr_fracture_pairs_async's list there): *n entries, relative to the event's first pair.  order ==
 * NULL returns the count only; cap < *n is SURTR_E_CAPACITY. */
int surtr_pair_order(surtr_ctx* ctx, uint32_t cap, uint32_t* n, uint32_t* order);

/* ---- host-side helpers of the harness (no GPU needed) ------------------ */
/* Poly::ExtractNeighborFromMesh, Src/Poly.cpp:128-263: welded triangle soup ->
 * neighbour rings.  nbr must hold 2*3*n_tris entries at most; returns
 * SURTR_E_TOPOLOGY where the reference throws. */
int surtr_neighbors_from_mesh(uint32_t nv, uint32_t n_tris, const int32_t* tris, uint32_t* nbr_off, int32_t* nbr);

/* The same on the device (directed-edge hash table + one fan walk per vertex): identical rings.  kernel_ms (may be NULL)
 * returns the time of the kernels, copies excluded. */
int surtr_neighbors_from_mesh_dev(surtr_ctx* ctx, uint32_t nv, uint32_t n_tris, const int32_t* tris, uint32_t* nbr_off, int32_t* nbr,
                                  float* kernel_ms);

/* Canonical bounded Voronoi cells of n seeds in the unit box (replaces the
 * voro++ call of Src/Surtr.cpp:2003-2070; see DESIGN.md for the face order).
 * Count-then-fill: pass NULL arrays to get n_faces / n_face_verts. */
int surtr_voronoi_cells(uint32_t n, const double* seeds, uint32_t* n_faces, uint32_t* n_face_verts,
                        uint32_t* cell_face_off, int32_t* face_gen, uint32_t* face_vert_off, double* verts);

/* VMACH::ConvexHull(points, limit) + Surtr::GenerateICHNormal (Src/VMACH.cpp:869-1161, Src/Surtr.cpp:1961-1974):
 * unit normals of the faces of the greedy limited hull, in face creation order.  Count-then-fill. */
int surtr_hull_normals(uint32_t n, const float* points, uint32_t limit, uint32_t capacity, float* normals, uint32_t* count);

/* Kdop::KdopContainer::Calc(vertices, maxAxisScale, planeGapInv) (Src/Kdop.cpp:15-51): for every normal the Min
 * plane then the Max plane (the order ClipWithPolyhedron clips in, :166-179); planes holds 8 floats per normal. */
int surtr_kdop_ach_planes(uint32_t n, const float* points, uint32_t k, const float* normals, double max_axis_scale,
                          float plane_gap_inv, float* planes);

/* Plane(p0, p1, p2) as PolygonFace::ConstructFacePlane builds it (Src/VMACH.cpp:302-310; normalised, SimpleMath.inl:2773-2780). */
int surtr_plane_from_points(const float p0[3], const float p1[3], const float p2[3], float plane[4]);

/* Kdop::KdopContainer::Calc(const Poly::Polyhedron&) (Src/Kdop.cpp:92-115): Min plane then Max plane per normal through the
 * first extreme vertices, not normalised, no gap (the refit variant; k_refit does the same per fragment on the device). */
int surtr_kdop_planes(uint32_t n, const float* points, uint32_t k, const float* normals, float* planes);

/* Poly::Moments (Src/Poly.cpp:55-87): signed volume and centroid of a closed solid (host; the test invariant of
 * fragment volumes partition the input). */
int surtr_moments(uint32_t nv, const float* pos, const uint32_t* nbr_off, const int32_t* nbr, double* volume, float centroid[3]);

/* ---- mesh files either side of the path (host) --------------------------------- */
/* Wavefront OBJ in, with the conventions of Surtr::LoadModelData and its assimp flags (Src/Surtr.cpp:2683-2727):
 * one vertex per distinct position in order of first use, polygons as fans, winding flipped, x negated, then
 * scale/translate.  Count-then-fill: with pos or tris NULL only *n_verts / *n_tris are written. */
int surtr_read_obj(const char* path, const float scale[3], const float translate[3], uint32_t cap_verts, uint32_t cap_tris,
                   float* pos, int32_t* tris, uint32_t* n_verts, uint32_t* n_tris);
/* The render buffers of an event (surtr_fragments: vnc = 36-byte VertexNormalColor, Inc/Mesh.h:4-13) as one OBJ
 * object per fragment. */
int surtr_write_obj(const char* path, uint32_t n_frag, const int32_t* frag_ids, const uint32_t* mesh_vert_off, const float* vnc,
                    const uint32_t* idx_off, const uint32_t* idx);

/* ---- the step after the event: compound regrouping (host side) ---------------- */
/* Surtr::ConvexOutOfSphere (Src/Surtr.cpp:2415-2458) for one Convex; sphere_points are already placed. */
int surtr_convex_out_of_sphere(uint32_t nv, const float* pos, const uint32_t* nbr_off, const int32_t* nbr, uint32_t n_sphere,
                               const float* sphere_points, const float origin[3], float radius, int* out);

/* Bind sets of ApplyFracture (Src/Surtr.cpp:2103-2146) + MergeOutOfImpact (:2368-2403, when `partial`) +
 * HandleConvexIsland (:2203-2366) on the un-refitted Convex solids of an event.
 * Pieces [0, n_outside) are the pieces kept whole outside the impact sphere (bind 0); pieces
 * [n_outside, n_pieces) are the event's fragments in output order, piece_cell[p] = their cell (consecutive
 * fragments of one cell form one compound).  conv_nbr_off is global over all vertices, conv_nbr local per piece.
 * Output: compound c owns compound_piece[compound_off[c] .. compound_off[c+1]) (ascending piece indices);
 * compound 0 is the outside set; compound_off needs n_pieces + 2 entries, compound_piece n_pieces. */
int surtr_regroup(uint32_t n_pieces, uint32_t n_outside, const int32_t* piece_cell,
                  const uint32_t* conv_vert_off, const float* conv_pos, const uint32_t* conv_nbr_off, const int32_t* conv_nbr,
                  int partial, uint32_t n_sphere, const float* sphere_points, const float origin[3], float radius,
                  uint32_t* n_compounds, uint32_t* compound_off, int32_t* compound_piece);

/* The same regrouping as a device step on the last event (regroup_dev.hip): the Convex solids stay in HBM; faces, planes, the
 * ConvexOutOfSphere test, candidate face pairs (radix sort by |d|), the overlap tests and the label propagation over pieces
 * run in kernels; only per-piece flags and labels come back.  Pieces are numbered as for surtr_regroup: the resident pieces
 * the event skipped (its `outside` mask, ascending), then the event's fragments in output order.  Call it BEFORE
 * surtr_event_refit (the reference regroups on the un-refitted Convex solids).  compound_off needs *n_pieces + 2 entries,
 * compound_piece *n_pieces (call with both NULL to get n_pieces).
 * Limits: a Convex of more than 4096 half-edges (or vertices), or more than 16 * faces + 1024 touching pairs of faces (only solids
 * thinner than the rule's 1e-3 window get there), give SURTR_E_CAPACITY; the context stays usable.
 * State: the skipped pieces are read from the resident pieces, so they must still be the ones the event ran over.  After
 * surtr_load_fragments there is no mask (see there).  After surtr_pieces_from_event the fragments are still the event's but its
 * pieces are gone: if the event's mask kept any piece out, the call returns SURTR_E_STATE (regroup before handing the fragments
 * on); an event without a mask, or with a mask of zeros, regroups as before.
 * After surtr_scene_fracture_event only the skipped pieces of the event's compound are numbered (ascending), then the fragments:
 * pieces of other bodies are in no bind set.
 * CAPACITY AFTER A BODIES EVENT: after surtr_scene_fracture_bodies with n_targets > 1 every body has a bind 0 of its own, and this
 * call (which takes no capacity) writes up to *n_pieces + n_targets + 1 offsets: size compound_off for that, not n_pieces + 2, or
 * use surtr_event_regroup_bodies, whose sizes-only call returns the number of bodies. */
int surtr_event_regroup(surtr_ctx* ctx, int partial, uint32_t n_sphere, const float* sphere_points, const float origin[3], float radius,
                        uint32_t* n_pieces, uint32_t* n_compounds, uint32_t* compound_off, int32_t* compound_piece);
/* The same with one more output: which compounds belong to which body of the event.  After surtr_scene_fracture_bodies a body is a
 * target of the click, in the order the targets were given; after any other event there is one body.  *n_bodies is set by every
 * call (the one with NULL arrays included); body_compound_off (may be NULL) gets *n_bodies + 1 entries: body b's compounds are
 * compounds [body_compound_off[b], body_compound_off[b + 1]), the first of them its bind 0 (the pieces out of the impact, possibly
 * none).  compound_off needs *n_pieces + *n_bodies + 1 entries.
 *   Pieces are numbered as above: the skipped resident pieces of every target, ascending, then the fragments in output order.
 *   A bind set belongs to one body: bind 0 is made per body; the cell binds are cut where the cell or the body changes (the last cell
 *   of one body and the first of the next may carry the same number); MergeOutOfImpact moves a fragment to its own body's bind 0;
 *   the groups HandleConvexIsland splits off follow their own body's binds.  The kernels run once over all the pieces.
 *   Each body's compounds are, in order and in membership, what surtr_event_regroup returns for that body's own event.
 * surtr_event_regroup after a bodies event returns the same compounds without the extra array (its compound_off then needs
 * *n_pieces + n_targets + 1 entries as well: every body has a bind 0 of its own). */
int surtr_event_regroup_bodies(surtr_ctx* ctx, int partial, uint32_t n_sphere, const float* sphere_points, const float origin[3], float radius,
                               uint32_t* n_pieces, uint32_t* n_compounds, uint32_t* compound_off, int32_t* compound_piece,
                               uint32_t* n_bodies, uint32_t* body_compound_off);
/* surtr_event_regroup_bodies after surtr_scene_fracture_impacts, with the sphere of each body's own impact: impact i has origin
 * origins[3i..], radius radii[i] and the points [sphere_off[i], sphere_off[i + 1]) of sphere_points (3 floats each; sphere_off[0] = 0,
 * ascending).  A body is a target, in the order the targets were given (impact after impact); ConvexOutOfSphere of a fragment
 * (k_rg_faces) uses the impact its body belongs to.  The per-body binds, the move to a body's own bind 0 and the island groups are
 * those of surtr_event_regroup_bodies; the kernels run once over all the pieces.  Each body's compounds are what
 * surtr_event_regroup returns for the event of that body's impact alone.  !partial: no sphere is read (the arrays may be NULL).
 * SURTR_E_STATE: the last event is not surtr_scene_fracture_impacts' over n_impacts impacts.  Sizes as surtr_event_regroup_bodies. */
int surtr_event_regroup_impacts(surtr_ctx* ctx, int partial, uint32_t n_impacts, const uint32_t* sphere_off, const float* sphere_points,
                                const float* origins, const float* radii, uint32_t* n_pieces, uint32_t* n_compounds, uint32_t* compound_off,
                                int32_t* compound_piece, uint32_t* n_bodies, uint32_t* body_compound_off);

/* surtr_event_regroup_impacts with a flag per impact (one byte each): the bodies of an impact with partial[i] == 0 are tested against
 * no sphere and see no MergeOutOfImpact; its cloud range may be empty, and its origin and radius are not used.  The bodies of the
 * other impacts are treated as surtr_event_regroup_impacts(partial = 1) treats them.  All ones equals
 * surtr_event_regroup_impacts(1, ...), all zeros surtr_event_regroup_impacts(0, ...), bit for bit.  After either placement. */
int surtr_event_regroup_impacts_partial(surtr_ctx* ctx, const uint8_t* partial, uint32_t n_impacts, const uint32_t* sphere_off, const float* sphere_points,
                                        const float* origins, const float* radii, uint32_t* n_pieces, uint32_t* n_compounds, uint32_t* compound_off,
                                        int32_t* compound_piece, uint32_t* n_bodies, uint32_t* body_compound_off);

/* Runs m_refittingTask (and the output scan) on the fragments of the last event: the reference regroups on the
 * un-refitted Convex solids and refits afterwards (Src/Surtr.cpp:1921-1939). */
int surtr_event_refit(surtr_ctx* ctx);

/* FractureArgs::RefittingPointLimit (Inc/Surtr.h:93): the points of the limited hull whose face normals give a fragment's
 * slab planes, per fragment min(mesh vertices, n).  4 (the default) to 32; anything else returns SURTR_E_INVALID and leaves
 * the setting as it was.  Read by SURTR_EVT_REFIT, surtr_event_refit and surtr_refit_solid.  A larger limit means more planes
 * per clip and larger Convex solids: set it before the event (or surtr_load_fragments) whose arena is to have room for them. */
int surtr_set_refit_point_limit(surtr_ctx* ctx, uint32_t n);
int surtr_get_refit_point_limit(surtr_ctx* ctx, uint32_t* n);
/* For tests: the device's limited hull (the one k_refit_n builds per fragment) of one cloud of n >= 4 points, as
 * surtr_hull_normals returns the host's; and the key of one coordinate in its edge keys -- the digits of printf("%f"):
 * sign bit, |x| * 10^6 rounded half-to-even on the exact value (SURTR_E_CAPACITY: out of range). */
int surtr_hull_normals_device(surtr_ctx* ctx, uint32_t n, const float* points, uint32_t limit, uint32_t capacity, float* normals, uint32_t* count);
int surtr_coord_key(float x, uint32_t* neg, uint64_t* scaled);

/* ---- mass properties (mass_dev.hip) ------------------------------------ */
/* What PxRigidBodyExt::updateMassAndInertia(body, 10.0f) gives InitCompound (Src/Surtr.cpp:2520), per closed solid.
 * Definition: the faces are the loops Poly::ExtractFaces walks on the neighbour rings, each fanned around its lowest-numbered
 * vertex; the volume integrals of 1, x, y, z, x^2, y^2, z^2, xy, yz, zx are taken relative to the solid's vertex 0 (the origin
 * shift of Poly::Moments, Src/Poly.cpp:55-87), with positions converted to double and every product and sum in double.  The
 * reductions run in a fixed order (no float atomics): two calls give the same bits whatever the stream, the events-in-flight
 * hint or the other contexts. */
typedef struct surtr_mass {
    double volume;         /* signed, the integral of 1 */
    double mass;           /* density * volume */
    double com[3];         /* centre of mass, world space */
    double inertia[6];     /* about com, world axes: Ixx Iyy Izz Ixy Iyz Izx as tensor entries (Ixy = -density * int (x-cx)(y-cy)) */
    uint32_t nv;           /* vertices of the solid */
    uint32_t status;       /* 0 ok; 1 fewer than 4 vertices (zero record, as Poly::Moments); 2 volume <= 0;
                            * 3 a face walk did not close (a ring does not list the vertex it was reached from) */
} surtr_mass;

/* One record per fragment of the last event, in fragment order, into dev_out (device memory, capacity_bytes >= 96 * n_frag).
 * set 0 = Mesh, 1 = Convex: the Convex the context holds (refitted after SURTR_EVT_REFIT or surtr_event_refit, un-refitted
 * otherwise).  Enqueued on the context's stream with no host synchronisation, like surtr_event_pack_dev; it uses one temporary
 * device allocation ordered on that stream.  SURTR_E_STATE with no event (or after an event that failed), SURTR_E_CAPACITY when
 * the buffer is too small; nothing is written in either case.  When the host does not hold the event's counts (after
 * surtr_fracture_event_async without surtr_event_counts) the capacity is checked on the device, which then writes nothing. */
int surtr_event_mass_dev(surtr_ctx* ctx, int set, float density, void* dev_out, size_t capacity_bytes);
/* The same for the resident pieces (surtr_upload_pieces / surtr_pieces_from_event), in piece order.  SURTR_E_STATE before any
 * upload. */
int surtr_pieces_mass_dev(surtr_ctx* ctx, int set, float density, void* dev_out, size_t capacity_bytes);
/* Host conveniences, synchronous: *n = number of records; out == NULL returns the count only; with out, *n must hold its
 * capacity (SURTR_E_CAPACITY and *n = the count when it is too small). */
int surtr_event_mass(surtr_ctx* ctx, int set, float density, uint32_t* n, surtr_mass* out);
int surtr_pieces_mass(surtr_ctx* ctx, int set, float density, uint32_t* n, surtr_mass* out);
/* The records of compounds from those of their pieces (parallel-axis theorem; host, no GPU): compound c is
 * compound_piece[compound_off[c] .. compound_off[c+1]), exactly as surtr_event_regroup returns them.  Its pieces are the resident
 * pieces the event skipped (its `outside` mask, ascending) followed by the event's fragments, so build `pieces` as
 *     pieces[k]              = surtr_pieces_mass record of the k-th skipped resident piece   (k < n_outside)
 *     pieces[n_outside + f]  = surtr_event_mass record of fragment f
 * taken BEFORE surtr_pieces_from_event replaces the resident pieces, with the same set and density.  volume, mass and nv add up,
 * status is the largest of the members' (2 when the sum of the volumes is <= 0); com is mass-weighted (volume-weighted when the
 * density is 0). */
int surtr_combine_mass(uint32_t n_compounds, const uint32_t* compound_off, const int32_t* compound_piece, const surtr_mass* pieces,
                       surtr_mass* out);

/* ---- picking: ray cast and sphere overlap on the resident pieces (query_dev.hip) ---- */
/* What OnMouseDown asks of PhysX (gScene->raycast, gScene->overlap, Src/Surtr.cpp:178-254), on the Convex solids of the resident
 * pieces in world space as they stand (after surtr_transform_pieces / surtr_pieces_from_event), without a download.
 * Definition: the faces of a solid are the loops Poly::ExtractFaces walks; a face's plane is surtr_plane_from_points through the
 * loop's smallest-numbered vertex and the two that follow it in loop order; inside is n.x + d <= 0.
 *   ray (origin o, direction d -- unit length if t is to be a distance; it is not normalised here --, max_dist >= 0, +inf allowed):
 *     the interval [0, max_dist] is clipped by every half-space (Cyrus-Beck); a solid is hit when t_enter <= t_exit, at
 *     t = max(t_enter, 0) with the normal of the entering plane.  An origin inside every half-space gives t = 0, pos = o,
 *     normal = -d and SURTR_RAY_STARTS_INSIDE (PhysX's initial overlap).  Over the pieces: the smallest t, the lowest piece on a tie.
 *   sphere (centre c, radius r >= 0): a solid is touched when the distance from c to it is <= r (0 inside; else the minimum over
 *     its edges and over the faces onto which c projects inside the face).
 * A piece is hit (touched) only if the ray crosses (the sphere reaches) the box of its vertices: no difference for a convex solid;
 * it bounds what a face plane through three nearly collinear vertices can claim.  Everything is evaluated in double from the
 * float positions; the records are float.
 * Max, min and lowest index are order-independent: two calls give the same bits whatever the stream or the other work on the GPU.
 * A solid that cannot be queried is never hit and never touched, and surtr_pieces_query_status says why. */
typedef struct surtr_ray_hit {
    int32_t piece;         /* resident piece hit, -1: none */
    uint32_t status;       /* SURTR_RAY_* bits */
    float t;               /* parameter of the hit along d */
    float pos[3];          /* o + t * d */
    float normal[3];       /* unit normal of the face entered (-d when the ray starts inside) */
    uint32_t reserved[3];  /* zero; the record is 48 bytes */
} surtr_ray_hit;
enum {
    SURTR_RAY_STARTS_INSIDE = 1,   /* the origin is inside the piece: t = 0 */
    SURTR_RAY_INVALID = 2          /* zero or non-finite direction, non-finite origin, max_dist negative or NaN: no hit (_dev forms) */
};
enum {                             /* per-piece status of a query; 0 = the solid was queried */
    SURTR_QUERY_FEW = 1,           /* fewer than four vertices */
    SURTR_QUERY_OPEN = 2,          /* a ring entry names no vertex, or a face walk does not close (or closes after two steps) */
    SURTR_QUERY_FLAT = 4,          /* a face of zero (or non-finite) normal */
    SURTR_QUERY_LONG = 8           /* a face loop of more than 256 vertices */
};
/* n_rays >= 1 rays of 7 floats (o, d, max_dist) in device memory -> n_rays records in dev_hits (capacity_bytes >= 48 * n_rays,
 * else SURTR_E_CAPACITY and nothing is written).  Enqueued on the context's stream with no host synchronisation; one temporary
 * device allocation ordered on that stream.  SURTR_E_STATE without resident pieces.  An invalid ray gets SURTR_RAY_INVALID. */
int surtr_pieces_raycast_dev(surtr_ctx* ctx, uint32_t n_rays, const float* dev_rays, void* dev_hits, size_t capacity_bytes);
/* The same from and to host arrays; synchronises.  An invalid ray is SURTR_E_INVALID here and nothing is run. */
int surtr_pieces_raycast(surtr_ctx* ctx, uint32_t n_rays, const float* rays, surtr_ray_hit* hits);
/* n_spheres >= 1 spheres of 4 floats (c, r) -> dev_mask[s * n_pieces + p] (capacity_bytes >= n_spheres * n_pieces): 0 not touched,
 * 1 touched.  With dev_mass_or_null (the n_pieces surtr_mass records surtr_pieces_mass_dev wrote) a touched piece of
 * mass <= min_mass gets 2 instead: touched but too light to fracture (Src/Surtr.cpp:228).  A sphere that is not finite or has a
 * negative radius touches nothing. */
int surtr_pieces_overlap_dev(surtr_ctx* ctx, uint32_t n_spheres, const float* dev_spheres, const void* dev_mass_or_null, float min_mass,
                             uint8_t* dev_mask, size_t capacity_bytes);
/* The same from and to host arrays; synchronises.  mask == NULL returns the number of resident pieces in *n_pieces; with mask,
 * *n_pieces must hold the pieces a row has room for (SURTR_E_CAPACITY and the count when too small).  A sphere that is not finite
 * or has a negative radius is SURTR_E_INVALID. */
int surtr_pieces_overlap(surtr_ctx* ctx, uint32_t n_spheres, const float* spheres, const surtr_mass* mass_or_null, float min_mass,
                         uint32_t* n_pieces, uint8_t* mask);
/* The SURTR_QUERY_* bits of every piece as the last query found them (n >= the pieces of that query; synchronises).
 * SURTR_E_STATE before the first query. */
int surtr_pieces_query_status(surtr_ctx* ctx, uint32_t n, uint32_t* status);

/* ---- the scene: several bodies in the resident set (scene_dev.hip) ---- */
/* FractureStorage::CompoundVec on the device, and the bookkeeping of ExecuteFractureRoutine (Src/Surtr.cpp:1829-1883): pick ->
 * fracture -> commit -> pick without a download.  A compound is a contiguous range of resident pieces, the order of
 * m_structuredBufferData (:1840-1843): compound c owns pieces [compound_off[c], compound_off[c + 1]).  After surtr_upload_pieces
 * and surtr_pieces_from_event the scene is ONE compound holding every piece, so every other call behaves as it does without these.
 *
 * surtr_scene_set_compounds: n_compounds + 1 offsets, ascending from 0 to the number of resident pieces, no empty compound;
 * anything else is SURTR_E_INVALID.  SURTR_E_STATE without resident pieces.
 * surtr_scene_get_compounds: count-then-fill -- compound_off == NULL returns *n_compounds only; with it, cap is the entries it
 * has room for (n_compounds + 1 are written; SURTR_E_CAPACITY when too small). */
int surtr_scene_set_compounds(surtr_ctx* ctx, uint32_t n_compounds, const uint32_t* compound_off);
int surtr_scene_get_compounds(surtr_ctx* ctx, uint32_t cap, uint32_t* n_compounds, uint32_t* compound_off);
/* Poly::Transform of the pieces of one compound only (:1846-1851): n = its number of pieces, world = one matrix per piece of the
 * compound as for surtr_transform_pieces.  The other pieces keep their bits; the derived data is rebuilt.  Like
 * surtr_transform_pieces it forgets the last event. */
int surtr_scene_transform_compound(surtr_ctx* ctx, uint32_t compound, uint32_t n, const float* world);
/* surtr_fracture_event over the pieces of `compound` only: `outside` (may be NULL) has one byte per piece of that compound, in
 * resident order; pieces of other compounds produce no pair; frag_ids carry RESIDENT piece numbers; fragments come in the same
 * cell-major order.  surtr_event_regroup after it numbers that compound's skipped pieces (ascending), then the fragments: pieces
 * of other bodies are in no bind set.  surtr_event_refit, surtr_event_mass(_dev) and surtr_event_download work as after any event. */
int surtr_scene_fracture_event(surtr_ctx* ctx, uint32_t compound, uint32_t cell_begin, uint32_t cell_end, const uint8_t* outside,
                               uint32_t flags, surtr_counts* counts);
int surtr_scene_fracture_event_async(surtr_ctx* ctx, uint32_t compound, uint32_t cell_begin, uint32_t cell_end, const uint8_t* outside,
                                     uint32_t flags);
/* One event over the pieces of several compounds: every body a click's impact sphere touches (OnMouseDown, Src/Surtr.cpp:213-253) in
 * one pass instead of one event, regroup and commit per body.  compounds: n_targets >= 1 compound numbers, STRICTLY DESCENDING (so
 * that the committed scene is the one n_targets commits in that order leave), no duplicate, in range; anything else is
 * SURTR_E_INVALID and changes nothing.  outside (may be NULL): one byte per piece of the listed compounds, concatenated in the order
 * given, each compound in resident order -- the layout surtr_scene_outside returns.  The pair list is target-major in the given
 * order and cell-major over the target's pieces within a target; frag_ids carry resident piece numbers.  With one target every
 * result equals surtr_scene_fracture_event's bit for bit.  Follow with surtr_event_regroup_bodies (or surtr_event_regroup),
 * surtr_event_refit and ONE surtr_scene_commit. */
int surtr_scene_fracture_bodies(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, uint32_t cell_begin, uint32_t cell_end,
                                const uint8_t* outside, uint32_t flags, surtr_counts* counts);
int surtr_scene_fracture_bodies_async(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, uint32_t cell_begin, uint32_t cell_end,
                                      const uint8_t* outside, uint32_t flags);
/* Surtr::ConvexOutOfSphere (Src/Surtr.cpp:2415-2458) of the resident Convex solids of the listed compounds (any order, in range), on
 * the device: one byte per piece, concatenated in the order the compounds are given, each compound in resident order; 1 where every
 * vertex is at least `radius` from `origin` and no point of the cloud lies inside all face planes -- the answer of
 * surtr_convex_out_of_sphere on the downloaded solid, bit for bit, for every solid that is a regular polyhedron (no ring lists a
 * neighbour twice, no face loop passes through a vertex twice: every convex hull and every unflagged fragment).  The kernel finds
 * the faces in parallel, not in ExtractFaces' visiting order; on a solid that breaks the precondition the byte is defined and
 * deterministic but may differ from the host's.  One launch, one wave per piece (k_scene_outside).
 * surtr_scene_outside: count-then-fill -- outside == NULL returns *n only; with it, cap is the bytes it has room for
 * (SURTR_E_CAPACITY when too small).  surtr_scene_outside_dev: cloud and mask in device memory, enqueued on the context's stream,
 * nothing is read back; the piece list goes through a buffer of the context that is reallocated (which waits for the device) only
 * when a call lists more pieces than any before it.  A Convex of more than 4096 half-edges (or vertices) gives SURTR_E_CAPACITY before anything is enqueued;
 * the context stays usable.  Poses are not applied: bake them first (surtr_scene_apply_poses). */
int surtr_scene_outside(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, uint32_t n_sphere, const float* sphere_points,
                        const float origin[3], float radius, uint32_t cap, uint32_t* n, uint8_t* outside);
int surtr_scene_outside_dev(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, uint32_t n_sphere, const float* dev_sphere_points,
                            const float origin[3], float radius, uint8_t* dev_outside, size_t capacity_bytes);
/* ---- several impacts in one frame: one event, one regroup, one commit ----
 * A solver reports several contacts above the threshold in one frame (setContactReportThreshold and the contact callback,
 * Src/Surtr.cpp:1163, 2518).  An IMPACT is an origin, a radius, a placement of the pattern, a range of cloud points and a list of
 * target compounds.  A call takes n_impacts >= 1 of them: impact i owns compounds[target_off[i] .. target_off[i + 1]) (target_off[0]
 * = 0).  The lists are pairwise disjoint; inside an impact the targets are strictly descending; across impacts any order.
 * THE RULE: every result is, bit for bit, what the one-impact calls leave when they run impact after impact in the order given
 * (surtr_scene_apply_poses, surtr_place_cells, surtr_scene_outside, surtr_scene_fracture_bodies, surtr_event_regroup_bodies,
 * surtr_event_refit, surtr_scene_commit; the later impacts' compound numbers moved down by the commits before them).  The committed
 * scene: every untouched compound in its old order with its pose, then what impact 0 made, then impact 1's, ...
 * Errors, each leaving the scene, table, poses and any current event as they were: SURTR_E_INVALID for n_impacts == 0, an impact
 * without a target, a compound out of range or listed twice (inside one impact or under two), targets inside an impact that do not
 * strictly descend; the event calls return SURTR_E_STATE without surtr_place_cells_impacts, or with another n_impacts than was placed.
 * Two impacts on one body are out of scope (the second would meet the first's fragments: a second call).
 *
 * surtr_scene_outside_impacts(_dev): surtr_scene_outside with a sphere per piece, one launch, one wave per listed piece
 * (k_scene_outside_impacts); every piece reads its impact's origin, radius and cloud range [sphere_off[i], sphere_off[i + 1]) from a
 * small device table.  The bytes come impact-major, then in surtr_scene_outside's layout, and equal surtr_scene_outside of each impact
 * alone.  Same 4096-half-edge rule, refused before anything is enqueued.  Count-then-fill / _dev as surtr_scene_outside.
 * surtr_scene_fracture_impacts(_async): the event over instance cells [cell_begin, cell_end) of each impact's placement.  The pair
 * list is impact-major, then target-major, then cell-major; frag_ids carry i * n_cells + c and resident piece numbers; outside (may be
 * NULL) is what surtr_scene_outside_impacts returns.  With one impact every result equals surtr_scene_fracture_bodies' bit for bit.
 * Follow with surtr_event_regroup_impacts, surtr_event_refit and ONE surtr_scene_commit, which erases every target of every impact
 * with its pose and appends the returned compounds in order. */
int surtr_scene_outside_impacts(surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* target_off, const uint32_t* compounds, const uint32_t* sphere_off,
                                const float* sphere_points, const float* origins, const float* radii, uint32_t cap, uint32_t* n, uint8_t* outside);
int surtr_scene_outside_impacts_dev(surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* target_off, const uint32_t* compounds, const uint32_t* sphere_off,
                                    const float* dev_sphere_points, const float* origins, const float* radii, uint8_t* dev_outside, size_t capacity_bytes);
int surtr_scene_fracture_impacts(surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* target_off, const uint32_t* compounds, uint32_t cell_begin,
                                 uint32_t cell_end, const uint8_t* outside, uint32_t flags, surtr_counts* counts);
int surtr_scene_fracture_impacts_async(surtr_ctx* ctx, uint32_t n_impacts, const uint32_t* target_off, const uint32_t* compounds, uint32_t cell_begin,
                                       uint32_t cell_end, const uint8_t* outside, uint32_t flags);
/* Makes the resident set what :1856-1875 make CompoundVec: the event's compound is erased, the compounds it broke into are pushed
 * to the back.  (n_compounds, compound_off, compound_piece) are the compounds exactly as surtr_event_regroup returned them for the
 * last scene event (compound 0, the pieces out of the impact, included).
 *   New order: the pieces of every other compound first, in their old order (the compounds above the target move down by one);
 *   then, for each returned compound in order, its members: skipped resident pieces are copied as they stand, fragments come from
 *   the event arena with the Convex the context holds (refitted if surtr_event_refit ran).  The new compounds get the numbers
 *   *first_new_compound .. + *n_new_compounds - 1.
 *   Left out: a fragment that is no solid (Mesh or Convex of fewer than four vertices, as surtr_pieces_from_event) or that is
 *   flagged (frag_status != 0); a compound left without pieces is not created.
 *   src (may be NULL; room for the resident pieces + the event's fragments): one value per new piece, >= 0 the old resident piece,
 *   -(f + 1) fragment f.  *n_pieces = the new number of resident pieces.
 * The layout is made on the host from the small tables; one kernel gathers both sets from the old pieces and the arena into spare
 * buffers kept in the context, which are then swapped in; the derived data of the whole scene is rebuilt.  From the second commit
 * of a scene of steady size on, surtr_upload_stats reports 0 allocations.
 * SURTR_E_STATE: no scene event; the event failed; the event was committed already; the resident pieces were replaced or
 * transformed, the compound table set, or the scene edited (surtr_scene_remove / _append / _cull), since the event.  SURTR_E_INVALID: the compounds do not cover pieces 0 .. n-1 exactly once
 * (or nothing would be left).  On any error the scene is unchanged.
 * After surtr_scene_fracture_bodies: every target is erased, with its pose; the other compounds stay first, in their old order;
 * the returned compounds (all bodies', as surtr_event_regroup_bodies gave them) are appended in order, the skipped pieces of any
 * target as they stand; one gather and one rebuild of the derived data.  Because the targets descend, the scene is the one that
 * one commit per target, in that order, leaves. */
int surtr_scene_commit(surtr_ctx* ctx, uint32_t n_compounds, const uint32_t* compound_off, const int32_t* compound_piece,
                       uint32_t* n_pieces, uint32_t* first_new_compound, uint32_t* n_new_compounds, int32_t* src);
/* InitCompound on the scene (Src/Surtr.cpp:2499-2529, m_initCompoundTask :1436-1447): the resident pieces of the listed compounds become
 * the current fragments, device to device.  `compounds == NULL` means every compound, ascending.  Fragments come in list order, and
 * inside a compound in piece order.  frag_ids = (compound, resident piece number, 0).  Convex slot = the piece's Convex.  Mesh slot =
 * the piece's Mesh, or with render_convex != 0 a second copy of the Convex.  flags: 0 or SURTR_EVT_RENDER.  With SURTR_EVT_RENDER the
 * Mesh slot is triangulated at once (EarClipping, or the fan when render_convex), as by surtr_event_triangulate(ctx, render_convex).
 * The scene, its table and its poses are not touched, and positions are those of the resident frame (no pose applied).  Like the
 * single-solid operators it uses the event arena: the fragments of the last event are gone, and a surtr_scene_commit after it is
 * SURTR_E_STATE.  Everything that reads the current fragments works on them: surtr_event_triangulate, surtr_event_refit,
 * surtr_event_mass(_dev), surtr_event_pack_dev, surtr_event_download.  Synchronises once to return the counts; the _async form does not.
 * Errors, each leaving the scene and any current event as they were: SURTR_E_STATE without resident pieces; SURTR_E_INVALID for a
 * compound out of range or listed twice, n_targets == 0 with a list, or any other flag (SURTR_EVT_REFIT included: call
 * surtr_event_refit next); SURTR_E_CAPACITY for more fragments than the fragment table can hold; a failed growth of the arena or the
 * scratch is reported as by surtr_load_fragments.  With surtr_set_profiling the copy kernel's time is slot 12 of surtr_kernel_times. */
int surtr_scene_fragments(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, int render_convex, uint32_t flags, surtr_counts* counts);
int surtr_scene_fragments_async(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds, int render_convex, uint32_t flags);
/* Diagnostic: host time of the last surtr_scene_commit in milliseconds, in two parts that both end in a stream synchronisation --
 * checks, layout, tables and the gather kernel; then the swap, the derived data of the whole scene (derive_set) and the piece
 * statistics. */
int surtr_scene_commit_times(surtr_ctx* ctx, float* gather_ms, float* derive_ms);

/* ---- per-body poses: pick, gate and break bodies that have moved (scene_dev.hip, query_dev.hip, mass_dev.hip) ---- */
/* Every body of the reference is a rigid actor whose pose Update writes into m_structuredBufferData[i].WorldMatrix each frame
 * (Src/Surtr.cpp:347-352); OnMouseDown queries the bodies where they are (:207-233) and ExecuteFractureRoutine bakes the pose into
 * the pieces just before the event (:1846-1851).  Here: one pose per compound, kept on the host next to the compound table.  The
 * resident pieces stay in the frame they were committed in (the body frame); a pose change rewrites no vertex.
 *
 * world: 16 floats per compound in the layout surtr_transform_pieces takes, x' = A x + b with A[c][k] = W[4c+k], b[c] = W[4c+3].
 * A pose must be rigid -- evaluated in double from the floats: every entry finite, the last row exactly (0,0,0,1),
 * max |A^T A - I| <= 1e-4, det A > 0.  Anything else, or an n_compounds that is not the scene's, is SURTR_E_INVALID and leaves the
 * table as it was.  No call keeps a host pointer.  An empty table means every pose is the identity.
 *   reset to the identity by: surtr_upload_pieces, surtr_pieces_from_event, surtr_scene_set_compounds;
 *   left alone by:            surtr_transform_pieces, surtr_scene_transform_compound (explicit bakes);
 *   surtr_scene_commit:       every surviving compound keeps its pose (those above the target move down by one with it), the
 *                             compounds it makes get the identity -- the event ran on baked, world-space pieces, which is what
 *                             InitCompound(compound, false) without a translate does (:1874-1875).  On any commit error the poses
 *                             are unchanged, as the scene is.
 *   surtr_scene_remove / _append / _cull: every surviving compound keeps its pose and moves down with it, an appended compound gets
 *                             the pose given with it (scene upkeep, below); on any error the poses are unchanged.
 * surtr_scene_get_poses: count-then-fill as surtr_scene_get_compounds (cap = the matrices world has room for).
 * surtr_scene_apply_pose: a pose that is bit for bit the identity matrix does nothing and forgets nothing; any other is exactly
 * surtr_scene_transform_compound(compound, n, that matrix n times) followed by pose := identity (the derived data is rebuilt, the
 * last event is forgotten). */
int surtr_scene_set_poses(surtr_ctx* ctx, uint32_t n_compounds, const float* world);
int surtr_scene_get_poses(surtr_ctx* ctx, uint32_t cap, uint32_t* n_compounds, float* world);
int surtr_scene_apply_pose(surtr_ctx* ctx, uint32_t compound);
/* surtr_scene_apply_pose for several compounds (any order, in range; one named twice is baked once): one transform launch per
 * compound whose pose is not bit for bit the identity, the derived data rebuilt ONCE, those poses set to the identity.  The resident
 * bits are those surtr_scene_apply_pose per compound leaves.  When every pose is the identity nothing happens at all. */
int surtr_scene_apply_poses(surtr_ctx* ctx, uint32_t n_targets, const uint32_t* compounds);

/* Ray cast and sphere overlap on the posed scene.  Definition: that of surtr_pieces_raycast / surtr_pieces_overlap, applied per
 * piece in that piece's body frame.  For piece p of compound c with pose (A, b):
 *   ray     o' = A^T (o - b), d' = A^T d, in double from the floats; the box test and Cyrus-Beck run on (o', d', max_dist) against the
 *           piece as it is resident.  t is the same number in both frames: over all pieces the smallest t, the lowest piece on a tie.
 *           pos = o + t d from the world ray; normal = A n' evaluated in double and rounded to float, not renormalised.  A ray that
 *           starts inside gives t = 0, pos = o, normal = -d of the world ray and SURTR_RAY_STARTS_INSIDE.
 *   sphere  c' = A^T (c - b), r unchanged, then the per-piece test.
 * With every pose the identity each value equals the corresponding value of surtr_pieces_raycast / surtr_pieces_overlap (-0 against
 * +0 in a normal apart).  Invalid rays and spheres, capacities, SURTR_E_STATE and surtr_pieces_query_status are as in those calls.
 * The device copy of the poses (A^T and b as 12 doubles per compound, a compound number per piece) is brought up to date on the
 * context's stream by the first query after a change. */
typedef struct surtr_scene_ray_hit {
    int32_t piece;         /* resident piece hit, -1: none */
    uint32_t status;       /* SURTR_RAY_* bits */
    float t;
    float pos[3];          /* o + t * d, world */
    float normal[3];       /* A n', world */
    int32_t compound;      /* the body of that piece; -1 with piece == -1 */
    uint32_t reserved[2];  /* zero; the record is 48 bytes */
} surtr_scene_ray_hit;
int surtr_scene_raycast_dev(surtr_ctx* ctx, uint32_t n_rays, const float* dev_rays, void* dev_hits, size_t capacity_bytes);
int surtr_scene_raycast(surtr_ctx* ctx, uint32_t n_rays, const float* rays, surtr_scene_ray_hit* hits);
/* dev_piece_mask (may be NULL; piece_cap >= n_spheres * n_pieces): [s * n_pieces + p] = 0 or 1, with no gate.
 * dev_body_mask (body_cap >= n_spheres * n_compounds): [s * n_compounds + c] = 0 no piece of c is touched, 1 some piece is, 2 touched
 * but body_mass[c].mass <= min_mass (Src/Surtr.cpp:228, on the actor as the reference does it); dev_body_mass_or_null: the
 * n_compounds records surtr_scene_mass_dev wrote, NULL: no gate. */
int surtr_scene_overlap_dev(surtr_ctx* ctx, uint32_t n_spheres, const float* dev_spheres, const void* dev_body_mass_or_null, float min_mass,
                            uint8_t* dev_piece_mask_or_null, size_t piece_cap, uint8_t* dev_body_mask, size_t body_cap);
/* From and to host arrays; synchronises.  body_mask == NULL returns the number of compounds in *n_compounds; with it, *n_compounds
 * must hold the compounds a row has room for (SURTR_E_CAPACITY and the count when too small). */
int surtr_scene_overlap(surtr_ctx* ctx, uint32_t n_spheres, const float* spheres, const surtr_mass* body_mass_or_null, float min_mass,
                        uint32_t* n_compounds, uint8_t* body_mask);

/* One surtr_mass record per compound of the scene, in the resident (body) frame: what setMass / setCMassLocalPose /
 * setMassSpaceInertiaTensor take for a body whose pose the solver holds.  Each record is bit-identical to surtr_combine_mass applied
 * to the surtr_pieces_mass records of that compound's pieces in resident order (the additions run in piece order; the by-volume rule
 * and the status rule carry over).  The _dev form (capacity_bytes >= 96 * n_compounds) is enqueued on the context's stream with no
 * host synchronisation and one temporary allocation for the per-piece records; the host form is count-then-fill as
 * surtr_pieces_mass. */
int surtr_scene_mass_dev(surtr_ctx* ctx, int set, float density, void* dev_out, size_t capacity_bytes);
int surtr_scene_mass(surtr_ctx* ctx, int set, float density, uint32_t* n, surtr_mass* out);

/* ---- collision hulls: face loops and planes of every Convex (hull_dev.hip) ---- */
/* What Compound::PieceExtractedConvex holds for CookingConvexManual (Src/Surtr.cpp:2151-2155, 2555-2614), for every Convex of the
 * current fragments or of the resident pieces, as the arrays PxConvexMeshDesc::polygons / indices take -- with planes that hold
 * (PxPlane(f[0], f[1], f[2]) in float does not where a loop starts on three nearly collinear vertices) and a verdict per solid.
 *
 * FACES.  The faces of a solid are the loops Poly::ExtractFaces yields, in its order: loops come by (start vertex, ring slot), each
 * starts at its smallest vertex, and a later slot that repeats a neighbour starts no face of its own.
 * PLANE of a loop q_0 .. q_(k-1), positions converted to double, every product and sum a separate double operation:
 *     N = sum_{i=1}^{k-2} (q_i - q_0) x (q_{i+1} - q_0), summed in loop order
 *     n = N / sqrt(N.N),  N.N = (Nx Nx + Ny Ny) + Nz Nz
 *     t_i = (n.x q_i.x + n.y q_i.y) + n.z q_i.z,   d = -(max t_i + min t_i) / 2
 *     plane = (n, d) rounded to float.  N exactly zero: plane = 0 and SURTR_HULL_FLAT; the polygon and its indices are still
 *     written, and the face takes no part in the two errors.
 * ERRORS, in double from the FLOAT plane as written, ((n.x x + n.y y) + n.z z) + d, then rounded to float:
 *     convexity = max over (vertex, non-flat face) of that value (0 when every face is flat): how far a vertex stands in front of a
 *                 face plane -- a sliver face whose normal is noise shows here;
 *     planarity = max over the non-flat faces and their OWN vertices of its magnitude.
 *   A maximum is order-independent and nothing is accumulated with atomics: the same bits whatever the stream, the
 *   events-in-flight hint or the other work on the GPU.
 * STATUS.  FEW: fewer than four vertices.  LARGE: more than 65 535 vertices or ring entries (decided from the counts, before any
 * walk; a solid with FEW or LARGE gets no other withholding bit).  OPEN: a ring entry names no vertex, a position is not finite, a
 * link lacks its way back, or a walk does not close within the solid's ring entries.  IRREGULAR: a ring lists a neighbour twice; the
 * walk of a half-edge comes back to its start vertex, on another half-edge, before it closes or meets a smaller vertex (ExtractFaces
 * ends a loop at its start vertex); the number of ring entries H is odd; or V - H / 2 + F != 2.  OVER_255: more than 255 vertices or
 * written faces (PhysX's hull limit): information only, it withholds nothing.
 * FEW, OPEN, IRREGULAR and LARGE WITHHOLD the output: n_faces = n_idx = max_loop = 0 and convexity = planarity = extent = 0.  A solid
 * with none of them carries exactly ExtractFaces' loops. */
typedef struct surtr_hull_polygon {     /* 20 bytes: PxHullPolygon's layout */
    float plane[4];        /* (n, d): inside is n.x + d <= 0 */
    uint16_t n_verts;      /* vertices of the loop */
    uint16_t index_base;   /* first index of the loop, counted from the solid's idx_off */
} surtr_hull_polygon;
typedef struct surtr_hull {             /* 48 bytes per solid */
    uint32_t nv, n_faces, n_idx, status;   /* n_faces / n_idx: what was WRITTEN for this solid; status: SURTR_HULL_* bits */
    uint32_t face_off, idx_off;            /* first polygon / first index: exclusive sums over the solids before it */
    uint32_t max_loop, reserved0;          /* vertices of the longest loop */
    float convexity;                       /* max over (vertex, non-flat face) of n.x + d */
    float planarity;                       /* max over non-flat faces and their OWN vertices of |n.x + d| */
    float extent;                          /* largest edge of the box of the vertices (float): the scale the two errors are read against */
    uint32_t reserved1;
} surtr_hull;
enum { SURTR_HULL_FEW = 1, SURTR_HULL_OPEN = 2, SURTR_HULL_FLAT = 4, SURTR_HULL_IRREGULAR = 8, SURTR_HULL_LARGE = 16, SURTR_HULL_OVER_255 = 32 };
/* The Convex of every current fragment (the one the context holds: refitted or not, whatever frag_status says), in fragment order.
 * dev_records (device memory) takes one 48-byte header, then one surtr_hull per fragment; the header's nv = the solids, n_faces /
 * n_idx = the totals, status = SURTR_OK or SURTR_E_CAPACITY.  dev_polys has room for polys_cap polygons, dev_idx for idx_cap
 * indices (16-bit, solid-local: PxConvexFlag::e16_BIT_INDICES); surtr_counts::conv_nbrs / 3 polygons and conv_nbrs indices are always
 * enough for solids that are written.  Enqueued on the context's stream with no host synchronisation; one temporary device allocation
 * ordered on that stream; with surtr_set_profiling, slot 14 of surtr_kernel_times is count + scan and slot 15 emit + errors.
 * SURTR_E_STATE with no event or after an event that failed.  SURTR_E_CAPACITY, before anything is enqueued, when records_bytes
 * cannot hold the header or -- where the host holds the event's counts -- the records.  Everything else is checked on the device (the
 * totals are known only there): when something does not fit, the header is written with status SURTR_E_CAPACITY and the totals
 * needed, and nothing else is. */
int surtr_event_hulls_dev(surtr_ctx* ctx, void* dev_records, size_t records_bytes, surtr_hull_polygon* dev_polys, size_t polys_cap,
                          uint16_t* dev_idx, size_t idx_cap);
/* The same for the Convex solids of the resident pieces, in piece order.  SURTR_E_STATE before any upload.  Bodies of the scene go
 * through surtr_scene_fragments(compounds, ...) and then surtr_event_hulls. */
int surtr_pieces_hulls_dev(surtr_ctx* ctx, void* dev_records, size_t records_bytes, surtr_hull_polygon* dev_polys, size_t polys_cap,
                           uint16_t* dev_idx, size_t idx_cap);
/* Host forms, synchronous, count-then-fill: with the three arrays NULL, *n / *n_polys / *n_idx return the records (without the
 * header), polygons and indices; with all three given they must hold the capacities (SURTR_E_CAPACITY and the counts when one is too
 * small; some but not all arrays NULL is SURTR_E_INVALID). */
int surtr_event_hulls(surtr_ctx* ctx, uint32_t* n, surtr_hull* records, uint32_t* n_polys, surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx);
int surtr_pieces_hulls(surtr_ctx* ctx, uint32_t* n, surtr_hull* records, uint32_t* n_polys, surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx);

/* ---- scene upkeep: world bounds per body; remove, append and cull bodies (upkeep_dev.hip) ---- */
/* BOUNDS.  What a solver's broad phase, a renderer's culling and a kill volume ask every frame: the world-space box of every body,
 * taken on the device from the resident pieces and the poses.  set 0 = Mesh, 1 = Convex.  For body c with float pose W the box is the
 * componentwise min / max over the positions surtr_scene_apply_pose(c) would write for its pieces: the arithmetic of
 * surtr_transform_pieces in float, operation for operation (one function computes both).  A body whose pose is bit for bit the
 * identity (or a scene without poses) gives the box of its resident positions, as apply_pose then rewrites nothing.  min and max are
 * exact and associative: the result does not depend on how the reduction is arranged (plain stores and wave reductions, no atomics);
 * results compare equal as numbers, -0 and +0 may differ.  Each of the three coordinates is taken by itself: one that is not finite
 * sets SURTR_BOUNDS_NONFINITE and takes no part, so lo / hi cover the finite ones (lo = FLT_MAX, hi = -FLT_MAX on an axis without any).
 * The per-piece boxes of surtr_pieces_derived (SURTR_DERIVED_BOX) are body-frame boxes: these are not boxes of those. */
typedef struct surtr_bounds { float lo[3]; float hi[3]; uint32_t n_vertices; uint32_t status; } surtr_bounds;   /* 32 bytes */
#define SURTR_BOUNDS_NONFINITE 1u   /* some coordinate of the body is not finite; lo / hi then cover the finite ones only */
/* One record per compound into dev_body (device memory, body_cap_bytes >= 32 * n_compounds) and, with dev_piece_or_null, the same
 * record per resident piece (piece_cap_bytes >= 32 * n_pieces), each piece under its body's pose.  Two launches on the context's
 * stream, no host synchronisation: one workgroup per piece, then one wave per body over its contiguous piece records.  The float
 * poses (64 bytes per compound) are brought to the device by the first call after the poses or the table change.  Without a piece
 * buffer the piece records go to a buffer of the context that is reallocated (which waits for the device) only when the scene has
 * more pieces than ever before.  SURTR_E_STATE without resident pieces, SURTR_E_CAPACITY when a buffer is too small; nothing is
 * written in either case. */
int surtr_scene_bounds_dev(surtr_ctx* ctx, int set, void* dev_body, size_t body_cap_bytes, void* dev_piece_or_null, size_t piece_cap_bytes);
/* Host form, synchronous, count-then-fill as surtr_scene_mass: the records of the compounds. */
int surtr_scene_bounds(surtr_ctx* ctx, int set, uint32_t* n, surtr_bounds* out);

/* EDITS.  The set of bodies changes without a solid leaving HBM: one gather of the kept pieces into the spare buffers of
 * surtr_scene_commit, a swap, and the derived data of the whole scene again -- the commit's own path (the layout code is shared).
 * From the second edit of a scene of steady size on, surtr_upload_stats reports 0 allocations.
 * State rules, for surtr_scene_remove, surtr_scene_append and a surtr_scene_cull that removes:
 *   the pieces move:          a surtr_scene_commit after an edit is SURTR_E_STATE, as after a transform;
 *   the last event:           its fragments stay downloadable, as after a commit; its `outside` mask and its compound numbers are
 *                             forgotten (surtr_event_regroup after an edit sees an event without a mask);
 *   poses:                    every surviving compound keeps its pose and moves down with it; appended compounds get the pose given;
 *   on any error:             the scene, the poses and the table are unchanged, bit for bit;
 *   surtr_set_events_in_flight and a non-default stream behave as for the commit.
 *
 * surtr_scene_remove: compounds[n] in any order, each in range and named once, else SURTR_E_INVALID; removing every body is
 * SURTR_E_INVALID, as a commit that keeps nothing is.  The surviving pieces keep their order, and so do the surviving compounds.
 * src (may be NULL; room for the resident pieces): the old resident piece of every new piece.  *n_pieces = the new count. */
int surtr_scene_remove(surtr_ctx* ctx, uint32_t n, const uint32_t* compounds, uint32_t* n_pieces, int32_t* src_or_null);
/* surtr_scene_append: n_bodies >= 1 new compounds go to the back (push_back); body b owns the new pieces
 * [body_piece_off[b], body_piece_off[b + 1]) (ascending from 0, no empty body).  The eight arrays are those of surtr_upload_pieces
 * for the new pieces alone.  No existing piece is uploaded again.  world_or_null: 16 floats per new body, rigid as
 * surtr_scene_set_poses demands (else SURTR_E_INVALID); NULL: the identity.  Existing poses stay; a scene without a pose table gets
 * one only if a pose arrives that is not bit for bit the identity.  The new pieces are vetted exactly as an upload vets them -- the
 * host checks of surtr_upload_pieces, then the link check on the device, run on the pieces where they are staged, before the scene
 * is touched: the same faults give the same codes, but unlike a refused upload a refused append leaves the scene as it was.
 * *first_new_compound = the number of the first appended compound. */
int surtr_scene_append(surtr_ctx* ctx, uint32_t n_bodies, const uint32_t* body_piece_off, const uint32_t* mvo, const float* mpos, const uint32_t* moff,
                       const int32_t* mnbr, const uint32_t* cvo, const float* cpos, const uint32_t* coff, const int32_t* cnbr,
                       const float* world_or_null, uint32_t* first_new_compound);
/* surtr_scene_cull: marks, on the device, the bodies a solver drops, and with apply != 0 removes them (surtr_scene_remove's path).
 * reason[c]: SURTR_CULL_LIGHT when the body's surtr_scene_mass record (set, density) has status == 0 and mass <= min_mass -- the
 * reference's gate 1e-4 of Src/Surtr.cpp:228 turned into a removal rule; SURTR_CULL_OUTSIDE when keep_box6_or_null (lo xyz, hi xyz;
 * a NaN in it is SURTR_E_INVALID) is given, the body's bounds of the CONVEX set have status == 0 and its box is disjoint from the
 * keep box: for some k, hi[k] < keep.lo[k] or lo[k] > keep.hi[k].  Masses and bounds stay on the device; one lane per body marks;
 * only the reason bytes come back.  Count-then-fill: reason == NULL returns *n_compounds only; with it, *n_compounds must hold its
 * capacity (SURTR_E_CAPACITY and the count when too small).  *n_removed = the bodies removed (0 without apply).  If every body is
 * marked, nothing is removed, the reasons are still filled and the call is SURTR_E_INVALID. */
enum { SURTR_CULL_LIGHT = 1, SURTR_CULL_OUTSIDE = 2 };
int surtr_scene_cull(surtr_ctx* ctx, int set, float density, float min_mass, const float* keep_box6_or_null, int apply,
                     uint32_t* n_compounds, uint8_t* reason, uint32_t* n_removed);

/* ---- scene contacts: which bodies are within a margin of each other, through which pieces, how far apart, where (contact_dev.hip) ----
 * What the fracture cycle takes as its input (surtr_scene_fracture_impacts: "a solver reports contacts"), from the resident Convex
 * solids and the poses, every frame, without a download.  DEFINITION, so that a result can be checked:
 *   World vertices   of piece p of body c: the float positions surtr_scene_apply_pose(c) would write for its Convex (transform_coord,
 *                    operation for operation; a pose that is bit for bit the identity transforms nothing), converted to double.
 *   Broad phase      on the surtr_bounds records of surtr_scene_bounds(set 1): bodies a < b are a candidate pair when, for every axis k,
 *                    (double)lo_a[k] - (double)hi_b[k] <= (double)margin and (double)lo_b[k] - (double)hi_a[k] <= (double)margin.  A body
 *                    whose record has SURTR_BOUNDS_NONFINITE is in no pair.
 *   Mid phase        the same test on the per-piece records, for every piece p of a and q of b of a candidate body pair.  Pieces of
 *                    one body are never paired.
 *   Narrow phase     d = the Euclidean distance between the convex hulls of the two world vertex sets, in double (GJK); S = the largest
 *                    absolute world coordinate of the two solids.  d <= 2^-24 * S: SURTR_CONTACT_OVERLAP, distance = 0, point_a =
 *                    point_b = a point of both hulls, normal = 0 (below that the float input cannot tell touching from penetrating; no
 *                    penetration depth is computed).  Otherwise point_a in hull(A) and point_b in hull(B) are closest points, normal =
 *                    (point_b - point_a) / d, distance = d, each rounded to float.  Where closest points are not unique any closest
 *                    pair is a valid answer.  A pair is REPORTED when it overlaps or d <= margin.
 *   Order            records ascend by (piece_a, piece_b); compounds are contiguous ranges of pieces and a < b, so body_a never descends.
 * GJK stops when the support vertex pair is already in the simplex, when |v|^2 - v.w <= 2^-36 |v|^2 + 2^-44 S |v| (v the simplex's
 * closest point, w the new support point: d is then known to a relative 2^-36 and an absolute 2^-44 S, far below the float rounding
 * of the output), when the simplex's new closest point is no nearer than its last (the old one lies in the new simplex: the arithmetic
 * has reached its own rounding), or after 96 iterations (SURTR_CONTACT_ITER: the best answer so far).  Ties in the support function go to the lowest
 * vertex number, nothing is accumulated with atomics, the lists are placed by count -> scan -> fill: two calls on the same scene give
 * the same bits, whatever the stream, the events-in-flight hint or the other work on the GPU. */
typedef struct surtr_contact {            /* 64 bytes */
    uint32_t body_a, body_b;              /* a < b */
    uint32_t piece_a, piece_b;            /* resident pieces; piece_a belongs to body_a */
    float    distance;                    /* >= 0 */
    uint32_t status;                      /* SURTR_CONTACT_* bits */
    float    point_a[3], point_b[3], normal[3];
    uint32_t reserved;                    /* zero */
} surtr_contact;
enum { SURTR_CONTACT_OVERLAP = 1, SURTR_CONTACT_ITER = 2 };
typedef struct surtr_contact_header {     /* 64 bytes, in front of the records of the _dev form */
    uint32_t status;                      /* SURTR_OK or SURTR_E_CAPACITY */
    uint32_t n_records;                   /* records written (with SURTR_E_CAPACITY: needed) */
    uint32_t n_body_pairs, n_piece_pairs; /* candidates of the broad / mid phase */
    uint32_t n_bodies, n_pieces;          /* of the scene */
    uint32_t lists;                       /* 0; bit 0 / bit 1: the body / piece candidates outgrew the call's lists (below) */
    uint32_t reserved[9];                 /* zero */
} surtr_contact_header;
#define SURTR_CONTACT_MAX_PAIRS 2097152u  /* candidates of either kind one call has room for */
/* dev_records (device memory) takes the header, then the records.  The rules of surtr_event_hulls_dev hold: enqueued on the context's
 * stream, no host synchronisation, one temporary device allocation ordered on that stream (besides the bounds records, which go to
 * buffers of the context as in surtr_scene_bounds_dev), no slot of surtr_kernel_times (all sixteen are taken; surtr_scene_contacts_times
 * below).  SURTR_E_INVALID for a margin that is negative or not finite, SURTR_E_STATE without resident pieces, SURTR_E_CAPACITY before
 * anything is enqueued when records_bytes cannot hold the header.  The totals are known only on the device: when the records do not fit,
 * the header is written with SURTR_E_CAPACITY and the totals needed, and nothing else is.  The candidate lists are sized on the host for
 * the worst case of the scene (every body near every other), up to SURTR_CONTACT_MAX_PAIRS entries each; a scene that outgrows that
 * gives the header SURTR_E_CAPACITY, the bit in `lists`, the totals found so far and zero for those behind (the body stage is
 * all-pairs; scenes of 10^5 bodies need a sweep or a grid in front of it, which is not here). */
int surtr_scene_contacts_dev(surtr_ctx* ctx, float margin, void* dev_records, size_t records_bytes);
/* Host form, count-then-fill, synchronises: out == NULL returns *n = the records; with out, *n must hold its capacity (SURTR_E_CAPACITY
 * and the count when too small).  The pairs are found once; the records are gathered again into room for all of them. */
int surtr_scene_contacts(surtr_ctx* ctx, float margin, uint32_t* n, surtr_contact* out);
/* The header of a run alone, on the host (status SURTR_OK unless a list was outgrown); synchronises. */
int surtr_scene_contacts_totals(surtr_ctx* ctx, float margin, surtr_contact_header* totals);
/* With surtr_set_profiling: the device time of the last surtr_scene_contacts_dev by phase, in ms: [0] bounds, [1] body and piece pairs
 * (count, scan, fill, twice), [2] distances, [3] flag scan, header and gather; -1 where not run.  Synchronises the context's stream. */
int surtr_scene_contacts_times(surtr_ctx* ctx, float ms[4]);

/* ---- cooked hulls: weld, convex hull and coplanar merge of the points of a Convex (cook_dev.hip) ---- */
/* For the solids surtr::HullUsable refuses (a sliver in the rings: SURTR_HULL_FLAT or a large convexity): the convex hull of the
 * solid's POINTS, built on the device, as the arrays PxConvexMeshDesc takes (points, PxHullPolygon records, 16-bit indices).  The
 * rings are not read.  What CookingConvex (Src/Surtr.cpp:2531-2553: eWELD_VERTICES, eCOMPUTE_CONVEX, planeTolerance 7e-6) asks of
 * PhysX.  Input per solid: float positions p_0 .. p_(n-1), weld_dist >= 0, plane_tol >= 0 (both absolute).  All arithmetic is double,
 * positions converted to double, every product, sum, division and square root a separate operation, in the order written.
 *
 * 1 WELD.  In ascending index, point i is KEPT iff no kept j < i has ((dx dx + dy dy) + dz dz) <= weld_dist * weld_dist (d = p_i -
 *   p_j).  At 0 that drops equal values (-0 == +0).  n_welded = the points dropped.  The kept points are K_0 .. K_(m-1), ascending.
 * 2 HULL of the kept points.  The plane of a triangle (a, b, c) is N = (b - a) x (c - a), n = N / sqrt((Nx Nx + Ny Ny) + Nz Nz),
 *   d = -((n.x a.x + n.y a.y) + n.z a.z); the distance of q is ((n.x q.x + n.y q.y) + n.z q.z) + d.
 *   START.  A = K_0.  B = the kept point with the largest squared distance from A.  C = the one with the largest |(B - A) x (q - A)|^2.
 *   D = the one with the largest |distance| from the plane of (A, B, C).  Every tie goes to the lowest index.  DEGENERATE when
 *   |B - A|^2 <= plane_tol^2, when |(B - A) x (C - A)|^2 <= plane_tol^2 |B - A|^2, or when |distance(D)| <= plane_tol (at plane_tol 0: when any of the three is zero).  With D in front of
 *   (A, B, C), B and C change places.  The four triangles are (A, B, C), (A, D, B), (B, D, C), (C, D, A), in table slots 0 .. 3.
 *   INSERTION.  Repeat: over all kept points that have not been a vertex of the table and all triangles of the table, take the largest distance;
 *   ties go to the lowest point.  Stop when it is not above plane_tol.  Otherwise that point P goes in: the triangles with distance(P) > 0
 *   are removed, the edges between a removed and a remaining triangle (the horizon, one closed walk) each give a triangle (a, b, P).
 *   The i-th edge of the walk -- it starts at the lowest removed slot's first horizon edge and runs counter-clockwise -- takes the i-th
 *   removed slot in ascending order and, past them, the two slots after the table's end; removed slots left over (a vertex all of
 *   whose triangles went has left the hull) are filled, lowest first, by the triangles from the table's end, last first.  When the loop stops, every kept point is
 *   at most plane_tol in front of every triangle.  The result does not depend on lanes, stream or batch.
 * 3 MERGE.  Every triangle starts as a class of its own.  Passes over (triangle slot t, edge k) in ascending order, for the
 *   neighbour u > t in another class, until a pass merges nothing (eight passes at most): the two classes become one when
 *   - the boundary of their union is one simple loop (no vertex twice),
 *   - every vertex of the union's triangles lies within plane_tol of the loop's plane (|distance| <= plane_tol; the plane of a loop is the
 *     one of the collision hulls above: Newell normal from the loop's smallest vertex, mid-range offset), and
 *   - every kept point lies at most 2 plane_tol in front of that plane (a small face far from a point tilts against it).
 *   A class whose boundary is not one simple loop is never formed: its triangles stay apart.
 *   FIX-UP.  A vertex left on fewer than three loops leaves the loops and the points; the plane of a face is the plane of its FINAL
 *   loop, from its smallest remaining vertex.  Repeated until nothing changes: a merged class goes back to its triangles when a
 *   vertex that leaves would leave fewer than three vertices on one of the faces it lies on, or when its final plane, rounded to
 *   float, misses one of the two BOUNDS of 5.  A hull of triangles alone passes, so this ends.
 * 4 FACES.  Each loop starts at its smallest vertex and runs counter-clockwise seen from outside; the faces come ordered by
 *   (smallest vertex, second vertex of the loop).  Inside is n.x + d <= 0.  The plane of a face is the plane of its final loop,
 *   rounded to float.  Output vertices are bit copies of input positions in ascending source index; src[k] names the input point.
 * 5 ERRORS, as for surtr_hull, from the FLOAT planes as written, evaluated in double and rounded to float: convexity = the largest
 *   distance over (EVERY INPUT POINT, welded ones included, face); planarity = the largest |distance| over the faces and their own
 *   vertices; extent = the largest edge of the box of the input points; reach = their largest coordinate magnitude.
 *   BOUNDS.  With s_f = 2^-24 ((|n_x| + |n_y| + |n_z|) reach + |d|), the rounding of a written plane: a solid is handed out only if, on
 *   the planes as written, every face's own vertices lie within plane_tol + s_f of it and every KEPT point at most 2 plane_tol + s_f in
 *   front of it (the FIX-UP below establishes this, the closing check tests it once more; a solid that misses it is FAILED).  A
 *   welded point lies within weld_dist of a kept one: convexity <= 2 plane_tol + weld_dist + s_f.
 * 6 STATUS.  SKIPPED: not selected.  NONFINITE: a coordinate is not finite (decided first).  LARGE: more than 65 535 input points, or
 *   more kept points than surtr_cook_max_vertices().  FEW: fewer than four kept points.  DEGENERATE: see START.  FAILED: the cooker's own
 *   closing check did not hold -- a triangle without area, a horizon or a class boundary that does not close, a loop of fewer than
 *   three vertices, a directed edge that does not occur exactly once with its reverse exactly once, V - E + F != 2, or a bound of 5 missed: such a solid
 *   is withheld, never handed out wrong.  OVER_255: more than 255 vertices or faces (PhysX's limit), information only.  Every bit but
 *   OVER_255 withholds the output: nv = n_faces = n_idx = max_loop = 0, the four floats 0; nv_in, status and n_welded (where the weld
 *   ran to its end) are still set.
 * Capacity bounds per written solid (Euler): points <= nv_in, polygons <= 2 nv_in - 4, indices <= 6 nv_in - 12. */
typedef struct surtr_cooked {            /* 64 bytes per solid */
    uint32_t nv_in, nv, n_faces, n_idx;     /* input points; hull vertices, polygons and indices WRITTEN for this solid */
    uint32_t status;                        /* SURTR_COOK_* bits */
    uint32_t pt_off, face_off, idx_off;     /* first point (and src entry) / polygon / index: exclusive sums over the solids before it */
    uint32_t max_loop, n_welded;
    float convexity, planarity, extent;
    float reach;                            /* the largest coordinate magnitude of the input points: the scale of a plane's rounding */
    uint32_t reserved[2];
} surtr_cooked;
enum { SURTR_COOK_SKIPPED = 1, SURTR_COOK_FEW = 2, SURTR_COOK_DEGENERATE = 4, SURTR_COOK_NONFINITE = 8, SURTR_COOK_LARGE = 16,
       SURTR_COOK_FAILED = 32, SURTR_COOK_OVER_255 = 64 };
/* The largest number of kept points the cooker takes per solid (at least 256). */
uint32_t surtr_cook_max_vertices(void);
/* The Convex of every current fragment / of every resident piece, in order.  dev_records takes one 64-byte header and one surtr_cooked
 * per solid; the header's nv_in = the solids, nv / n_faces / n_idx = the totals, status = SURTR_OK or SURTR_E_CAPACITY.  dev_points
 * (3 floats each) and dev_src (the solid-local input index of each point) have room for points_cap points, dev_polys for polys_cap
 * polygons, dev_idx for idx_cap indices (16-bit, solid-local).  Selection: with dev_hull_records_or_null -- the buffer
 * surtr_event_hulls_dev / surtr_pieces_hulls_dev wrote for the same solids, header included, on the same stream -- solid f is cooked iff
 * its hull record is not usable: a FEW / OPEN / IRREGULAR / LARGE / FLAT bit, or convexity or planarity above (float) rel_tol * extent.
 * A hull header that reports an error or another number of solids gives the header status SURTR_E_STATE and nothing else.  With NULL
 * every solid is cooked.  The rules of surtr_event_hulls_dev hold: enqueued on the context's stream, no host synchronisation, one
 * temporary allocation ordered on that stream, no profiling slot (all sixteen are taken); SURTR_E_STATE with no event or after an event
 * that failed (before any upload for the pieces); SURTR_E_CAPACITY before anything is enqueued when records_bytes cannot hold the
 * header or, where the host knows the count, the records; every other capacity is checked on the device: the header is written with
 * SURTR_E_CAPACITY and the totals needed, and nothing else is.  SURTR_E_INVALID for a tolerance that is negative or not finite. */
int surtr_event_cook_dev(surtr_ctx* ctx, const void* dev_hull_records_or_null, float rel_tol, float weld_dist, float plane_tol, void* dev_records,
                         size_t records_bytes, float* dev_points, size_t points_cap, uint32_t* dev_src, surtr_hull_polygon* dev_polys,
                         size_t polys_cap, uint16_t* dev_idx, size_t idx_cap);
int surtr_pieces_cook_dev(surtr_ctx* ctx, const void* dev_hull_records_or_null, float rel_tol, float weld_dist, float plane_tol, void* dev_records,
                          size_t records_bytes, float* dev_points, size_t points_cap, uint32_t* dev_src, surtr_hull_polygon* dev_polys,
                          size_t polys_cap, uint16_t* dev_idx, size_t idx_cap);
/* Host forms, synchronous, count-then-fill as surtr_event_hulls: with the five arrays NULL the four counts come back (records without
 * the header, points, polygons, indices); with all five given the counts must hold the capacities.  hull_records_or_null: n_hull
 * surtr_hull records in host memory (what surtr_event_hulls / surtr_pieces_hulls returned; n_hull must be the number of solids, else
 * SURTR_E_INVALID) select as above; NULL cooks every solid. */
int surtr_event_cook(surtr_ctx* ctx, const surtr_hull* hull_records_or_null, uint32_t n_hull, float rel_tol, float weld_dist, float plane_tol,
                     uint32_t* n, surtr_cooked* records, uint32_t* n_points, float* points, uint32_t* src, uint32_t* n_polys,
                     surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx);
int surtr_pieces_cook(surtr_ctx* ctx, const surtr_hull* hull_records_or_null, uint32_t n_hull, float rel_tol, float weld_dist, float plane_tol,
                      uint32_t* n, surtr_cooked* records, uint32_t* n_points, float* points, uint32_t* src, uint32_t* n_polys,
                      surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx);
/* The whole collision hand-off of the current fragments in one call: surtr_event_hulls_dev, surtr_event_cook_dev right behind it on the
 * context's stream (the selection is made on the device from the records where they lie), one read of the two headers and ONE download
 * of both answers.  Every array is given, and every count holds the capacity of its array on entry and what was written on return
 * (SURTR_E_CAPACITY and the counts when one is too small; nothing is written then).  Always enough, from surtr_event_counts: n_frag
 * records of each kind, conv_nbrs hull polygons and hull indices, conv_verts points, 2 conv_verts polygons, 6 conv_verts indices. */
int surtr_event_hulls_cook(surtr_ctx* ctx, float rel_tol, float weld_dist, float plane_tol, uint32_t* n, surtr_hull* hulls, uint32_t* n_hull_polys,
                           surtr_hull_polygon* hull_polys, uint32_t* n_hull_idx, uint16_t* hull_idx, surtr_cooked* records, uint32_t* n_points,
                           float* points, uint32_t* src, uint32_t* n_polys, surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx);
/* The same kernels on point sets in host memory: solid s has the points [vert_off[s], vert_off[s + 1]) of pos (vert_off ascending from
 * 0, n_solids + 1 entries; an empty solid is FEW).  Every solid is cooked.  For the ACH of PrepareFracture, and for point sets no
 * Convex has.  The context's event and pieces are not touched. */
int surtr_cook_points(surtr_ctx* ctx, uint32_t n_solids, const uint32_t* vert_off, const float* pos, float weld_dist, float plane_tol,
                      uint32_t* n, surtr_cooked* records, uint32_t* n_points, float* points, uint32_t* src, uint32_t* n_polys,
                      surtr_hull_polygon* polys, uint32_t* n_idx, uint16_t* idx);

/* ---- lit render buffers: the face normal on every triangle vertex (shade_dev.hip) ---- */
/* What Poly::RenderPolyhedronNormal (Inc/Poly.h:50-61, Src/Poly.cpp:619-679; VMACH::PolygonFace::Render, Src/VMACH.cpp:99-141) hands a
 * renderer: three unshared VertexNormalColor per triangle, each with the normal of its face, and running indices.  k_faces writes
 * Poly::RenderPolyhedron's buffers, whose normals are zero and which the reference's pixel shader draws unlit.
 *
 * INPUT.  The current fragments (an event's, surtr_load_fragments' or surtr_scene_fragments') after they have been triangulated:
 * SURTR_EVT_RENDER was set or surtr_event_triangulate ran.  The solid in the Mesh slot and its idx are the input, whatever
 * render_convex / is_convex was.
 * FACES.  The loops Poly::ExtractFaces yields, numbered in its order: by leading half-edge, i.e. by (start vertex, ring slot), each loop
 * from its smallest vertex -- the definition the collision hulls use.  The half-edge (a -> b) is the entry b of ring(a); its id is its
 * position in the fragment's packed rings; its successor is the entry of ring(b) listed just before a (the last one when a is first).
 * NORMAL of a loop q_0 .. q_(k-1), positions converted to double: T_i = (q_i - q_0) x (q_(i+1) - q_0), i = 1 .. k-2; N = sum T_i in
 *   double; n = N / sqrt((Nx Nx + Ny Ny) + Nz Nz) rounded to float; n = (0, 0, 0) when N.N is zero or not finite or k < 3 (drawn
 *   unlit, as the reference's shader does).  In loop order this is outward, the direction RenderPolyhedronNormal's IsCCW flip settles
 *   on.  THE ORDER OF THE SUM IS FIXED: the loop's terms lie in loop order and are added as a balanced tree -- in round d = 1, 2, 4, ...
 *   entry i with i mod 2d == 0 takes entry i + d (where there is one) -- so the bits are the same from run to run, on any stream,
 *   under any in-flight hint and beside any other work; nothing is accumulated with floating-point atomics.  Deviation, stated: the
 *   reference takes the magnitude from the loop's first three vertices, which does not hold on slivers; this is no bit-parity item.
 * FACE OF A TRIANGLE (a, b, c) of idx: the face that owns a half-edge leaving a, one leaving b and one leaving c; the lowest-numbered
 *   when several do.  Triangles are not counted per face: a face that stalled and wrote none disturbs nothing.
 * FALLBACK.  A fragment whose successor is no permutation of its half-edges (a ring lists a neighbour twice, a link lacks its way
 *   back, an entry names no vertex, the rings are not packed in vertex order) takes it as a whole and has n_faces == 0; a single
 *   triangle takes it when no face is common to its corners.  Then n = (b - a) x (c - a) in double, normalised (zero stays zero), the
 *   face number is SURTR_SHADE_NO_FACE and the fragment's record carries SURTR_SHADE_PER_TRIANGLE.
 * OUTPUT.  Vertex j is the 36-byte VertexNormalColor {position, normal, colour} of index j of the packed idx (fragment order, at the
 *   idx_off surtr_event_download reports): the position of Mesh vertex idx[j] of its fragment, the normal above, `color` (NULL: 0.25
 *   grey, as surtr_triangulate).  The index buffer is 0, 1, 2, ... and is not written.  tri_face[j / 3] (optional): the face number
 *   within the fragment.  One surtr_shaded record per fragment behind a 16-byte header of the same shape: first_vertex = the
 *   fragments, n_vertices = the vertices of all, n_faces = the faces of all, status = SURTR_OK or SURTR_E_CAPACITY.  A fragment
 *   without triangles writes nothing and has n_vertices == 0 (its faces are still counted). */
typedef struct surtr_shaded {
    uint32_t first_vertex, n_vertices;     /* = idx_off, idx_n of the fragment */
    uint32_t n_faces;                      /* loops of the fragment; 0 when it took the fallback as a whole */
    uint32_t status;                       /* SURTR_SHADE_* bits */
} surtr_shaded;
enum { SURTR_SHADE_PER_TRIANGLE = 1 };
#define SURTR_SHADE_NO_FACE 0xFFFFFFFFu
/* Into device buffers: dev_records has records_bytes bytes (16 per fragment + the header), dev_vnc room for vnc_cap vertices (36 bytes
 * each), dev_tri_face (may be NULL, then tri_cap must be 0) for tri_cap triangles.  Enqueued on the context's stream with no host
 * synchronisation; one temporary device allocation ordered on that stream; no profiling slot (all sixteen of surtr_kernel_times are
 * taken).  SURTR_E_STATE with no current fragments, after an event that failed, or when they were never triangulated.
 * SURTR_E_CAPACITY before anything is enqueued where the host holds the event's counts (surtr_counts::n_idx vertices, n_idx / 3
 * triangles and n_frag + 1 records always suffice); where only the device knows them, the header is written with SURTR_E_CAPACITY and
 * the totals needed, and nothing else is.  SURTR_E_INVALID for a NULL context or record buffer, or an array that is NULL with a
 * capacity (or the reverse).  On any error the context and the current fragments are unchanged; the call never changes them. */
int surtr_event_shaded_dev(surtr_ctx* ctx, const float color[3], void* dev_records, size_t records_bytes, float* dev_vnc, size_t vnc_cap,
                           uint32_t* dev_tri_face, size_t tri_cap);
/* Host form, synchronous, count-then-fill as surtr_event_hulls: with records and vnc NULL, *n, *n_vertices and *n_faces come back
 * (fragments, vertices, faces of all); with both given *n and *n_vertices must hold their capacities (SURTR_E_CAPACITY and the counts
 * when one is too small, nothing written); tri_face (may be NULL) has room for *n_vertices / 3 entries.  One of records / vnc without
 * the other, or tri_face without them, is SURTR_E_INVALID. */
int surtr_event_shaded(surtr_ctx* ctx, const float color[3], uint32_t* n, surtr_shaded* records, uint32_t* n_vertices, float* vnc,
                       uint32_t* tri_face, uint32_t* n_faces);
/* Diagnostic, for tests: fragments of up to `half_edges` half-edges keep their topology and partial sums in LDS, larger ones in global
 * scratch.  0: the built-in limit, which is also the largest value taken.  The result does not depend on it. */
int surtr_set_shade_tier(surtr_ctx* ctx, uint32_t half_edges);

#ifdef __cplusplus
}
#endif
#endif /* SURTR_HIP_H */
