"""The event's capacity limits: exact fit, one short, nothing written past a device buffer.

Two public calls shrink buffers under the event's kernels: set_arena (result vertices, ring entries, triangle indices, handed out
with atomicAdd on CUR_V / CUR_H / CUR_I by every clipper's park and by k_faces) and set_scratch (CV, CH of the Mesh clip's
per-workgroup global scratch: clip_global and the literal clipper).  What they promise (include/surtr_hip.h, next to the two
calls): ANY capacity gives either the
exact event or SURTR_E_CAPACITY, and nothing is written past it.  tests/test_alloc_failures.py is the twin of this module for
allocations that fail.

CPU TIER, on the emulation (tests/emul/hip_emul.h), whose hipMalloc puts a red zone before and after every device block
(surtr_emul_guard_check) and whose launches can run their blocks last to first (surtr_emul_block_order): forward, block 0 takes
every ticket; reversed, block grid - 1 does, on another scratch slice.  WHAT THE ZONES SEE: writes past a buffer that is one
device block -- the arena's arrays, the tables, the blobs -- which is what the ARENA cases are about.  WHAT THEY DO NOT SEE: a
write past the end of a scratch SLICE or of one of its 256-byte-rounded arrays.  Every pool holds more slices than a launch has
blocks (the Mesh clip's: max_wg + n_wg_big + 32 catcher slices against min(pairs, max_wg) blocks), so in either order the working
slice is followed by another slice, never by the pool's zone.  In the SCRATCH, THRESHOLD and LITERAL cases `damaged() == 0` therefore
says nothing about the slices; there an overrun shows only as a changed event (every rung is compared bit for bit) and at the
threshold probe, which is what refused the clip_global mutation below.  ONE case puts the working slice at the pool's end, with
no padding before the zone: scratch-torus40-last (scratch_case, last_slice).  Tried by hand: clip_global storing one word at
t_ring[CH], the first word past its slice, is refused there ('a red zone is damaged', (3072, 27648)) and by no other scratch
case.  That covers the END of a slice on the catcher's route; an overrun of an array inside a slice stays invisible to the zones.
Every case runs in a child process under a time limit.

  ARENA, per case of ARENA_CASES (scene x route; the device counters must show that the route took work), forward and reversed:
   (a) two automatic runs leave the same marks (queue_stats()[0:3]) and the same bits: no route takes speculatively;
   (b) the marks are not below what the oracle's event holds (mesh + conv vertices, ring entries, n_idx), the I mark equals the
       oracle's n_idx (no face stalls in these scenes), and an arena one short of the ORACLE's totals in one capacity (the others
       automatic) is refused -- a bound that does not come from the engine;
   (c) an arena of exactly the marks gives the automatic run's bits, which are the oracle's event (assert_event_equal);
   (d) the marks with one entry lowered by one give SURTR_E_CAPACITY;
   (e) so does every rung of a ladder below: the value 1, and for each stage's share [a, b) of the cursor the rungs a - 1, a and
       (a + b) / 2.  The stages are Convex clip, Mesh clip, refit (V and H) and faces (I); their shares come from the counts and
       marks of automatic runs with flags 0 and with the case's flags (the Convex clip's share is the flags-0 mark less the
       Meshes).  The emulation runs the stages in that order, so the stage that fails first on a rung is known in advance, and
       what the refused event leaves behind must say the same: a failed pair without a Convex (its cost is the bare 8) -> the
       Convex clip; failed pairs, all with their Convex -> the Mesh clip; no failed pair and the I mark within its capacity -> the
       refit; no failed pair and the I mark beyond -> the faces.  (frag_status travels with download(), which a refused event
       rightly does not give: the pairs' records and the marks are the evidence.)  Every stage fails first on some rung;
   (f) after every refusal event_counts() and download() raise SURTR_E_CAPACITY, pack_dev writes the zero-count header with the
       status and nothing behind it, no red zone is damaged; after set_arena(0, 0, 0) the same engine gives the same bits again;
       after close() the live allocations are back where they were.
  ENTRIES that size the arena themselves (load_fragments + event_refit, scene_fragments): the same bits under set_arena(1, 1, 1)
  as without, nothing damaged.  One scene_fracture_event at the boundary: exact fit, one short refused with the resident scene
  unchanged (tests/test_scene.py's snapshot) and the commit refused, recovery.
  SCRATCH on libsurtr_emul_small.so (every band leaves the tiny LDS topology for clip_global), blocks reversed: the ladder of
  (CV, CH) from (2 vmax, 3 hmax) down to (1, 1); every rung is the automatic run's bits or SURTR_E_CAPACITY (never another event,
  never a topology flag), monotone, some rung below (vmax, hmax) succeeds and some fails (the one that fails proves that
  clip_global ran: its SURTR_OVERFLOW is the only source of that code there); set_scratch(0, 0) recovers.  (The zones are checked
  after every rung, for the arena and the tables; for the scratch slices themselves see WHAT THEY DO NOT SEE above.)
  LITERAL clipper: tests/golden/degenerate_sliver_convex.npz with a scratch of (64, 64), too small for LIT_STRIDE rings of its
  four vertices: the pair is flagged (SURTR_E_TOPOLOGY, n_failed 1), queue_stats()[90] counts it, and the automatic scratch gives
  the unflagged event again.

  THRESHOLD of the scratch: see scratch_threshold_case (a pair that needs 64 k + 1 slots, probed at CV = 64 k).

MUTATIONS, each tried by hand on a copy of the sources (never committed, never run on a GPU), every CPU case of this module run
against it, and the assertion that refused it:
  * arena_take with `<` for `<=` on V (surtr_hip.hip): where arena_take makes the event's last take -- the cube's cases, the render-only
    cases, refit12-blob, islands-urchin, scene-event -- (c): the event under an arena of exactly the marks raised SURTR_E_CAPACITY;
    where sc_park makes the last take (blob and torus with the limit-4 refit, on every build), (e): "stage that failed first",
    V rung = end of the Mesh clip's share (blob 4143, torus 3164): 'mesh' where the refit had to be the first to fail.
  * wc_park's comparison without `+ H` (wave_clip.h): the red zones, ('a red zone is damaged', [V, 510, I]) on the H rung in the
    Mesh clip's share in every case whose pairs the record clipper parks (default-, rec-, refit12-, tier2- blob and torus;
    islands-urchin already at (b)): the rings went past the 510-entry ring buffer.  Two children died of it (exit 139 / 134).
  * k_faces' direct take reserving one triangle fewer than it writes (both the atomicAdd and its comparison): assert_event_equal,
    'idx', in every arena case and in scene-event, before (b) came to compare the I mark with the oracle's n_idx.
  * clip_global with T.capV = S.CV + 1 (surtr_hip.hip): NOT refused by the ladders, the red zones or the block order (every array
    of a scratch slice is rounded up to 256 bytes: one slot past CV is padding; and no zone borders a slice).  scratch_threshold_case was added for it and
    refuses it: ('another event', pair 10, CV 640).
  * write_solid writing one vertex past the last (clip_core.h): the red zones: "(c) a red zone is damaged after the exact fit"
    (default-cube-refit, refit12-blob, islands-urchin, scene-event) and ('a red zone is damaged', caps) on the V rung at the end
    of the Mesh clip's share (small-blob, small-torus); the record clipper's cases park through wc_park and do not run it last.

GPU TIER (gpu mark, one child process per case through helpers.run_gpu_child): the arena boundary -- (a), (c), (d) and of (f)
the raising calls, the header-only blob (pack_dev into a torch buffer: k_pack's path for a refused event, on the device) and
the recovery -- on cube, blob_scene(64) and the 48 x 32 torus with 12 cells, and the scratch rungs automatic, (vmax, hmax),
halves and eighths on a 200 x 120 torus cut by 2 cells, whose bands (about 12 000 vertices) cannot stay in LDS; the record clipper
is switched off for that case (SURTR_REC=0) so that the bands go to the general clipper.  Nothing below one short is run there.
MEASURED_GPU_SECONDS holds each case's first run (0.7 .. 0.8 s for the arena cases, 2.7 s for the scratch case, python start, scene
and oracle included); the time limit is four times that, 60 s at the least.  On the device the scratch rungs gave: automatic and
(24 000, 144 000) the same bits, (12 000, 72 000) and (3 000, 18 000) SURTR_E_CAPACITY.
"""
import ctypes
import os
import subprocess
import sys
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.join(ROOT, "tests")
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from helpers import assert_event_equal, fragment, run_gpu_child      # noqa: E402
from surtr_amd import engine, meshgen, scenes      # noqa: E402

CAP = engine.E_CAPACITY
CHILD_SECONDS = 120      # (a case takes 1 .. 4 s: the limit is for a kernel that does not end)


# ------------------------------------------------------------------ scenes and routes
SCENES = {
    "cube": lambda: scenes.cube_scene(8),
    "blob": lambda: scenes.blob_scene(12),
    "torus": lambda: scenes.make_scene(*meshgen.bumpy_torus(48, 32), 12),
    "urchin": lambda: scenes.make_scene(*meshgen.urchin(), 64),      # (tests/test_clip_definition.py's island scene)
    "blob64": lambda: scenes.blob_scene(64),
    "torus40": lambda: scenes.make_scene(*meshgen.bumpy_torus(48, 32), 40),      # (32 pairs or more: every catcher workgroup is launched)
}


def _route_default(qs, c, n, ev):
    # (a weak check: it says that the plan's usual kernels took the pairs, not which clipper parked each; the cases below name theirs)
    assert qs[80] + qs[81] == n, qs[80:82].tolist()                     # every Convex went through k_clip_convex's chain
    queued = int(qs[16:32].sum())                                       # pairs the pre-pass queued for the Mesh clip kernels
    assert queued in (0, n) and (queued == 0 or qs[88] + qs[94] > 0), (queued, qs[88], qs[94])      # ... and who clipped them


def _route_small(qs, c, n, ev):
    assert qs[84] > 0 or qs[16 + 14] + qs[16 + 15] > 0, qs[16:32].tolist()      # bands beyond the tiny LDS topology: clip_global


def _route_rec(qs, c, n, ev):
    assert qs[88] > 0 and qs[89] > 0, qs[88:90].tolist()                # CUR_REC_TOOK, CUR_REC_HANDED: parked by wc_park, and handed on


def _route_islands(qs, c, n, ev):
    assert qs[3] == c.n_frag, (qs[3], c.n_frag)                         # CUR_ISL: one island record per fragment ...
    assert len(set(map(tuple, ev["frag_ids"][:, :2].tolist()))) < c.n_frag and ev["frag_ids"][:, 2].max() >= 1      # ... several to a pair


def _route_tier(qs, c, n, ev):
    assert qs[85] > 0, qs[85:87].tolist()                               # CUR_FACES2_N: fragments pushed to the second tier of k_faces


def _route_refit_n(qs, c, n, ev):
    # k_refit and k_refit_n move these counters alike: they show that every fragment was refitted, not by which kernel.  That it was
    # k_refit_n is shown by get_refit_point_limit() == 12 (arena_case), which alone selects it in launch_refit, by marks above the
    # limit-4 run's, and by the Convexes being oracle.refit's at 12 (oracle_reference), which k_refit's four-point hull does not give.
    assert qs[82] + qs[83] == c.n_frag and qs[95] == 0, (qs[82:84].tolist(), qs[95])      # every fragment refitted, none given up


# id: (emulation library, environment, scene, flags, RefittingPointLimit, route check)
ARENA_CASES = {
    "default-cube-render": ("libsurtr_emul.so", {}, "cube", 2, 4, _route_default),
    "default-cube-refit": ("libsurtr_emul.so", {}, "cube", 3, 4, _route_default),
    "default-blob-render": ("libsurtr_emul.so", {}, "blob", 2, 4, _route_default),
    "default-blob-refit": ("libsurtr_emul.so", {}, "blob", 3, 4, _route_default),
    "default-torus-render": ("libsurtr_emul.so", {}, "torus", 2, 4, _route_default),
    "default-torus-refit": ("libsurtr_emul.so", {}, "torus", 3, 4, _route_default),
    "refit12-blob": ("libsurtr_emul.so", {}, "blob", 3, 12, _route_refit_n),
    "small-blob": ("libsurtr_emul_small.so", {}, "blob", 3, 4, _route_small),
    "small-torus": ("libsurtr_emul_small.so", {}, "torus", 3, 4, _route_small),
    "rec-torus": ("libsurtr_emul_rec.so", {}, "torus", 3, 4, _route_rec),
    "rec-blob": ("libsurtr_emul_rec.so", {}, "blob", 3, 4, _route_rec),
    "islands-urchin": ("libsurtr_emul.so", {}, "urchin", 3, 4, _route_islands),
    "tier2-blob": ("libsurtr_emul.so", {"SURTR_FACES_TIER_HE": "64"}, "blob", 3, 4, _route_tier),
}
OTHER_CASES = {
    "entries": ("libsurtr_emul.so", {}),
    "scene-event": ("libsurtr_emul.so", {}),
    "scratch-blob": ("libsurtr_emul_small.so", {}),
    "scratch-torus": ("libsurtr_emul_small.so", {}),
    "scratch-threshold": ("libsurtr_emul_small.so", {}),
    "scratch-torus40-last": ("libsurtr_emul_small.so", {"SURTR_BIG_QUOTA": "0"}),
    "literal": ("libsurtr_emul.so", {}),
}


# ------------------------------------------------------------------ the emulation's hooks
class Emul:
    def blob(self, nbytes):
        return HostBlob(nbytes)

    def __init__(self, path):
        engine._use_library_for_tests(path)
        self.L = ctypes.CDLL(path)
        for f in ("surtr_emul_live_allocs", "surtr_emul_guard_check"):
            getattr(self.L, f).restype = ctypes.c_long
        self.L.surtr_emul_block_order.argtypes = [ctypes.c_int]

    def live(self):
        return self.L.surtr_emul_live_allocs()

    def damaged(self):
        return self.L.surtr_emul_guard_check()

    def order(self, reverse):
        self.L.surtr_emul_block_order(int(reverse))


class HostBlob:
    """A buffer for pack_dev: host memory is device memory in the emulation."""
    def __init__(self, nbytes):
        self.a = np.zeros(nbytes, np.uint8)

    def fill(self, byte):
        self.a[:] = byte
        return self.a.ctypes.data, self.a.nbytes

    def host(self):
        return self.a


class TorchBlob:
    def __init__(self, nbytes):
        import torch
        self.torch, self.a = torch, torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")

    def fill(self, byte):
        self.a.fill_(byte)
        self.torch.cuda.synchronize()
        return self.a.data_ptr(), self.a.numel()

    def host(self):
        self.torch.cuda.synchronize()      # (pack_dev is enqueued on the context's stream, the default one here)
        return self.a.cpu().numpy()


class Device:
    """The hooks' stand-in on the GPU: no red zones, the hardware's own block order."""
    blob = TorchBlob

    def live(self):
        return 0

    def damaged(self):
        return 0

    def order(self, reverse):
        pass


def same_bits(a, b):
    return a.keys() == b.keys() and all(a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a)


def setup(eng, sc, limit=4):
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.set_refit_point_limit(limit)


def raises(code, call):
    try:
        call()
    except engine.SurtrError as e:
        assert e.code == code, (e.code, code, str(e))
        return
    raise AssertionError("not refused (SURTR error %d expected)" % code)


def oracle_reference(sc, flags, limit):
    """The oracle's event with the case's flags; at a RefittingPointLimit above 4 its un-refitted event with every Convex refitted
    by oracle.refit (the oracle's event refits at 4 only)."""
    from oracle import oracle as O
    planes = O.place_cells(sc["v012"], sc["scale"], sc["translate"])
    ev = O.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=bool(flags & 1) and limit == 4, render=bool(flags & 2), threads=4)
    if flags & 1 and limit != 4:
        conv = [O.refit(fragment(ev, k, "conv"), fragment(ev, k, "mesh"), limit) for k in range(ev["frag_ids"].shape[0])]
        nv = [c["pos"].shape[0] for c in conv]
        ev["conv_vert_off"] = np.cumsum([0] + nv).astype(np.uint32)
        ev["conv_pos"] = np.concatenate([c["pos"].reshape(-1, 3) for c in conv]).astype(np.float32)
        base = np.cumsum([0] + [int(c["off"][-1]) for c in conv])
        ev["conv_nbr_off"] = np.concatenate([c["off"][:-1].astype(np.int64) + base[k] for k, c in enumerate(conv)] + [base[-1:]]).astype(np.uint32)
        ev["conv_nbr"] = np.concatenate([c["nbr"] for c in conv]).astype(np.int32)
    return ev


def oracle_needs(ref, flags):
    return (ref["mesh_pos"].shape[0] + ref["conv_pos"].shape[0], ref["mesh_nbr"].shape[0] + ref["conv_nbr"].shape[0],
            ref["idx"].shape[0] if flags & 2 else 0)


# ------------------------------------------------------------------ the arena
def first_failed_stage(eng, n, caps):
    """What a refused event left behind -> the stage that failed first (module docstring, (e))."""
    ps, cost, left = eng.pair_status(n), eng.pair_costs(n), eng.queue_stats()[0:3]
    assert set(np.unique(ps).tolist()) <= {0, CAP}, np.unique(ps)
    if (ps == CAP).any():
        return "convex" if ((ps == CAP) & (cost == 8)).any() else "mesh"
    if caps[2] and left[2] > caps[2]:
        return "faces"
    assert any(c and m > c for m, c in zip(left[:2].tolist(), caps[:2])), (left.tolist(), caps)
    return "refit"


def refused(em, eng, n, flags, caps, blob):
    """(d), (e), (f): the event under set_arena(*caps) is refused, cleanly.  -> the stage that failed first."""
    eng.set_arena(*caps)
    raises(CAP, lambda: eng.fracture_event(0, n, flags=flags))
    raises(CAP, eng.event_counts)
    raises(CAP, eng.download)
    eng.pack_dev(*blob.fill(0xAB))
    got = blob.host()
    hdr = got[:36].view(np.uint32)
    assert hdr[:6].tolist() == [0] * 6 and hdr[6] == n and hdr[7] == CAP and hdr[8] == 0, ("blob header of a refused event", hdr.tolist())
    assert (got[36:] == 0xAB).all(), "pack_dev wrote behind the header of a refused event"
    assert em.damaged() == 0, ("a red zone is damaged", caps)
    return first_failed_stage(eng, n, caps)


def ladder_rungs(bounds):
    """bounds: the cursor's value at the end of each stage, [0, b1, ..., full] -> {rung: index of the stage that fails first}."""
    full, out = bounds[-1], {}
    for s in range(len(bounds) - 1):
        a, b = bounds[s], bounds[s + 1]
        if b > a:
            for r in (a - 1, a, (a + b) // 2, b - 1):
                if 1 <= r < full:
                    out[r] = max(t for t in range(len(bounds) - 1) if bounds[t] <= r)
    out[1] = max(t for t in range(len(bounds) - 1) if bounds[t] <= 1)
    return out


def arena_case(em, sc, flags, limit, route, ref, ladders=True):
    n = sc["n_cells"]
    live0 = em.live()
    need = oracle_needs(ref, flags)
    forward = None
    for reverse in (0, 1):
        em.order(reverse)
        eng = engine.Engine(0)
        setup(eng, sc, limit)
        assert eng.get_refit_point_limit() == limit      # (above 4: k_refit_n)
        c0 = eng.fracture_event(0, n, flags=0)
        m0 = eng.queue_stats()[0:3].tolist()
        # (a)
        c = eng.fracture_event(0, n, flags=flags)
        qs = eng.queue_stats()
        marks = qs[0:3].tolist()
        auto = eng.download()
        route(qs, c, n, auto)
        assert c.status == 0 and c.n_failed == 0 and not auto["frag_status"].any()
        eng.fracture_event(0, n, flags=flags)
        assert eng.queue_stats()[0:3].tolist() == marks, ("(a) marks differ between two automatic runs", marks, eng.queue_stats()[0:3].tolist())
        assert same_bits(eng.download(), auto), "(a) two automatic runs differ"
        if forward is None:
            forward = (marks, auto)
            assert_event_equal(auto, ref, render=bool(flags & 2))
        else:
            assert marks == forward[0] and same_bits(auto, forward[1]), "block order: reversed differs from forward"
        print("marks", marks, "oracle needs", need, "flags-0 marks", m0, "flags-0 meshes", (c0.mesh_verts, c0.mesh_nbrs))
        # (b)
        assert all(m >= w for m, w in zip(marks, need)), ("(b) marks below the oracle's totals", marks, need)
        assert marks[2] == need[2], ("(b) I mark is not the oracle's n_idx", marks[2], need[2])
        blob = em.blob(engine.blob_bytes(c) + 64)
        for k in range(3):
            if ladders and need[k] >= 2:
                caps = [0, 0, 0]; caps[k] = need[k] - 1
                refused(em, eng, n, flags, caps, blob)
        # (c)
        eng.set_arena(*marks)
        eng.fracture_event(0, n, flags=flags)
        assert eng.queue_stats()[0:3].tolist() == marks
        assert same_bits(eng.download(), auto), "(c) an arena of exactly the marks gives another event"
        assert em.damaged() == 0, "(c) a red zone is damaged after the exact fit"
        # (d)
        stages = set()
        for k in range(3):
            if marks[k] >= 2:
                caps = list(marks); caps[k] -= 1
                stages.add(refused(em, eng, n, flags, caps, blob))
        # (e)
        if ladders:
            names = ["convex", "mesh"] + (["refit"] if flags & 1 else [])
            for k in range(2):
                bounds = [0, m0[k] - (c0.mesh_verts, c0.mesh_nbrs)[k], m0[k]] + ([marks[k]] if flags & 1 else [])
                assert bounds == sorted(bounds) and bounds[-1] == marks[k], bounds
                for r, s in sorted(ladder_rungs(bounds).items()):
                    caps = list(marks); caps[k] = r
                    got = refused(em, eng, n, flags, caps, blob)
                    assert got == names[s], ("(e) stage that failed first", "VH"[k], r, bounds, got, names[s])
                    stages.add(got)
            if flags & 2:
                for r in sorted({1, marks[2] // 4, marks[2] // 2, 3 * marks[2] // 4, marks[2] - 2}):
                    if 1 <= r < marks[2]:
                        got = refused(em, eng, n, flags, [marks[0], marks[1], r], blob)
                        assert got == "faces", ("(e) stage that failed first", "I", r, got)
                        stages.add(got)
            want = set(names) | ({"faces"} if flags & 2 else set())
            assert stages == want, ("(e) stages that failed first on some rung", stages, want)
        # (f)
        eng.set_arena(0, 0, 0)
        eng.fracture_event(0, n, flags=flags)
        assert same_bits(eng.download(), auto), "(f) the engine does not recover after set_arena(0, 0, 0)"
        eng.close()
        assert em.damaged() == 0 and em.live() == live0, ("(f) after close", em.damaged(), em.live(), live0)
    em.order(0)


# ------------------------------------------------------------------ entries that size the arena themselves
def entries_case(em):
    from oracle import oracle as O
    sc = SCENES["blob"]()
    n = sc["n_cells"]
    planes = O.place_cells(sc["v012"], sc["scale"], sc["translate"])
    ref = O.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=True, render=False, threads=4)
    live0, forward = em.live(), {}
    for reverse in (0, 1):
        em.order(reverse)
        eng = engine.Engine(0)
        setup(eng, sc)
        eng.fracture_event(0, n, flags=0)
        ev0 = eng.download()
        meshes, convexes = scenes.fragments_as_pieces(ev0)
        got = []
        for arena in ((0, 0, 0), (1, 1, 1)):
            eng.set_arena(*arena)
            eng.load_fragments(meshes, convexes, ev0["frag_ids"])
            eng.event_refit()
            c = eng.event_counts()
            assert c.status == 0 and c.n_failed == 0
            got.append(eng.download())
            assert em.damaged() == 0, ("load_fragments + event_refit", arena)
        assert same_bits(got[0], got[1]), "load_fragments + event_refit under set_arena(1, 1, 1)"
        assert_event_equal(got[0], ref, render=False)
        forward.setdefault("refit", got[0])
        assert same_bits(got[0], forward["refit"]), "block order: load_fragments + event_refit reversed differs from forward"
        eng.close()
        # scene_fragments over three resident bodies
        from test_scene import three_bodies
        eng, _ = three_bodies(engine)
        got = []
        for arena in ((0, 0, 0), (1, 1, 1)):
            eng.set_arena(*arena)
            c = eng.scene_fragments()
            assert c.status == 0 and c.n_frag == 3 and c.n_idx > 0
            got.append(eng.download())
            assert em.damaged() == 0, ("scene_fragments", arena)
        assert same_bits(got[0], got[1]), "scene_fragments under set_arena(1, 1, 1)"
        forward.setdefault("scene", got[0])
        assert same_bits(got[0], forward["scene"]), "block order: scene_fragments reversed differs from forward"
        eng.close()
        assert em.live() == live0
    em.order(0)


def scene_event_case(em):
    from test_scene import SHIFT_B, assert_unchanged, bodies, snapshot, three_bodies
    live0, forward = em.live(), {}
    for reverse in (0, 1):
        em.order(reverse)
        eng, _ = three_bodies(engine)
        cube = bodies(engine)["cube"]
        eng.upload_pattern(cube["face_off"], cube["v012"])
        eng.place_cells(cube["scale"], (cube["translate"] + SHIFT_B).astype(np.float32))
        before = snapshot(eng)
        c = eng.scene_fracture_event(1, 0, 8, flags=3)
        marks = eng.queue_stats()[0:3].tolist()
        auto = eng.download()
        assert c.status == 0 and c.n_frag == 8 and marks[2] == c.n_idx
        forward.setdefault("event", (marks, auto))
        assert marks == forward["event"][0] and same_bits(auto, forward["event"][1]), "block order: scene event reversed differs from forward"
        co, cp = eng.event_regroup()
        eng.set_arena(*marks)
        eng.scene_fracture_event(1, 0, 8, flags=3)
        assert same_bits(eng.download(), auto) and em.damaged() == 0, "scene event, exact fit"
        for k in range(3):
            caps = list(marks); caps[k] -= 1
            eng.set_arena(*caps)
            raises(CAP, lambda: eng.scene_fracture_event(1, 0, 8, flags=3))
            raises(CAP, eng.download)
            assert em.damaged() == 0, ("scene event, one short", caps)
            assert_unchanged(eng, before)
            raises(engine.E_STATE, lambda: eng.scene_commit(co, cp))
            assert_unchanged(eng, before)
        eng.set_arena(0, 0, 0)
        eng.scene_fracture_event(1, 0, 8, flags=3)
        assert same_bits(eng.download(), auto)
        co, cp = eng.event_regroup()
        assert eng.scene_commit(co, cp)[0] == 10
        eng.close()
        assert em.damaged() == 0 and em.live() == live0
    em.order(0)


# ------------------------------------------------------------------ the scratch
def scratch_rungs(v, h, short=False):
    if short:
        return [(0, 0), (v, h), (v // 2, h // 2), (v // 8, h // 8)]
    return ([(2 * v, 3 * h), (v, h)] + [(v // d, h // d) for d in (2, 3, 4, 8)] + [(v // d, h) for d in (2, 3, 4, 8)] +
            [(v, h // d) for d in (2, 3, 4, 8)] + [(64, 256), (64, 64), (1, 1)])


def scratch_case(em, sc, rungs, flags=3, last_slice=False):
    """last_slice: the case where the working slice IS the pool's last one.  The Mesh clip's pool is max_wg + n_wg_big + 32 slices
    (launch_event), the last 32 being k_clip_pairs_catch's, whose grid is min(32, pairs).  With SURTR_BIG_QUOTA=0 on the small-LDS
    build every band is queued in class 13, the catcher's own; with 32 pairs or more and the blocks reversed its block 31 runs
    first and takes every ticket, on slice max_wg + n_wg_big + 31.  The slice's last array is t_ring (CH words): where 4 CH is a
    multiple of 256 it ends at the pool's red zone with no padding between.  The counters must show that the catcher clipped
    every queued pair."""
    n = sc["n_cells"]
    v, h = sc["mesh"]["pos"].shape[0], int(sc["mesh"]["off"][-1])
    live0 = em.live()
    em.order(1)
    eng = engine.Engine(0)
    setup(eng, sc)
    c = eng.fracture_event(0, n, flags=flags)
    auto = eng.download()
    assert c.status == 0 and c.n_failed == 0
    if last_slice:
        qs = eng.queue_stats()
        assert n >= 32 and qs[16 + 13] > 0 and qs[16:32].sum() == qs[16 + 13] == qs[94], (n, qs[16:32].tolist(), qs[94])
        assert all((4 * ch) % 256 == 0 for _, ch in rungs if ch >= 64), rungs
    outcome = {}
    for cv, ch in rungs:
        eng.set_scratch(cv, ch)
        t = time.time()
        try:
            c = eng.fracture_event(0, n, flags=flags)
        except engine.SurtrError as e:
            assert e.code == CAP, ((cv, ch), e.code, str(e))
            ps = eng.pair_status(n)
            assert set(np.unique(ps).tolist()) <= {0, CAP} and (ps == CAP).any(), ((cv, ch), np.unique(ps))
            raises(CAP, eng.download)
            outcome[(cv, ch)] = False
        else:
            got = eng.download()
            assert c.status == 0 and c.n_failed == 0 and not got["frag_status"].any(), ((cv, ch), "a topology flag")
            assert same_bits(got, auto), ((cv, ch), "another event")
            outcome[(cv, ch)] = True
        print("scratch", (cv, ch), "ok" if outcome[(cv, ch)] else "refused", "%.2f s" % (time.time() - t))
        assert em.damaged() == 0, ("a red zone is damaged", (cv, ch))
    real = {k: o for k, o in outcome.items() if k != (0, 0)}
    for (a, b), ok in real.items():
        if ok:
            assert all(o for (p, q), o in real.items() if p >= a and q >= b), ("not monotone", (a, b), outcome)
    eng.set_scratch(0, 0)
    eng.fracture_event(0, n, flags=flags)
    assert same_bits(eng.download(), auto), "the engine does not recover after set_scratch(0, 0)"
    eng.close()
    assert em.damaged() == 0 and em.live() == live0
    em.order(0)
    return outcome


def scratch_threshold_case(em):
    """The smallest CV (CH automatic) at which each pair of the 40 x 24 torus x 12 cells still succeeds, by bisection, blocks
    reversed; every probe is the automatic run's bits or SURTR_E_CAPACITY.  The slices of the scratch pool round every array up to
    256 bytes, so a slot one past CV lands in padding and changes nothing -- unless CV is a multiple of 64, where it is slot 0 of
    the next array.  The scene is chosen so that one pair needs 64 k + 1 slots (pair 10: 641): with CV = 640 a clipper that takes
    one slot too many writes into live data there, and the event is no longer the automatic one."""
    sc = scenes.make_scene(*meshgen.bumpy_torus(40, 24), 12)
    v = sc["mesh"]["pos"].shape[0]
    em.order(1)
    eng = engine.Engine(0)
    setup(eng, sc)
    needs = []
    for p in range(sc["n_cells"]):
        eng.set_scratch(0, 0)
        c = eng.fracture_pairs([p], [0], flags=3)
        auto = eng.download()
        assert c.status == 0 and c.n_failed == 0

        def fits(cv):
            eng.set_scratch(cv, 0)
            try:
                c = eng.fracture_pairs([p], [0], flags=3)
            except engine.SurtrError as e:
                assert e.code == CAP, (p, cv, e.code, str(e))
                assert em.damaged() == 0, ("a red zone is damaged", p, cv)
                return False
            assert c.status == 0 and c.n_failed == 0 and same_bits(eng.download(), auto), ("another event", p, cv)
            assert em.damaged() == 0, ("a red zone is damaged", p, cv)
            return True
        lo, hi = 64, 2 * v + 4096      # (64 is the floor of CV; the automatic capacity is 2 vmax + 4096)
        assert fits(hi)
        if fits(lo):
            needs.append(lo)
            continue
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (lo, mid) if fits(mid) else (mid, hi)
        assert fits(hi) and not fits(hi - 1)
        needs.append(hi)
    print("slots needed per pair", needs)
    assert any(t % 64 == 1 for t in needs), ("no pair needs 64 k + 1 slots any more: choose a scene that has one (docstring)", needs)
    eng.close()
    assert em.damaged() == 0
    em.order(0)


def literal_case(em):
    d = np.load(os.path.join(HERE, "golden", "degenerate_sliver_convex.npz"))
    mesh = {"pos": d["mesh_pos"], "off": d["mesh_off"], "nbr": d["mesh_nbr"]}
    conv = {"pos": d["conv_pos"], "off": d["conv_off"], "nbr": d["conv_nbr"]}
    planes = np.asarray(d["planes"], np.float32).reshape(-1, 4)
    fo = np.uint32([0, planes.shape[0]])
    for reverse in (0, 1):
        em.order(reverse)
        eng = engine.Engine(0)
        eng.upload_pieces([mesh], [conv])
        eng.upload_planes(fo, planes)
        c = eng.fracture_event(0, 1, flags=3)
        assert (c.status, c.n_frag, c.n_failed) == (0, 0, 0) and eng.queue_stats()[90] == 0      # the literal clipper answers: nothing is left
        eng.set_scratch(64, 64)
        c = eng.fracture_event(0, 1, flags=3)
        assert (c.status, c.n_frag, c.n_failed) == (0, 0, 1), (c.status, c.n_frag, c.n_failed)
        assert eng.pair_status(1).tolist() == [engine.E_TOPOLOGY] and eng.queue_stats()[90] == 1
        assert em.damaged() == 0
        eng.set_scratch(0, 0)
        c = eng.fracture_event(0, 1, flags=3)
        assert (c.status, c.n_frag, c.n_failed) == (0, 0, 0) and eng.queue_stats()[90] == 0
        eng.close()
        assert em.damaged() == 0
    em.order(0)


# ------------------------------------------------------------------ the children
def run_child(case, lib_dir):
    if case in ARENA_CASES:
        lib, _, scene, flags, limit, route = ARENA_CASES[case]
        em = Emul(os.path.join(lib_dir, lib))
        sc = SCENES[scene]()
        arena_case(em, sc, flags, limit, route, oracle_reference(sc, flags, limit))
    else:
        em = Emul(os.path.join(lib_dir, OTHER_CASES[case][0]))
        if case == "entries":
            entries_case(em)
        elif case == "scene-event":
            scene_event_case(em)
        elif case == "literal":
            literal_case(em)
        elif case == "scratch-threshold":
            scratch_threshold_case(em)
        else:
            sc = SCENES[case.split("-")[1]]()
            v, h = sc["mesh"]["pos"].shape[0], int(sc["mesh"]["off"][-1])
            outcome = scratch_case(em, sc, scratch_rungs(v, h), last_slice=case == "scratch-torus40-last")
            below = [ok for (a, b), ok in outcome.items() if a <= v and b <= h and (a, b) != (v, h)]
            assert any(below) and not all(below), ("below (vmax, hmax): some rung succeeds and some is refused", outcome)
    assert em.damaged() == 0
    print("ok " + case)


def _child(case, emul_lib_path, env_extra):
    env = dict(os.environ)
    for k in ("SURTR_FACES_TIER_HE", "SURTR_WAVE", "SURTR_REC", "SURTR_SPLIT", "SURTR_HALF", "SURTR_FRONT_PAR", "SURTR_CVX_LEAN", "SURTR_BIG_QUOTA"):
        env.pop(k, None)
    env.update(env_extra)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), case, os.path.dirname(emul_lib_path)], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=CHILD_SECONDS)
    except subprocess.TimeoutExpired:
        raise AssertionError("%s did not end within %d s" % (case, CHILD_SECONDS))
    out = "\n".join(l for l in (r.stdout + r.stderr).splitlines() if not l.startswith("record clip:"))
    assert r.returncode == 0 and ("ok " + case) in r.stdout, "%s: exit %d\n%s" % (case, r.returncode, out[-4000:])


@pytest.mark.parametrize("case", sorted(ARENA_CASES))
def test_arena_exact_fit_one_short_and_ladder(case, emul_lib_path, oracle):
    _child(case, emul_lib_path, ARENA_CASES[case][1])


@pytest.mark.parametrize("case", ["entries", "scene-event"])
def test_entries_that_size_the_arena_themselves(case, emul_lib_path, oracle):
    _child(case, emul_lib_path, OTHER_CASES[case][1])


@pytest.mark.parametrize("case", ["scratch-blob", "scratch-torus", "scratch-threshold", "scratch-torus40-last"])
def test_scratch_ladder_exact_event_or_capacity(case, emul_lib_path):
    _child(case, emul_lib_path, OTHER_CASES[case][1])


def test_literal_clipper_without_room_flags_and_counts(emul_lib_path):
    _child("literal", emul_lib_path, OTHER_CASES["literal"][1])


# ------------------------------------------------------------------ GPU tier
# seconds of each child on its first run on the MI355X (python start, scene and oracle included)
MEASURED_GPU_SECONDS = {"arena-cube": 0.8, "arena-blob64": 0.7, "arena-torus": 0.7, "scratch-torus200": 2.7}
GPU_CHILD = """
import os, sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import test_capacity_limits as T
T.gpu_case(sys.argv[1])
"""


def gpu_case(case):
    t = time.time()
    engine._use_library_for_tests(None)
    em = Device()
    if case.startswith("arena-"):
        sc = SCENES[case.split("-")[1]]()
        arena_case(em, sc, 3, 4, lambda qs, c, n, ev: None, oracle_reference(sc, 3, 4), ladders=False)
    else:
        os.environ["SURTR_REC"] = "0"      # the bands to the general clipper: the record clipper has scratch of its own
        sc = scenes.make_scene(*meshgen.bumpy_torus(200, 120), 2)
        v, h = sc["mesh"]["pos"].shape[0], int(sc["mesh"]["off"][-1])
        outcome = scratch_case(em, sc, scratch_rungs(v, h, short=True))
        # (the automatic rung is compared with itself: a rung with capacities of its own has to succeed, and one to be refused)
        assert outcome[(0, 0)] and outcome[(v, h)] and not all(outcome.values()), outcome
    print("%s: %.1f s" % (case, time.time() - t))
    print("ok " + case)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(MEASURED_GPU_SECONDS))
def test_gpu_capacity_boundary(case, oracle):
    run_gpu_child(GPU_CHILD, case, max(60, int(4 * MEASURED_GPU_SECONDS[case])))


if __name__ == "__main__":
    run_child(sys.argv[1], sys.argv[2])
