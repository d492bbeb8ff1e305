"""The pattern library: pattern_store / pattern_select / pattern_info / pattern_clear, place_cells_patterns (k_place_cells_patterns),
placed_cells, scene_fracture_impacts over CELLS_ALL and event_regroup_impacts_partial (a "no sphere" entry for k_rg_faces).

THE REFERENCE IS THE EXISTING CODE and never runs a new call.  A twin engine runs the impacts of a frame one after the other through
upload_pattern (of that impact's pattern), scene_apply_poses, place_cells, scene_outside (no mask when the impact is not partial),
scene_fracture_bodies, event_regroup_bodies (with that impact's flag), event_refit and scene_commit.  Everything is compared without a
tolerance: planes, masks, counts, the refitted event fragment after fragment, frag_ids (cell - cell_base[i]; piece numbers translated to
the scene before the frame), the compounds body by body, the composed src, every resident Mesh and Convex, table, poses, scene_mass.

Patterns, stored in this order: A the 8-cell cube pattern of test_scene.bodies (68 faces, stored after upload_pattern), B build_cells of
five seeds (uniform_seeds(5, 72): cells of differing face counts), C build_cells of two seeds (uniform_seeds(2, 73)); B and C are
stored after build_cells.  The library's buffers get half as much room again (and 64 words) as the first store needs, so storing B and
C (together more than half of A's faces and 64 words; asserted) makes them grow with A inside.  Six instances of A are 408 planes:
more than one 256-thread workgroup, with an instance boundary inside a workgroup.

Scene and impacts: test_scene_impacts' (six compounds after click 1; MAIN's two spheres).  Three conditions are asserted on the
sequential reference alone (frame_conditions): (a) under the partial impact a fragment moves to its body's bind 0; (b) for the impact
that is not partial the same reference run with the flag on would mask a piece or move a fragment; (c) the two patterns give that
impact's bodies different fragment counts.  MAIN's origins and radii are kept.  With the first seed tried for B, 71, (c) failed on the
CPU tier: compound 2 breaks into 14 fragments under A and under B alike.  Seed 72 was chosen by running the reference alone over the
seeds 71..83: compound 2 gives 14 fragments under A and 16 under B, compounds {4, 0} give 8 and 5, and (a) and (b) hold in the frame and
in the swapped frame.

The CPU tier runs on the emulation library (conftest's emul_engine); the GPU tier runs the same cases on the MI355X in child processes
under a time limit (helpers.run_gpu_child)."""
import textwrap

import numpy as np
import pytest

import test_scene as TS
import test_scene_bodies as TB
import test_scene_impacts as TI
from helpers import run_gpu_child
from surtr_amd import engine, scenes

SEEDS_B, SEEDS_C = (5, 72), (2, 73)
N_FACES_A = 68
_PATTERNS = {}


def patterns(E):
    """A, B, C as dict(face_off, v012[, seeds]); B's and C's arrays are what build_cells leaves (download_cells).  Computed once."""
    if not _PATTERNS:
        cube = TS.bodies(E)["cube"]
        _PATTERNS["A"] = dict(face_off=np.asarray(cube["face_off"], np.uint32), v012=np.asarray(cube["v012"], np.float32).reshape(-1, 9))
        tmp = E.Engine(0)
        for name, (n, seed) in (("B", SEEDS_B), ("C", SEEDS_C)):
            seeds = scenes.uniform_seeds(n, seed)
            tmp.build_cells(seeds)
            got = tmp.download_cells()
            _PATTERNS[name] = dict(face_off=got["cell_face_off"], v012=got["v012"], seeds=seeds)
        tmp.close()
        a, b, c = (_PATTERNS[k] for k in "ABC")
        nf = [x["v012"].shape[0] for x in (a, b, c)]
        assert nf[0] == N_FACES_A and len(a["face_off"]) == 9 and len(b["face_off"]) == 6 and len(c["face_off"]) == 3
        assert len(set(np.diff(b["face_off"].astype(np.int64)))) > 1, b["face_off"]           # cells with differing face counts
        assert 9 * sum(nf) > 9 * nf[0] + 9 * nf[0] // 2 + 64, nf                              # the library grows while A is in it
    return _PATTERNS


ORDER = "ABC"


def n_cells(P):
    return len(P["face_off"]) - 1


def install(eng, P):
    """The parent's only routes to a pattern."""
    if "seeds" in P:
        eng.build_cells(P["seeds"])
    else:
        eng.upload_pattern(P["face_off"], P["v012"])


def fill_library(E, eng, check=None):
    pats = patterns(E)
    for k, name in enumerate(ORDER):
        install(eng, pats[name])
        assert eng.pattern_store() == k and eng.pattern_count() == k + 1
        if check:
            check(k)
    return pats


PLACE = (np.float32([1.5, 2.25, 0.75]), np.float32([0.25, -1.0, 3.0]))


def planes_of(E, P, place=PLACE):
    """place_cells on a fresh engine after the parent's route to pattern P."""
    ref = E.Engine(0)
    install(ref, P)
    ref.place_cells(*place)
    out = ref.download_planes()
    ref.close()
    return out


# ------------------------------------------------------------------ 1. the library's state
def run_library(E):
    pats = patterns(E)
    want = {k: planes_of(E, pats[name]) for k, name in enumerate(ORDER)}
    eng = E.Engine(0)

    def selected_equals(k, upto):
        for j in range(upto + 1):
            eng.pattern_select(j)
            eng.place_cells(*PLACE)
            got = eng.download_planes()
            assert got.shape == want[j].shape and got.tobytes() == want[j].tobytes(), (k, j)
    fill_library(E, eng, check=lambda k: selected_equals(k, k))      # after every store: before the growth (k = 0) and after it
    for k, name in enumerate(ORDER):
        assert eng.pattern_info(k) == (n_cells(pats[name]), pats[name]["v012"].shape[0]), k
    # a pattern that was itself installed by pattern_select
    eng.pattern_select(1)
    assert eng.pattern_store() == 3 and eng.pattern_count() == 4 and eng.pattern_info(3) == eng.pattern_info(1)
    want[3] = want[1]
    selected_equals(3, 3)
    eng.close()
    # a whole event after pattern_select against the one after the parent's route, every array
    out = []
    for route in ("select", "parent"):
        e, world = TS.three_bodies(E)
        if route == "select":
            fill_library(E, e)
            e.pattern_select(1)
        else:
            install(e, pats["B"])
        e.place_cells(np.float32([2, 2, 2]), np.float32([0.1, 0.0, -0.1]))
        c = e.scene_fracture_event(0, 0, n_cells(pats["B"]))
        ev = e.download()
        out.append((bytes(c), {k: np.asarray(v).tobytes() for k, v in ev.items()}))
        e.close()
    assert out[0][0] == out[1][0] and engine.Counts.from_buffer_copy(out[0][0]).n_frag > 1
    assert out[0][1].keys() == out[1][1].keys()
    for k in out[0][1]:
        assert out[0][1][k] == out[1][1][k], k


# ------------------------------------------------------------------ 2. placement
def transforms(k):
    """k distinct anisotropic scales and translates."""
    i = np.arange(k, dtype=np.float32)[:, None]
    return (np.float32([1.5, 2.25, 0.75]) + np.float32([0.5, 0.125, 0.25]) * i).astype(np.float32), \
           (np.float32([0.25, -1.0, 3.0]) + np.float32([-1.5, 0.75, 0.5]) * i).astype(np.float32)


def run_placement(E):
    eng, twin = E.Engine(0), E.Engine(0)
    pats = fill_library(E, eng)
    fill_library(E, twin)
    eng.pattern_select(1)
    eng.place_cells(*PLACE)
    plain = eng.download_planes()
    for ids in ([2, 0, 2, 1], [1], [0] * 6):
        s, t = transforms(len(ids))
        eng.place_cells_patterns(ids, s, t)
        got = eng.download_planes(impacts=True)
        nf = [pats[ORDER[k]]["v012"].shape[0] for k in ids]
        pre = np.cumsum([0] + nf)
        assert got.shape[0] == pre[-1]
        for i, k in enumerate(ids):
            twin.pattern_select(k)
            twin.place_cells(s[i], t[i])
            assert got[pre[i]:pre[i + 1]].tobytes() == twin.download_planes().tobytes(), (ids, i)
        assert list(eng.placed_cells()) == list(np.cumsum([0] + [n_cells(pats[ORDER[k]]) for k in ids])), ids
        # the installed pattern and the plain placement are as they were
        assert eng.download_planes().tobytes() == plain.tobytes()
    assert 6 * N_FACES_A > 256 and 256 % N_FACES_A != 0            # more than one workgroup, an instance boundary inside one
    # one pattern for all instances: place_cells_impacts of the same transforms
    s, t = transforms(6)
    twin.pattern_select(0)
    twin.place_cells_impacts(s, t)
    assert eng.download_planes(impacts=True).tobytes() == twin.download_planes(impacts=True).tobytes()
    assert list(eng.placed_cells()) == list(twin.placed_cells()) == [8 * i for i in range(7)]
    eng.place_cells(*PLACE)
    assert eng.download_planes().tobytes() == plain.tobytes()
    eng.close(); twin.close()


# ------------------------------------------------------------------ 3. the frame
def with_choice(im, pattern, partial):
    return dict(im, pattern=pattern, partial=bool(partial))


def sequential(ref, pats, impacts, probe=False):
    """The reference: the parent's calls, impact after impact, each with its own pattern and flag (see the module's docstring).
    -> per impact what test_scene_impacts.sequential_impacts returns, and with probe, measured on the reference before the impact
    runs: n_frag_by[name] of an unmasked event on its targets for every pattern of the frame, would_mask (scene_outside under its
    sphere), and after its event moved_if_partial (event_regroup_bodies with the flag on)."""
    table0 = [int(x) for x in ref.scene_compounds()]
    now = list(range(len(table0) - 1))
    piece_orig = list(range(table0[-1]))
    origin_of = [("old", p) for p in range(table0[-1])]
    names = sorted(set(im["pattern"] for im in impacts))
    out = []
    for i, im in enumerate(impacts):
        P, partial = pats[im["pattern"]], im["partial"]
        targets = [now[c] for c in im["targets"]]
        assert None not in targets
        ref.scene_apply_poses(targets)
        n_frag_by = {}
        for name in names if probe else ():
            ref.upload_pattern(pats[name]["face_off"], pats[name]["v012"])
            ref.place_cells(im["scale"], im["translate"])
            n_frag_by[name] = int(ref.scene_fracture_bodies(targets, 0, n_cells(pats[name]), flags=0).n_frag)
        ref.upload_pattern(P["face_off"], P["v012"])
        ref.place_cells(im["scale"], im["translate"])
        planes = ref.download_planes()
        table = [int(x) for x in ref.scene_compounds()]
        would_mask = ref.scene_outside(targets, im["cloud"], im["origin"], im["radius"])
        mask = would_mask if partial else None
        c = ref.scene_fracture_bodies(targets, 0, n_cells(P), outside=mask, flags=0)
        kw = dict(partial=True, sphere_points=im["cloud"], origin=im["origin"], radius=im["radius"])
        co, cp, bo = ref.event_regroup_bodies(**(kw if partial else {}))
        skipped = [piece_orig[p] for t in sorted(targets) for j, p in enumerate(range(table[t], table[t + 1]))
                   if partial and mask[sum(table[u + 1] - table[u] for u in targets[:targets.index(t)]) + j]]
        moved = TI.moved_fragments(co, cp, bo, len(skipped))
        moved_if_partial = TI.moved_fragments(*ref.event_regroup_bodies(**kw), len(skipped)) if probe else None
        ref.event_refit()
        ev = ref.download()
        ids = ev["frag_ids"].reshape(-1, 3).copy()
        ids[:, 1] = [piece_orig[p] for p in ids[:, 1]]
        n, first, n_new, src = ref.scene_commit(co, cp)
        origin_of = [origin_of[s] if s >= 0 else ("frag", i, -int(s) - 1) for s in src]
        piece_orig = [piece_orig[s] if s >= 0 else None for s in src]
        gone = sorted(targets)
        now = [None if (k is None or k in gone) else k - sum(1 for g in gone if g < k) for k in now]
        out.append(dict(mask=mask if partial else np.zeros(len(would_mask), np.uint8), n_frag=int(c.n_frag), n_pairs=int(c.n_pairs), ev=ev, ids=ids,
                        co=co, cp=cp, bo=bo, skipped=skipped, moved=moved, planes=planes, partial=partial, pattern=im["pattern"],
                        n_frag_by=n_frag_by, would_mask=would_mask, moved_if_partial=moved_if_partial))
    return out, origin_of


def frame_conditions(seq):
    """On the sequential reference alone: a kernel that ignores the pattern or the flag cannot pass the comparison."""
    print([(s["pattern"], s["partial"], s["n_frag"], s["moved"], s["would_mask"], s["moved_if_partial"], s["n_frag_by"]) for s in seq])
    assert all(s["n_frag"] > 0 for s in seq)
    assert any(len(m) for s in seq if s["partial"] for m in s["moved"])                                               # (a)
    assert all(s["would_mask"].any() or any(len(m) for m in s["moved_if_partial"]) for s in seq if not s["partial"])  # (b)
    assert any(not s["partial"] for s in seq) and any(s["partial"] for s in seq)
    assert any(len(set(s["n_frag_by"].values())) > 1 for s in seq if not s["partial"])                               # (c)


def library_frame(E, eng, ref, impacts, conditions=None, use_async=False, library=True, sparse_clouds=True):
    """The frame through the new calls on eng (which holds the library A, B, C), everything compared with the reference on ref.
    library=False: one pattern for all impacts through place_cells_impacts and its cell range, with the flags per impact."""
    pats = patterns(E)
    table0 = [int(x) for x in eng.scene_compounds()]
    seq, origin_of = sequential(ref, pats, impacts, probe=conditions is not None)
    if conditions is not None:
        conditions(seq)
    K = len(impacts)
    targets = [im["targets"] for im in impacts]
    flat = [t for ts in targets for t in ts]
    flags = [im["partial"] for im in impacts]
    eng.scene_apply_poses(flat)
    scales, translates = [im["scale"] for im in impacts], [im["translate"] for im in impacts]
    if library:
        eng.place_cells_patterns([ORDER.index(im["pattern"]) for im in impacts], scales, translates)
        cells = (0, E.CELLS_ALL)
    else:
        assert len(set(im["pattern"] for im in impacts)) == 1
        eng.pattern_select(ORDER.index(impacts[0]["pattern"]))
        eng.place_cells_impacts(scales, translates)
        cells = (0, n_cells(pats[impacts[0]["pattern"]]))
    base = [int(x) for x in eng.placed_cells()]
    assert base == list(np.cumsum([0] + [n_cells(pats[im["pattern"]]) for im in impacts]))
    planes = eng.download_planes(impacts=True)
    pre = np.cumsum([0] + [pats[im["pattern"]]["v012"].shape[0] for im in impacts])
    assert planes.shape[0] == pre[-1]
    for i in range(K):
        assert planes[pre[i]:pre[i + 1]].tobytes() == seq[i]["planes"].tobytes(), ("planes", i)
    clouds, origins, radii = [im["cloud"] for im in impacts], [im["origin"] for im in impacts], [im["radius"] for im in impacts]
    mask = eng.scene_outside_impacts(targets, clouds, origins, radii)
    assert mask.tobytes() == np.concatenate([s["would_mask"] for s in seq]).tobytes()
    at = 0
    for s in seq:                                        # the caller zeroes the bytes of the impacts that are not partial
        if not s["partial"]:
            mask[at:at + len(s["would_mask"])] = 0
        at += len(s["would_mask"])
    assert mask.tobytes() == np.concatenate([s["mask"] for s in seq]).tobytes()
    if use_async:
        eng.scene_fracture_impacts_async(targets, cells[0], cells[1], outside=mask, flags=0)
        c = eng.event_counts()
    else:
        c = eng.scene_fracture_impacts(targets, cells[0], cells[1], outside=mask, flags=0)
    assert c.status == 0 and c.n_frag == sum(s["n_frag"] for s in seq) and c.n_pairs == sum(s["n_pairs"] for s in seq)
    frag_off = np.cumsum([0] + [s["n_frag"] for s in seq])
    # (an impact that is not partial has no cloud here: its range is empty)
    co, cp, bo = eng.event_regroup_impacts_partial(flags, [cl if f or not sparse_clouds else None for cl, f in zip(clouds, flags)], origins, radii)
    skipped = sorted(p for s in seq for p in s["skipped"])
    body0 = np.cumsum([0] + [len(ts) for ts in targets])
    assert len(bo) == len(flat) + 1 and bo[0] == 0 and bo[-1] == len(co) - 1
    for i, s in enumerate(seq):
        def local(q):
            if q < len(skipped):
                return s["skipped"].index(skipped[q])
            f = q - len(skipped)
            assert frag_off[i] <= f < frag_off[i + 1], (i, q)
            return len(s["skipped"]) + f - int(frag_off[i])
        for b, want in enumerate(TI.body_compounds(s)):
            g = int(body0[i]) + b
            got = [[local(int(q)) for q in cp[co[k]:co[k + 1]]] for k in range(int(bo[g]), int(bo[g + 1]))]
            assert got == want, (i, b, got, want)
    eng.event_refit()
    ev = eng.download()
    ids = ev["frag_ids"].reshape(-1, 3)
    for i, s in enumerate(seq):
        mine = ids[frag_off[i]:frag_off[i + 1]]
        assert ((mine[:, 0] >= base[i]) & (mine[:, 0] < base[i + 1])).all() and list(mine[:, 0] - base[i]) == list(s["ids"][:, 0]), (i, mine[:, 0])
        assert list(mine[:, 1]) == list(s["ids"][:, 1]) and list(mine[:, 2]) == list(s["ids"][:, 2]), (i, mine, s["ids"])
    for key in TS.EVENT_KEYS:
        if key.endswith("_off"):
            assert list(np.diff(ev[key].astype(np.int64))) == [int(d) for s in seq for d in np.diff(s["ev"][key].astype(np.int64))], key
        else:
            assert np.asarray(ev[key]).tobytes() == b"".join(np.asarray(s["ev"][key]).tobytes() for s in seq), key
    n, first, n_new, src = eng.scene_commit(co, cp)
    assert first == len(table0) - 1 - len(flat) and n == int(ref.scene_compounds()[-1]) and first + n_new == len(ref.scene_compounds()) - 1
    got_origin = []
    for sv in src:
        if sv >= 0:
            got_origin.append(("old", int(sv)))
        else:
            f = -int(sv) - 1
            i = int(np.searchsorted(frag_off, f, side="right")) - 1
            got_origin.append(("frag", i, f - int(frag_off[i])))
    assert got_origin == origin_of
    TB.assert_same_scene(eng, ref)
    return seq


def fresh(E):
    eng, ref = TI.fresh(E)
    fill_library(E, eng)
    return eng, ref


def run_frame(E, choice=(("A", 1), ("B", 0)), use_async=False):
    eng, ref = fresh(E)
    frame = [with_choice(im, *ch) for im, ch in zip(TI.MAIN, choice)]
    seq = library_frame(E, eng, ref, frame, conditions=frame_conditions, use_async=use_async)
    eng.close(); ref.close()
    return [s["n_frag"] for s in seq]


def run_frame_swapped(E):
    return run_frame(E, (("B", 0), ("A", 1)))


def run_frame_async(E):
    return run_frame(E, use_async=True)


THREE = [TI.impact((6.0, 0.0, 0.7), 4.0, [4]), TI.impact((11.0, 0.5, 0.3), 2.0, [2]), TI.impact((0.4, 0.2, 0.1), 0.8, [0])]


def run_frame_three(E):
    eng, ref = fresh(E)
    frame = [with_choice(im, *ch) for im, ch in zip(THREE, (("A", 1), ("C", 0), ("A", 1)))]

    def conditions(seq):
        print([(s["pattern"], s["partial"], s["n_frag"], s["n_frag_by"]) for s in seq])
        assert all(s["n_frag"] > 0 for s in seq)
    library_frame(E, eng, ref, frame, conditions=conditions)
    eng.close(); ref.close()


# ------------------------------------------------------------------ 4. the flags of the regrouping
def run_flags(E):
    pats = patterns(E)
    a, b = TI.MAIN
    clouds, origins, radii = [a["cloud"], b["cloud"]], [a["origin"], b["origin"]], [a["radius"], b["radius"]]
    targets = [a["targets"], b["targets"]]
    eng, ref = fresh(E)
    ref.close()
    eng.scene_apply_poses([t for ts in targets for t in ts])
    eng.place_cells_patterns([0, 1], [a["scale"], b["scale"]], [a["translate"], b["translate"]])
    mask = eng.scene_outside_impacts(targets, clouds, origins, radii)
    eng.scene_fracture_impacts(targets, 0, E.CELLS_ALL, outside=mask, flags=0)
    same = lambda x, y: all(list(p) == list(q) for p, q in zip(x, y)) and len(x) == len(y) == 3
    ones = eng.event_regroup_impacts(partial=True, sphere_points=clouds, origins=origins, radii=radii)
    zeros = eng.event_regroup_impacts(n_impacts=2)
    assert not same(ones, zeros)
    assert same(eng.event_regroup_impacts_partial([1, 1], clouds, origins, radii), ones)
    assert same(eng.event_regroup_impacts_partial([0, 0], clouds, origins, radii), zeros)
    assert same(eng.event_regroup_impacts_partial([0, 0]), zeros)                     # no sphere at all: none is read
    mixed = [eng.event_regroup_impacts_partial(f, clouds, origins, radii) for f in ([1, 0], [0, 1])]
    assert same(mixed[0], eng.event_regroup_impacts_partial([1, 0], [clouds[0], None], origins, radii))      # an empty cloud
    assert same(mixed[1], eng.event_regroup_impacts_partial([0, 1], [None, clouds[1]], origins, radii))
    assert not same(mixed[0], mixed[1]) and len(set(repr([list(x) for x in r]) for r in (ones, zeros, mixed[0], mixed[1]))) >= 3
    eng.close()
    # [1, 0] and [0, 1] against the per-impact reference, after place_cells_impacts too (after place_cells_patterns: the frames above)
    for flags in ((1, 0), (0, 1)):
        eng, ref = fresh(E)
        library_frame(E, eng, ref, [with_choice(im, "A", f) for im, f in zip(TI.MAIN, flags)], library=False, sparse_clouds=bool(flags[0]))
        eng.close(); ref.close()


# ------------------------------------------------------------------ 5. refusals
def run_refusals(E):
    pats = patterns(E)
    a, b = TI.MAIN
    s2, t2 = [a["scale"], b["scale"]], [a["translate"], b["translate"]]
    eng = TB.scene_after_click_one(E)
    before = TS.snapshot(eng)

    def state():
        """The library, the installed pattern, the placements and the current event, as far as a caller can read them."""
        out = [eng.pattern_count(), [eng.pattern_info(k) for k in range(eng.pattern_count())]]
        for what in (lambda: eng.download_planes().tobytes(), lambda: eng.download_planes(impacts=True).tobytes(), lambda: list(eng.placed_cells()),
                     lambda: bytes(eng.event_counts()), lambda: eng.download()["frag_ids"].tobytes()):
            try:
                out.append(what())
            except engine.SurtrError as e:
                out.append(("error", e.code))
        return out

    def refused(code, call):
        was = state()
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == code, e.value
        assert state() == was
        TS.assert_unchanged(eng, before)
    # store without a pattern (a context that never had one), and after upload_planes
    bare = E.Engine(0)
    for call in (bare.pattern_store, bare.placed_cells):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == engine.E_STATE and bare.pattern_count() == 0
    bare.close()
    refused(engine.E_INVALID, lambda: eng.pattern_select(0))
    refused(engine.E_INVALID, lambda: eng.place_cells_patterns([0], s2[:1], t2[:1]))
    eng.upload_pattern(pats["A"]["face_off"], pats["A"]["v012"])
    eng.place_cells(*PLACE)
    planes = eng.download_planes()
    eng.upload_planes(pats["A"]["face_off"], planes)
    refused(engine.E_STATE, eng.pattern_store)
    assert eng.pattern_count() == 0
    fill_library(E, eng)
    eng.place_cells(*PLACE)
    # an id out of range
    for bad in (3, 0xFFFFFFFF):
        refused(engine.E_INVALID, lambda: eng.pattern_select(bad))
        refused(engine.E_INVALID, lambda: eng.pattern_info(bad))
        refused(engine.E_INVALID, lambda: eng.place_cells_patterns([0, bad], s2, t2))
    refused(engine.E_INVALID, lambda: eng.place_cells_patterns([], np.zeros((0, 3)), np.zeros((0, 3))))      # n_impacts == 0
    # the event: no instances; another range than CELLS_ALL; another n_impacts than was placed
    refused(engine.E_STATE, lambda: eng.scene_fracture_impacts([[4, 0], [2]], 0, E.CELLS_ALL, flags=0))
    eng.place_cells_patterns([0, 1], s2, t2)
    for call in (eng.scene_fracture_impacts, eng.scene_fracture_impacts_async):
        for rng in ((0, 8), (0, 13), (0, 5), (1, E.CELLS_ALL), (0, E.CELLS_ALL - 1)):
            refused(engine.E_INVALID, lambda: call([[4, 0], [2]], rng[0], rng[1], flags=0))
        refused(engine.E_STATE, lambda: call([[4, 2, 0]], 0, E.CELLS_ALL, flags=0))
        refused(engine.E_STATE, lambda: call([[4], [2], [0]], 0, E.CELLS_ALL, flags=0))
    # CELLS_ALL after place_cells_impacts stays refused
    eng.pattern_select(0)
    eng.place_cells(*PLACE)
    eng.place_cells_impacts(s2, t2)
    refused(engine.E_INVALID, lambda: eng.scene_fracture_impacts([[4, 0], [2]], 0, E.CELLS_ALL, flags=0))
    # a current event stays as it is through refused calls
    eng.place_cells_patterns([0, 1], s2, t2)
    eng.scene_fracture_impacts([[4, 0], [2]], 0, E.CELLS_ALL, flags=0)
    refused(engine.E_INVALID, lambda: eng.scene_fracture_impacts([[4, 0], [2]], 0, 8, flags=0))
    refused(engine.E_INVALID, lambda: eng.place_cells_patterns([0, 7], s2, t2))
    refused(engine.E_STATE, lambda: eng.event_regroup_impacts_partial([1, 0, 1]))
    refused(engine.E_INVALID, lambda: eng.event_regroup_impacts_partial([]))
    # select forgets the placed instances; so does clear, which also empties the library
    eng.pattern_select(2)
    refused(engine.E_STATE, lambda: eng.scene_fracture_impacts([[4, 0], [2]], 0, E.CELLS_ALL, flags=0))
    refused(engine.E_STATE, eng.placed_cells)
    eng.place_cells_patterns([0, 1], s2, t2)
    eng.pattern_clear()
    assert eng.pattern_count() == 0
    refused(engine.E_STATE, lambda: eng.scene_fracture_impacts([[4, 0], [2]], 0, E.CELLS_ALL, flags=0))
    refused(engine.E_INVALID, lambda: eng.place_cells_patterns([0, 1], s2, t2))
    # ... but not the installed pattern (C, selected above), and ids start again at 0
    assert eng.pattern_store() == 0 and eng.pattern_info(0) == (n_cells(pats["C"]), pats["C"]["v012"].shape[0])
    eng.place_cells_patterns([0, 0], s2, t2)
    c = eng.scene_fracture_impacts([[4, 0], [2]], 0, E.CELLS_ALL, flags=0)
    assert c.status == 0 and c.n_frag > 0 and list(eng.placed_cells()) == [0, 2, 4]
    eng.close()


# ------------------------------------------------------------------ CPU tier (emulation)
def test_library_state_and_select_equals_the_upload(emul_engine):
    run_library(emul_engine)


def test_placement_with_a_pattern_per_instance(emul_engine):
    run_placement(emul_engine)


def test_frame_with_a_pattern_and_a_flag_per_impact_equals_sequential_impacts(emul_engine):
    print(run_frame(emul_engine))


def test_frame_with_patterns_and_flags_swapped(emul_engine):
    print(run_frame_swapped(emul_engine))


def test_frame_of_three_impacts_on_two_patterns(emul_engine):
    run_frame_three(emul_engine)


def test_frame_async_event_then_event_counts(emul_engine):
    print(run_frame_async(emul_engine))


def test_regroup_flags_per_impact(emul_engine):
    run_flags(emul_engine)


def test_refusals_leave_library_pattern_placements_scene_and_event_unchanged(emul_engine):
    run_refusals(emul_engine)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_pattern_library as T
    case = sys.argv[1]
    getattr(T, "run_" + case)(engine)
    print("ok", case)
""")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["library", "placement", "frame", "frame_swapped", "frame_three", "frame_async", "flags", "refusals"])
def test_gpu_pattern_library(case):
    run_gpu_child(GPU_CHILD, case, 120)
