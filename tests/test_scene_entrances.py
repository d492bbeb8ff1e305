"""The three entrances of the scene fracture cycle -- one compound (scene_fracture_event, event_regroup), several bodies
(scene_outside, scene_fracture_bodies, event_regroup_bodies) and several impacts (scene_outside_impacts, scene_fracture_impacts,
event_regroup_impacts) -- pinned where they share code: what each refuses and with which code, that they agree where their
arguments say the same thing, and the state each leaves behind.  Nothing here has a tolerance.

(a) REFUSALS.  One bad argument at a time, and pairs of faults where the order of the checks decides the code.  After every refusal
    the scene is what it was, and the correct call gives the bits it gives on a fresh engine.  The codes are what the library returns;
    where include/surtr_hip.h says less or something else, the library's behaviour is what is pinned:
      * K == 0 is SURTR_E_INVALID for scene_fracture_impacts even when nothing is placed (the header lists it, and lists SURTR_E_STATE
        for "without surtr_place_cells_impacts", without saying which wins); with K >= 1, SURTR_E_STATE wins over any bad target list;
      * scene_outside with an empty list is SURTR_E_INVALID on an engine without pieces, with any other list SURTR_E_STATE;
        scene_outside_impacts on such an engine is SURTR_E_STATE whatever the lists hold (K == 0 excepted);
      * the regroup calls check the event before the sphere: no event and no origin is SURTR_E_STATE; event_regroup_impacts checks K == 0
        (SURTR_E_INVALID) before the event, and the event (SURTR_E_STATE) before sphere_off;
      * the header does not say that a fracture call on pieces without a placement is SURTR_E_STATE whatever else is wrong with it.
(b) IDENTITIES.  scene_fracture_bodies([c]) is scene_fracture_event(c); scene_fracture_impacts of one impact after
    place_cells_impacts of one instance is scene_fracture_bodies after place_cells of that scale and translate -- with a mask that
    keeps some pieces out and not others, over cells [3, 8): counts, event, frag_ids, regroup tables, commit and committed scene.
    (The whole-pattern forms are test_scene_bodies.run_one_target and test_scene_impacts.run_one_impact, run here as well.)
(c) STATE.  Which compounds scene_commit erases after each entrance; the plain placement's planes through an impacts event; the
    impacts placement's planes through a plain event.

Scene: test_scene_bodies' (six compounds after click 1) with the 8-cell cube pattern.  The CPU tier runs on the emulation library, the
GPU tier runs the same cases in child processes under a time limit (helpers.run_gpu_child)."""
import ctypes
import textwrap

import numpy as np
import pytest

import test_scene as TS
import test_scene_bodies as TB
import test_scene_impacts as TI
from helpers import run_gpu_child
from surtr_amd import engine

INVALID, CAPACITY, STATE = engine.E_INVALID, engine.E_CAPACITY, engine.E_STATE
N_CELLS = TI.N_CELLS
A, B = TI.MAIN                                    # two impacts: targets [4, 0] and [2]
FRAME = [A["targets"], B["targets"]]
CLOUDS, ORIGINS, RADII = [A["cloud"], B["cloud"]], [A["origin"], B["origin"]], [A["radius"], B["radius"]]
u32, f32 = ctypes.c_uint32, ctypes.c_float


def arr(x, dtype):
    return None if x is None else np.ascontiguousarray(x, dtype)


def ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def scene(E, place="both"):
    """test_scene_bodies' scene with the pattern uploaded; place: None, "plain" (A's click) or "both" (and the frame's two instances)."""
    eng = TB.scene_after_click_one(E)
    cube = TS.bodies(E)["cube"]
    eng.upload_pattern(cube["face_off"], cube["v012"])
    if place:
        eng.place_cells(A["scale"], A["translate"])
    if place == "both":
        eng.place_cells_impacts([A["scale"], B["scale"]], [A["translate"], B["translate"]])
    return eng


def event_bits(eng, counts=None):
    ev = eng.download()
    c = eng.event_counts() if counts is None else counts
    return [bytes(c)] + [np.asarray(ev[k]).tobytes() for k in TS.EVENT_KEYS + ("frag_ids",)] + [eng.pair_order().tobytes()]


def code_of(call):
    """The code a call is refused with, through the Python wrapper (SurtrError) or as the library's return value."""
    try:
        rc = call()
    except engine.SurtrError as e:
        return e.code
    assert isinstance(rc, int) and rc != 0, ("not refused", rc)
    return rc


def check_refusals(eng, cases, good, want_bits):
    """Every case is refused with its code, leaves the scene alone, and the correct call after it gives want_bits."""
    before, poses = TS.snapshot(eng), eng.scene_poses().tobytes()
    for name, code, call in cases:
        assert code_of(call) == code, name
        TS.assert_unchanged(eng, before)
        assert eng.scene_poses().tobytes() == poses, name
        assert good(eng) == want_bits, ("after", name)


# ------------------------------------------------------------------ (a) 1. the fracture entrances
def good_event(eng):
    return event_bits(eng, eng.scene_fracture_event(2, 0, N_CELLS, flags=0))


def good_bodies(eng):
    return event_bits(eng, eng.scene_fracture_bodies(TB.CLICK_TARGETS, 0, N_CELLS, flags=0))


def good_impacts(eng):
    return event_bits(eng, eng.scene_fracture_impacts(FRAME, 0, N_CELLS, flags=0))


def run_refusals_fracture(E):
    fresh = {}
    for good in (good_event, good_bodies, good_impacts):
        eng = scene(E)
        fresh[good] = good(eng)
        eng.close()
    bare = E.Engine(0)                            # no pieces: SURTR_E_STATE, also with a second fault; K == 0 alone is named first
    unplaced = scene(E, None)                     # pieces and a pattern, no placement: the same
    plain = scene(E, "plain")                     # no impacts placement
    for e in (bare, unplaced):
        for call in (e.scene_fracture_event, e.scene_fracture_event_async):
            assert code_of(lambda: call(2, 0, N_CELLS, flags=0)) == STATE
            assert code_of(lambda: call(99, 5, 3, flags=0)) == STATE
        for call in (e.scene_fracture_bodies, e.scene_fracture_bodies_async):
            assert code_of(lambda: call([4, 2, 0], 0, N_CELLS, flags=0)) == STATE
            assert code_of(lambda: call([0, 2, 2], 0, N_CELLS + 1, flags=0)) == STATE
            assert code_of(lambda: call([], 0, N_CELLS, flags=0)) == STATE
    for e in (bare, unplaced, plain):
        for call in (e.scene_fracture_impacts, e.scene_fracture_impacts_async):
            assert code_of(lambda: call(FRAME, 0, N_CELLS, flags=0)) == STATE
            assert code_of(lambda: call([[4, 4], []], 5, 3, flags=0)) == STATE
            assert code_of(lambda: call([], 0, N_CELLS, flags=0)) == INVALID
    # a plain placement is enough for the one-compound and the bodies entrance, after the refusals above
    assert good_event(plain) == fresh[good_event] and good_bodies(plain) == fresh[good_bodies]
    for e in (bare, unplaced, plain):
        e.close()

    eng = scene(E)
    for call in (eng.scene_fracture_event, eng.scene_fracture_event_async):
        check_refusals(eng, [
            ("compound out of range", INVALID, lambda: call(6, 0, N_CELLS, flags=0)),
            ("cell_begin > cell_end", INVALID, lambda: call(2, 5, 3, flags=0)),
            ("cell_end > n_cells", INVALID, lambda: call(2, 0, N_CELLS + 1, flags=0)),
            ("compound and cells", INVALID, lambda: call(6, N_CELLS + 2, N_CELLS + 1, flags=0)),
        ], good_event, fresh[good_event])
    check_refusals(eng, [("mask of another length", INVALID, lambda: eng.scene_fracture_event(2, 0, N_CELLS, outside=[0] * 4, flags=0))],
                   good_event, fresh[good_event])
    for call in (eng.scene_fracture_bodies, eng.scene_fracture_bodies_async):
        check_refusals(eng, [
            ("no target", INVALID, lambda: call([], 0, N_CELLS, flags=0)),
            ("compound out of range", INVALID, lambda: call([6, 2], 0, N_CELLS, flags=0)),
            ("ascending", INVALID, lambda: call([0, 2, 4], 0, N_CELLS, flags=0)),
            ("twice", INVALID, lambda: call([4, 2, 2], 0, N_CELLS, flags=0)),
            ("cell_begin > cell_end", INVALID, lambda: call([4, 2, 0], 5, 3, flags=0)),
            ("cell_end > n_cells", INVALID, lambda: call([4, 2, 0], 0, N_CELLS + 1, flags=0)),
            ("mask of another length", INVALID, lambda: call([4, 2, 0], 0, N_CELLS, outside=[0] * 6, flags=0)),
        ], good_bodies, fresh[good_bodies])
    for call in (eng.scene_fracture_impacts, eng.scene_fracture_impacts_async):
        check_refusals(eng, [
            ("K == 0", INVALID, lambda: call([], 0, N_CELLS, flags=0)),
            ("another K: fewer", STATE, lambda: call([[4, 2, 0]], 0, N_CELLS, flags=0)),
            ("another K: more", STATE, lambda: call([[4], [2], [0]], 0, N_CELLS, flags=0)),
            ("another K and a bad list", STATE, lambda: call([[4, 4], [2], []], 5, 3, flags=0)),
            ("an impact without a target", INVALID, lambda: call([[4, 0], []], 0, N_CELLS, flags=0)),
            ("compound out of range", INVALID, lambda: call([[4, 0], [6]], 0, N_CELLS, flags=0)),
            ("ascending inside an impact", INVALID, lambda: call([[0, 4], [2]], 0, N_CELLS, flags=0)),
            ("twice inside an impact", INVALID, lambda: call([[4, 4], [2]], 0, N_CELLS, flags=0)),
            ("a compound named in two impacts", INVALID, lambda: call([[4, 0], [0]], 0, N_CELLS, flags=0)),
            ("cell_begin > cell_end", INVALID, lambda: call(FRAME, 5, 3, flags=0)),
            ("cell_end > n_cells", INVALID, lambda: call(FRAME, 0, N_CELLS + 1, flags=0)),
            ("mask of another length", INVALID, lambda: call(FRAME, 0, N_CELLS, outside=[0] * 6, flags=0)),
        ], good_impacts, fresh[good_impacts])
    eng.close()


# ------------------------------------------------------------------ (a) 2. the outside entrances
def raw_outside(eng, compounds, n_sphere, points, origin, radius, cap, with_out=True):
    t, sp, org = arr(compounds, np.uint32), arr(points, np.float32), arr(origin, np.float32)
    n, out = u32(), np.zeros(64, np.uint8)
    return int(E_lib().surtr_scene_outside(eng._h, u32(0 if t is None else t.shape[0]), ptr(t), u32(n_sphere), ptr(sp), ptr(org), f32(radius), u32(cap),
                                           ctypes.byref(n), ptr(out) if with_out else None))


def raw_outside_impacts(eng, target_off, compounds, sphere_off, points, origins, radii, cap):
    to, t, so = arr(target_off, np.uint32), arr(compounds, np.uint32), arr(sphere_off, np.uint32)
    sp, org, rad = arr(points, np.float32), arr(origins, np.float32), arr(radii, np.float32)
    n, out = u32(), np.zeros(64, np.uint8)
    return int(E_lib().surtr_scene_outside_impacts(eng._h, u32(to.shape[0] - 1), ptr(to), ptr(t), ptr(so), ptr(sp), ptr(org), ptr(rad), u32(cap),
                                                   ctypes.byref(n), ptr(out)))


def E_lib():
    return engine.lib()


def good_outside(eng):
    return [eng.scene_outside(TB.CLICK_TARGETS, A["cloud"], A["origin"], A["radius"]).tobytes()]


def good_outside_impacts(eng):
    return [eng.scene_outside_impacts(FRAME, CLOUDS, ORIGINS, RADII).tobytes()]


def run_refusals_outside(E):
    eng = scene(E, None)                          # (the masks need no pattern and no placement)
    fresh = {good: good(eng) for good in (good_outside, good_outside_impacts)}
    assert len(fresh[good_outside][0]) == len(fresh[good_outside_impacts][0]) == 7 and 0 < sum(fresh[good_outside_impacts][0]) < 7
    eng.close()
    bare = E.Engine(0)
    assert code_of(lambda: bare.scene_outside([4, 2, 0], A["cloud"], A["origin"], A["radius"])) == STATE
    assert code_of(lambda: bare.scene_outside([99], A["cloud"], A["origin"], A["radius"])) == STATE
    assert code_of(lambda: bare.scene_outside([], A["cloud"], A["origin"], A["radius"])) == INVALID
    assert code_of(lambda: bare.scene_outside_impacts(FRAME, CLOUDS, ORIGINS, RADII)) == STATE
    assert code_of(lambda: bare.scene_outside_impacts([[4, 4], []], CLOUDS, ORIGINS, RADII)) == STATE
    assert code_of(lambda: bare.scene_outside_impacts([], [], [], [])) == INVALID
    bare.close()

    eng = scene(E, None)
    cloud, org, r = A["cloud"], A["origin"], A["radius"]
    check_refusals(eng, [
        ("no target", INVALID, lambda: eng.scene_outside([], cloud, org, r)),
        ("compound out of range", INVALID, lambda: eng.scene_outside([4, 6], cloud, org, r)),
        ("a capacity one short", CAPACITY, lambda: eng.scene_outside([4, 2, 0], cloud, org, r, capacity=6)),
        ("out of range and one short", INVALID, lambda: eng.scene_outside([4, 6], cloud, org, r, capacity=1)),
        ("points missing", INVALID, lambda: raw_outside(eng, [4, 2, 0], 64, None, org, r, 7)),
        ("origin missing", INVALID, lambda: raw_outside(eng, [4, 2, 0], 64, cloud, None, r, 7)),
        ("points missing and out of range", INVALID, lambda: raw_outside(eng, [6], 64, None, org, r, 7)),
    ], good_outside, fresh[good_outside])
    assert raw_outside(eng, [2, 4, 2], 64, cloud, org, r, 0, with_out=False) == 0      # (the mask's list may ascend and repeat: sizes only here)
    to, t, so = [0, 2, 3], [4, 0, 2], [0, 64, 128]
    pts, orgs = np.concatenate(CLOUDS), np.asarray(ORIGINS, np.float32)
    check_refusals(eng, [
        ("K == 0", INVALID, lambda: eng.scene_outside_impacts([], [], [], [])),
        ("an impact without a target", INVALID, lambda: eng.scene_outside_impacts([[4, 0], []], CLOUDS, ORIGINS, RADII)),
        ("compound out of range", INVALID, lambda: eng.scene_outside_impacts([[4, 0], [6]], CLOUDS, ORIGINS, RADII)),
        ("ascending inside an impact", INVALID, lambda: eng.scene_outside_impacts([[0, 4], [2]], CLOUDS, ORIGINS, RADII)),
        ("a compound named in two impacts", INVALID, lambda: eng.scene_outside_impacts([[4, 0], [0]], CLOUDS, ORIGINS, RADII)),
        ("a capacity one short", CAPACITY, lambda: eng.scene_outside_impacts(FRAME, CLOUDS, ORIGINS, RADII, capacity=6)),
        ("a bad list and one short", INVALID, lambda: eng.scene_outside_impacts([[4, 0], [0]], CLOUDS, ORIGINS, RADII, capacity=1)),
        ("target_off not from 0", INVALID, lambda: raw_outside_impacts(eng, [1, 2, 3], t, so, pts, orgs, RADII, 7)),
        ("sphere_off not from 0", INVALID, lambda: raw_outside_impacts(eng, to, t, [1, 64, 128], pts, orgs, RADII, 7)),
        ("sphere_off decreasing", INVALID, lambda: raw_outside_impacts(eng, to, t, [0, 64, 32], pts, orgs, RADII, 7)),
        ("sphere_off missing", INVALID, lambda: raw_outside_impacts(eng, to, t, None, pts, orgs, RADII, 7)),
        ("origins missing", INVALID, lambda: raw_outside_impacts(eng, to, t, so, pts, None, RADII, 7)),
        ("radii missing", INVALID, lambda: raw_outside_impacts(eng, to, t, so, pts, orgs, None, 7)),
        ("points missing while sphere_off[K] > 0", INVALID, lambda: raw_outside_impacts(eng, to, t, so, None, orgs, RADII, 7)),
        ("sphere_off decreasing and one short", INVALID, lambda: raw_outside_impacts(eng, to, t, [0, 64, 32], pts, orgs, RADII, 6)),
    ], good_outside_impacts, fresh[good_outside_impacts])
    assert raw_outside_impacts(eng, to, t, [0, 0, 0], None, orgs, RADII, 7) == 0        # no points and none asked for
    eng.close()


# ------------------------------------------------------------------ (a) 3. the regroup entrances
def raw_regroup(eng, bodies, partial, n_sphere, points, origin, radius, with_nc=True, with_nb=True):
    sp, org = arr(points, np.float32), arr(origin, np.float32)
    n, nc, nb = u32(), u32(), u32()
    head = (eng._h, ctypes.c_int(partial), u32(n_sphere), ptr(sp), ptr(org), f32(radius), ctypes.byref(n), ctypes.byref(nc) if with_nc else None, None, None)
    if bodies:
        return int(E_lib().surtr_event_regroup_bodies(*head, ctypes.byref(nb) if with_nb else None, None))
    return int(E_lib().surtr_event_regroup(*head))


def raw_regroup_impacts(eng, partial, k, sphere_off, points, origins, radii, with_nc=True):
    so, sp, org, rad = arr(sphere_off, np.uint32), arr(points, np.float32), arr(origins, np.float32), arr(radii, np.float32)
    n, nc, nb = u32(), u32(), u32()
    return int(E_lib().surtr_event_regroup_impacts(eng._h, ctypes.c_int(partial), u32(k), ptr(so), ptr(sp), ptr(org), ptr(rad), ctypes.byref(n),
                                                   ctypes.byref(nc) if with_nc else None, None, None, ctypes.byref(nb), None))


def regroup_bits(out):
    return [np.asarray(x).tobytes() for x in out]


def run_refusals_regroup(E):
    kw = dict(partial=True, sphere_points=A["cloud"], origin=A["origin"], radius=A["radius"])
    kwi = dict(partial=True, sphere_points=CLOUDS, origins=ORIGINS, radii=RADII)
    pts, orgs, so = np.concatenate(CLOUDS), np.asarray(ORIGINS, np.float32), [0, 64, 128]
    # ---- no event at all: SURTR_E_STATE, also with a second fault; a missing count pointer and K == 0 come first
    b = TS.bodies(E)
    eng = E.Engine(0)      # (the scene after click 1 still holds that click's fragments: an engine that never ran an event)
    eng.upload_pieces(b["meshes"][:2], b["convexes"][:2])
    for bodies in (False, True):
        assert raw_regroup(eng, bodies, 0, 0, None, None, 1.0) == STATE
        assert raw_regroup(eng, bodies, 1, 64, None, None, 1.0) == STATE
        assert raw_regroup(eng, bodies, 0, 0, None, None, 1.0, with_nc=False) == INVALID
    assert raw_regroup(eng, True, 0, 0, None, None, 1.0, with_nb=False) == INVALID
    assert raw_regroup_impacts(eng, 0, 2, None, None, None, None) == STATE
    assert raw_regroup_impacts(eng, 1, 2, [1, 0, 0], None, None, None) == STATE
    assert raw_regroup_impacts(eng, 0, 0, None, None, None, None) == INVALID
    eng.close()
    # ---- after a one-compound and after a bodies event
    eng = scene(E)
    for fracture in (lambda: eng.scene_fracture_event(2, 0, N_CELLS, outside=[1, 0, 0, 0, 1], flags=0),
                     lambda: eng.scene_fracture_bodies(TB.CLICK_TARGETS, 0, N_CELLS, outside=eng.scene_outside(TB.CLICK_TARGETS, *[kw[k] for k in ("sphere_points", "origin", "radius")]), flags=0)):
        fracture()
        want = regroup_bits(eng.event_regroup(**kw)) + regroup_bits(eng.event_regroup_bodies(**kw)) + regroup_bits(eng.event_regroup()) + \
            regroup_bits(eng.event_regroup_bodies())
        for name, code, call in [
                ("partial without an origin", INVALID, lambda: raw_regroup(eng, False, 1, 0, None, None, 1.0)),
                ("partial without an origin, bodies", INVALID, lambda: raw_regroup(eng, True, 1, 0, None, None, 1.0)),
                ("points missing", INVALID, lambda: raw_regroup(eng, False, 1, 64, None, A["origin"], 1.0)),
                ("points missing, bodies", INVALID, lambda: raw_regroup(eng, True, 1, 64, None, A["origin"], 1.0)),
                ("no count pointer", INVALID, lambda: raw_regroup(eng, True, 1, 64, None, A["origin"], 1.0, with_nc=False)),
                ("impacts regroup after another event", STATE, lambda: eng.event_regroup_impacts(n_impacts=2)),
                ("impacts regroup after another event, one impact", STATE, lambda: eng.event_regroup_impacts(n_impacts=1)),
                ("impacts regroup after another event, with spheres", STATE, lambda: eng.event_regroup_impacts(**kwi)),
                ("impacts regroup after another event, K == 0", INVALID, lambda: raw_regroup_impacts(eng, 0, 0, None, None, None, None))]:
            assert code_of(call) == code, name
            got = regroup_bits(eng.event_regroup(**kw)) + regroup_bits(eng.event_regroup_bodies(**kw)) + regroup_bits(eng.event_regroup()) + \
                regroup_bits(eng.event_regroup_bodies())
            assert got == want, ("after", name)
    eng.close()
    # ---- after an impacts event
    eng = scene(E)
    mask = eng.scene_outside_impacts(FRAME, CLOUDS, ORIGINS, RADII)
    eng.scene_fracture_impacts(FRAME, 0, N_CELLS, outside=mask, flags=0)

    def good(e):
        return regroup_bits(e.event_regroup_impacts(**kwi)) + regroup_bits(e.event_regroup_impacts(n_impacts=2)) + regroup_bits(e.event_regroup_bodies(**kw))
    check_refusals(eng, [
        ("K == 0", INVALID, lambda: raw_regroup_impacts(eng, 1, 0, so, pts, orgs, RADII)),
        ("another K: fewer", STATE, lambda: eng.event_regroup_impacts(partial=True, sphere_points=CLOUDS[:1], origins=ORIGINS[:1], radii=RADII[:1])),
        ("another K: more", STATE, lambda: eng.event_regroup_impacts(n_impacts=3)),
        ("another K and a bad sphere_off", STATE, lambda: raw_regroup_impacts(eng, 1, 3, [1, 0, 0, 0], None, None, None)),
        ("no count pointer", INVALID, lambda: raw_regroup_impacts(eng, 1, 2, so, pts, orgs, RADII, with_nc=False)),
        ("sphere_off missing", INVALID, lambda: raw_regroup_impacts(eng, 1, 2, None, pts, orgs, RADII)),
        ("origins missing", INVALID, lambda: raw_regroup_impacts(eng, 1, 2, so, pts, None, RADII)),
        ("radii missing", INVALID, lambda: raw_regroup_impacts(eng, 1, 2, so, pts, orgs, None)),
        ("sphere_off not from 0", INVALID, lambda: raw_regroup_impacts(eng, 1, 2, [1, 64, 128], pts, orgs, RADII)),
        ("sphere_off decreasing", INVALID, lambda: raw_regroup_impacts(eng, 1, 2, [0, 64, 32], pts, orgs, RADII)),
        ("points missing while sphere_off[K] > 0", INVALID, lambda: raw_regroup_impacts(eng, 1, 2, so, None, orgs, RADII)),
    ], good, good(eng))
    assert raw_regroup_impacts(eng, 0, 2, [1, 0, 0], None, None, None) == 0      # !partial: no sphere is read
    assert raw_regroup_impacts(eng, 1, 2, [0, 0, 0], None, orgs, RADII) == 0     # no points and none asked for
    eng.close()


# ------------------------------------------------------------------ (b) identities
def cycle(eng, fracture, regroup):
    """fracture -> regroup -> refit -> commit on one engine; everything that comes out, as bytes."""
    c = fracture(eng)
    out = [bytes(c), eng.download()["frag_ids"].tobytes(), eng.pair_order().tobytes()] + [regroup_bits(r(eng)) for r in regroup]
    eng.event_refit()
    out += event_bits(eng)
    co, cp = regroup[0](eng)[:2]
    out.append([np.asarray(x).tobytes() if hasattr(x, "__len__") else x for x in eng.scene_commit(co, cp)])
    return out


def run_identities(E):
    cells = (3, N_CELLS)
    kw = dict(partial=True, sphere_points=A["cloud"], origin=A["origin"], radius=A["radius"])
    kwi = dict(partial=True, sphere_points=[A["cloud"]], origins=[A["origin"]], radii=[A["radius"]])
    plain = [lambda e: e.event_regroup(**kw), lambda e: e.event_regroup_bodies(**kw)[:2], lambda e: e.event_regroup()]
    # ---- scene_fracture_bodies([c]) == scene_fracture_event(c): the five-piece compound, two of its pieces kept out
    a, b = scene(E, "plain"), scene(E, "plain")
    mask = a.scene_outside([2], A["cloud"], A["origin"], A["radius"])
    assert len(mask) == 5 and 0 < int(mask.sum()) < 5, mask
    ra = cycle(a, lambda e: e.scene_fracture_bodies([2], *cells, outside=mask, flags=0), plain)
    rb = cycle(b, lambda e: e.scene_fracture_event(2, *cells, outside=mask, flags=0), plain)
    assert ra == rb and ra[0] != bytes(engine.Counts())
    TB.assert_same_scene(a, b)
    a.close(); b.close()
    # ---- one impact == the bodies event: three targets, the mask of the click
    a, b = scene(E, None), scene(E, "plain")
    a.place_cells_impacts([A["scale"]], [A["translate"]])
    assert a.download_planes(impacts=True).tobytes() == b.download_planes().tobytes()
    mask = b.scene_outside(TB.CLICK_TARGETS, A["cloud"], A["origin"], A["radius"])
    assert a.scene_outside_impacts([TB.CLICK_TARGETS], [A["cloud"]], [A["origin"]], [A["radius"]]).tobytes() == mask.tobytes() and 0 < int(mask.sum()) < 7
    ra = cycle(a, lambda e: e.scene_fracture_impacts([TB.CLICK_TARGETS], *cells, outside=mask, flags=0),
               [lambda e: e.event_regroup_impacts(**kwi), lambda e: e.event_regroup_bodies(**kw), lambda e: e.event_regroup_impacts(n_impacts=1)])
    rb = cycle(b, lambda e: e.scene_fracture_bodies(TB.CLICK_TARGETS, *cells, outside=mask, flags=0),
               [lambda e: e.event_regroup_bodies(**kw), lambda e: e.event_regroup_bodies(**kw), lambda e: e.event_regroup_bodies()])
    assert ra == rb and ra[0] != bytes(engine.Counts())
    TB.assert_same_scene(a, b)
    a.close(); b.close()
    # ---- the whole-pattern forms the feature tests keep
    TB.run_one_target(E)
    TI.run_one_impact(E)


# ------------------------------------------------------------------ (c) state left behind
def run_state(E):
    eng = scene(E)
    plain0, inst0 = eng.download_planes().tobytes(), eng.download_planes(impacts=True).tobytes()
    assert len(inst0) == 2 * len(plain0) and inst0[:len(plain0)] == plain0 and inst0[len(plain0):] != plain0

    def commit_erases(targets, regroup):
        """Full fracture of `targets`: the commit keeps every other compound, in order, in front, and nothing of the targets."""
        table = [int(x) for x in eng.scene_compounds()]
        co, cp = regroup()[:2]
        eng.event_refit()
        n, first, n_new, src = eng.scene_commit(co, cp)
        kept = [p for c in range(len(table) - 1) if c not in targets for p in range(table[c], table[c + 1])]
        now = [int(x) for x in eng.scene_compounds()]
        assert first == len(table) - 1 - len(targets) and [int(s) for s in src[:now[first]]] == kept and (src[now[first]:] < 0).all()
        assert now[:first + 1] == list(np.cumsum([0] + [table[c + 1] - table[c] for c in range(len(table) - 1) if c not in targets]))
        made.append(n_new)
        assert len(now) - 1 >= 4      # (the next targets: the last compound and the third from last)
        return len(now) - 2, len(now) - 4
    made = []
    # an impacts event reads the instances and leaves the plain placement alone; so does its commit
    eng.scene_fracture_impacts(FRAME, 0, N_CELLS, flags=0)
    assert eng.download_planes().tobytes() == plain0 and eng.download_planes(impacts=True).tobytes() == inst0
    hi, lo = commit_erases([4, 2, 0], lambda: eng.event_regroup_impacts(n_impacts=2))
    assert eng.download_planes().tobytes() == plain0 and eng.download_planes(impacts=True).tobytes() == inst0
    # a plain event (bodies, then one compound) leaves the instances alone, and an impacts event after it still runs on them
    eng.scene_fracture_bodies([hi, lo], 0, N_CELLS, flags=0)
    assert eng.download_planes().tobytes() == plain0 and eng.download_planes(impacts=True).tobytes() == inst0
    hi, lo = commit_erases([hi, lo], eng.event_regroup_bodies)
    eng.scene_fracture_event(lo, 0, N_CELLS, flags=0)
    hi, lo = commit_erases([lo], eng.event_regroup)
    assert eng.download_planes().tobytes() == plain0 and eng.download_planes(impacts=True).tobytes() == inst0
    eng.scene_fracture_impacts([[lo], [hi]], 0, N_CELLS, flags=0)
    hi, lo = commit_erases([lo, hi], lambda: eng.event_regroup_impacts(n_impacts=2))
    # a refused event leaves the targets of the pending one to the commit
    eng.scene_fracture_bodies([hi, lo], 0, N_CELLS, flags=0)
    assert code_of(lambda: eng.scene_fracture_bodies([lo, hi], 0, N_CELLS, flags=0)) == INVALID
    assert code_of(lambda: eng.scene_fracture_impacts([[lo], []], 0, N_CELLS, flags=0)) == INVALID
    commit_erases([hi, lo], eng.event_regroup_bodies)
    print("compounds made per commit:", made)
    assert made[0] >= 3
    # a new placement of the pattern keeps the instances; a new pattern drops them
    eng.place_cells(B["scale"], B["translate"])
    assert eng.download_planes().tobytes() == inst0[len(plain0):] and eng.download_planes(impacts=True).tobytes() == inst0
    cube = TS.bodies(E)["cube"]
    eng.upload_pattern(cube["face_off"], cube["v012"])
    assert code_of(lambda: eng.download_planes(impacts=True)) == STATE
    assert code_of(lambda: eng.scene_fracture_impacts([[1], [0]], 0, N_CELLS, flags=0)) == STATE
    eng.close()


CASES = ["refusals_fracture", "refusals_outside", "refusals_regroup", "identities", "state"]


# ------------------------------------------------------------------ CPU tier (emulation)
@pytest.mark.parametrize("case", CASES)
def test_scene_entrances(emul_engine, case):
    globals()["run_" + case](emul_engine)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_scene_entrances as T
    case = sys.argv[1]
    getattr(T, "run_" + case)(engine)
    print("ok", case)
""")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_gpu_scene_entrances(case):
    run_gpu_child(GPU_CHILD, case, 90)
