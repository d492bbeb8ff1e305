"""The grids of an event's persistent queue kernels with several events in flight (plan_event's many-mode sizes).

k_clip_convex_lean and its second tier, k_clip_pairs_catch and its sweep, k_clip_pairs_big, k_refit and both tiers of k_faces take
their tasks from a queue: any grid of one workgroup or more must give the same event.  A context told that it is one of several
(set_events_in_flight(6)) reads one override per grid (SURTR_CVX_LEAN_WG_MANY, SURTR_CVX2_WG_MANY, SURTR_CATCH_WG_MANY,
SURTR_SWEEP_WG_MANY, SURTR_BIG_WG_MANY, SURTR_REFIT_WG_BOTH, SURTR_FACES_WG_BOTH, SURTR_FACES2_WG_MANY); the tests set every grid
to 1, to 2, to an odd value below the task count and to a value above it and compare every array, count and status with the default
grids' (bit for bit) and with the oracle's.  Engine.event_plan says which grids the event really took.

Shapes, the smallest at which such a kernel can go wrong (more tasks than workgroups, fewer, one workgroup for everything):
  blob    the 2 562-vertex blob with its ACH x 64 cells
  torus   meshgen.bumpy_torus(64, 40), 2 560 vertices (the pre-pass kernel and the record clipper take it) x 256 cells
Both with SURTR_CVX_LEAN=1 (at this size the plan would take the one-kernel Convex clip) and a first k_faces tier of 192 half-edges
(SURTR_FACES_TIER_HE), so that the lean kernel and the second tier of k_faces run and have fragments to work on.

The plans that must not change: a context alone on the GPU ignores the new overrides; a small event (Convex clip beside the
pre-pass), the general clipper arrangement and a context alone get the same grids as before, and the event that does queue up on the
lean arrangement never gets a larger grid than a context alone.

One more case runs tests/inflight_driver.py: six contexts, two rounds, small grids, every blob against the one-at-a-time event.
The GPU tier runs each case in a child process under a time limit (helpers.run_gpu_child); the CPU tier in-process on the emulation."""
import contextlib
import os
import sys
import time

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
for _d in (os.path.dirname(HERE), HERE):
    if _d not in sys.path:
        sys.path.insert(0, _d)

from helpers import assert_event_equal, run_gpu_child      # noqa: E402
from surtr_amd import meshgen, scenes      # noqa: E402

E = 6
CHILD_SECONDS = 240      # (a case takes a few seconds: the limit is for a kernel that does not end)
BASE_ENV = {"SURTR_CVX_LEAN": 1, "SURTR_FACES_TIER_HE": 192}
SHAPES = {"blob": 64, "torus": 256}
SETTINGS = ("one", "two", "odd", "above")
# plan field -> override, in the order of the kernels in launch_event
GRIDS = (("n_wg_lean", "SURTR_CVX_LEAN_WG_MANY"), ("n_wg_cvx2", "SURTR_CVX2_WG_MANY"), ("n_wg_big", "SURTR_BIG_WG_MANY"),
         ("n_catch", "SURTR_CATCH_WG_MANY"), ("n_wg_sweep", "SURTR_SWEEP_WG_MANY"), ("g_refit", "SURTR_REFIT_WG_BOTH"),
         ("g_faces", "SURTR_FACES_WG_BOTH"), ("g_faces2", "SURTR_FACES2_WG_MANY"))
MANY_ONLY = [v for _, v in GRIDS if v.endswith("_MANY")]


@contextlib.contextmanager
def _env(**kw):
    old = {k: os.environ.get(k) for k in kw}
    try:
        for k, v in kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_cache = {}


def _scene(engine_mod, oracle, shape):
    """The scene and the oracle's event, once per shape (the ACH and the cells come from the engine under test, as bench.py's)."""
    import inflight_driver
    n_cells = SHAPES[shape]
    eng = engine_mod.Engine(0)
    try:
        if shape == "blob":
            sc = scenes.blob_scene(n_cells)
            sc["convex"], _ = scenes.ach_convex(eng, sc["mesh"]["pos"])
        else:
            sc = inflight_driver._bench_scene(engine_mod, scenes, meshgen, eng, (64, 40), n_cells)
            assert sc["mesh"]["pos"].shape[0] == 2560
    finally:
        eng.close()
    key = (shape, sc["convex"]["pos"].tobytes(), np.asarray(sc["v012"]).tobytes())
    if key not in _cache:
        planes = oracle.place_cells(sc["v012"], sc["scale"], sc["translate"])
        _cache[key] = oracle.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=True, render=True, threads=8)
    return sc, _cache[key]


def _event(engine_mod, sc, n_cells, in_flight, env):
    """One event of all pairs on a fresh context with the hint at `in_flight`; returns counts, arrays, pair status and the plan."""
    with _env(**env):
        eng = engine_mod.Engine(0)
        try:
            eng.set_events_in_flight(in_flight)
            eng.upload_pieces([sc["mesh"]], [sc["convex"]])
            eng.upload_pattern(sc["face_off"], sc["v012"])
            eng.place_cells(sc["scale"], sc["translate"])
            c = eng.fracture_event(0, n_cells, flags=3)
            got = eng.download()
            ps = eng.pair_status(n_cells)
            qs = np.array(eng.queue_stats(), np.int64)
            plan = eng.event_plan(n_cells, flags=3)
            # what the context has room for: an event of very many pairs fills every grid (the Convex kernels' scratch is k_refit's)
            room = eng.event_plan(1 << 20, flags=3)
            plan["lean_cap"], plan["refit_cap"] = room["n_wg_lean"], room["n_wg_cvx"]
        finally:
            eng.close()
    return c, got, ps, plan, qs


def _values(setting, plan, n_pairs, n_frag):
    """The grid of every queue kernel for one setting.  Tasks: the pairs for the Convex clip, the fragments for refit and faces;
    what the second tiers, the catcher and k_clip_pairs_big get is a handful, so their "above" is the most they have scratch for.
    (The emulation's device has one compute unit and room for eight and five workgroups where the MI355X has room for thousands:
    there "above" is all the room there is.)"""
    # (k_faces has scratch for twice its default grid beside the refit: all of it on the device, a handful of slices on the emulation)
    faces_cap = 2 * plan["g_faces"]
    if setting in ("one", "two"):
        v = {f: 1 if setting == "one" else 2 for f, _ in GRIDS}
    elif setting == "odd":
        v = {"n_wg_lean": 7, "n_wg_cvx2": 3, "n_wg_big": 3, "n_catch": 3, "n_wg_sweep": 3, "g_refit": 7, "g_faces": min(5, faces_cap - 1),
             "g_faces2": min(3, plan["g_faces2"])}
        assert 7 < n_pairs and 7 < n_frag and v["g_faces"] % 2 == 1
    else:
        v = {"n_wg_lean": min(n_pairs + 5, plan["lean_cap"]), "n_wg_cvx2": min(64, plan["refit_cap"]), "n_wg_big": plan["n_wg_big"], "n_catch": 32,
             "n_wg_sweep": 32, "g_refit": min(n_frag + 3, plan["refit_cap"]), "g_faces": min(n_frag + 3, faces_cap), "g_faces2": plan["g_faces2"]}
    return v


def check_grids(engine_mod, oracle, shape):
    sc, ref = _scene(engine_mod, oracle, shape)
    n_cells = SHAPES[shape]
    base = dict(BASE_ENV, **{v: None for _, v in GRIDS})
    c0, got0, ps0, plan0, qs0 = _event(engine_mod, sc, n_cells, E, base)
    assert c0.status == 0 and c0.n_failed == 0
    assert_event_equal(got0, ref)
    n_frag = int(c0.n_frag)
    # the arrangement under test: record clipper + catcher, the lean Convex kernel and its second tier, both tiers of k_faces
    assert plan0["wave"] and plan0["split"] and plan0["cvx_lean"] and plan0["both"] and plan0["g_faces2"] > 0, plan0
    assert plan0["prep_kind"] == 2, plan0
    assert qs0[85] > 0, "no fragment reached the second tier of k_faces"
    for setting in SETTINGS:
        want = _values(setting, plan0, n_cells, n_frag)
        env = dict(base, **{var: want[f] for f, var in GRIDS})
        c, got, ps, plan, qs = _event(engine_mod, sc, n_cells, E, env)
        assert {f: plan[f] for f, _ in GRIDS} == want, (setting, plan)
        for f in plan:      # nothing else of the plan moves
            if f not in want and not f.endswith("_cap"):
                assert plan[f] == plan0[f], (setting, f, plan[f], plan0[f])
        assert (c.status, c.n_failed, c.n_frag) == (0, 0, n_frag), (setting, c.status, c.n_failed, c.n_frag)
        assert sorted(got) == sorted(got0)
        for k in got0:
            assert got[k].shape == got0[k].shape and got[k].dtype == got0[k].dtype and np.array_equal(got[k], got0[k]), (setting, k)
        assert ps.tolist() == ps0.tolist(), setting
        for f in ("n_frag", "mesh_verts", "mesh_nbrs", "conv_verts", "conv_nbrs", "n_idx"):
            assert getattr(c, f) == getattr(c0, f), (setting, f)
        assert_event_equal(got, ref)
        # the same pairs and fragments went the same ways: Convexes small_clip took / handed on, pairs given up, second-tier fragments
        for q in (80, 81, 85, 87, 88, 89):
            assert qs[q] == qs0[q], (setting, q, qs[q], qs0[q])


def check_plans(engine_mod, oracle):
    """What must not change, on the blob's context after one event (the plan reads the capacities that event set)."""
    sc, _ = _scene(engine_mod, oracle, "blob")
    n_cells = SHAPES["blob"]
    grid_fields = [f for f, _ in GRIDS]
    small = {v: 1 for v in MANY_ONLY}

    def plans(in_flight, env, sizes):
        with _env(**env):
            eng = engine_mod.Engine(0)
            try:
                eng.set_events_in_flight(in_flight)
                eng.upload_pieces([sc["mesh"]], [sc["convex"]])
                eng.upload_pattern(sc["face_off"], sc["v012"])
                eng.place_cells(sc["scale"], sc["translate"])
                assert eng.fracture_event(0, n_cells, flags=3).status == 0
                return [eng.event_plan(n, flags=3) for n in sizes]
            finally:
                eng.close()

    sizes = (n_cells, 700, 4096, 20000)
    none = {v: None for _, v in GRIDS}
    alone = plans(1, none, sizes)
    # a context alone on the GPU: the overrides of the several-events grids are not read, no plan has the many-mode grids
    assert plans(1, dict(none, **small), sizes) == alone
    assert not any(p["many_grids"] for p in alone)
    several = plans(E, none, sizes)
    for a, s in zip(alone, several):
        if s["front_par"]:
            # a small event: the Convex clip beside the pre-pass; its grids are those of a context alone
            assert s["n_pairs"] <= 1024 and not s["many_grids"], s
            assert [s[f] for f in grid_fields] == [a[f] for f in grid_fields], (s, a)
        else:
            # an event that queues up on the lean arrangement: never a larger grid than alone, never an empty one
            assert s["many_grids"] and s["wave"] and s["split"], s
            for f in grid_fields:
                assert (1 <= s[f] <= a[f]) or (f == "g_faces2" and s[f] == a[f] == 0), (f, s, a)
            # the rule: one workgroup of k_clip_pairs_big per 128 pairs, three of the lean Convex kernel per eight; the others kept
            n = s["n_pairs"]
            assert s["n_wg_big"] == max(1, min(a["n_wg_big"], (n + 127) // 128)), (s, a)
            assert s["n_wg_lean"] == max(1, min(a["n_wg_lean"], (3 * n + 7) // 8)), (s, a)
            assert [s[f] for f in grid_fields if f not in ("n_wg_big", "n_wg_lean")] == \
                [a[f] for f in grid_fields if f not in ("n_wg_big", "n_wg_lean")], (s, a)
        assert s["n_wg"] == a["n_wg"] and s["n_wg_prep"] == a["n_wg_prep"], (s, a)      # the kernels with the real work keep theirs
    assert several[0]["front_par"] and several[1]["front_par"] and not several[2]["front_par"] and not several[3]["front_par"]
    # the general clipper arrangement keeps its plan as well
    general = plans(E, dict(none, SURTR_WAVE=0), sizes)
    general_alone = plans(1, dict(none, SURTR_WAVE=0), sizes)
    for g, a in zip(general, general_alone):
        assert not g["wave"] and not g["many_grids"], g
        assert [g[f] for f in grid_fields] == [a[f] for f in grid_fields], (g, a)


def check_six_contexts(engine_mod, emul_lib):
    """Six contexts, two rounds of the torus x 256 cells with small grids everywhere: every blob equals the one-at-a-time event
    (which tests/inflight_driver.py checks against the oracle)."""
    import inflight_driver
    env = dict(BASE_ENV, SURTR_CVX_LEAN_WG_MANY=5, SURTR_CVX2_WG_MANY=2, SURTR_BIG_WG_MANY=2, SURTR_CATCH_WG_MANY=3, SURTR_SWEEP_WG_MANY=1,
               SURTR_REFIT_WG_BOTH=7, SURTR_FACES_WG_BOTH=5, SURTR_FACES2_WG_MANY=2)
    with _env(**env):
        rep = inflight_driver.run("whole", 2, E, emul_lib=emul_lib, torus=(64, 40), n_cells=256, threads=8)
    assert rep["error"] is None and not rep["bad"], (rep["error"], rep["bad"][:3])
    assert rep["events_checked"] == rep["events_ok"] == 2 * E and rep["pass_b"]["events_ok"] == 2 * E and rep["ok"]


# -------------------------------------------------------------------------------------------------------------------- GPU tier
GPU_CHILD = """
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import test_inflight_grids as T
T.gpu_case(sys.argv[1])
"""


def gpu_case(case):
    from surtr_amd import engine
    from oracle import oracle
    t = time.time()
    engine._use_library_for_tests(None)
    if case in SHAPES:
        check_grids(engine, oracle, case)
    elif case == "plans":
        check_plans(engine, oracle)
    else:
        assert case == "six"
        check_six_contexts(engine, None)
    print("ok %s (%.1f s)" % (case, time.time() - t))


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(SHAPES) + ["plans", "six"])
def test_inflight_grids_gpu(case):
    run_gpu_child(GPU_CHILD, case, CHILD_SECONDS)


# -------------------------------------------------------------------------------------------------------------------- CPU tier
@pytest.mark.parametrize("shape", list(SHAPES))
def test_inflight_grids_emulation(emul_engine, oracle, shape):
    check_grids(emul_engine, oracle, shape)


def test_inflight_plans_emulation(emul_engine, oracle):
    check_plans(emul_engine, oracle)


def test_inflight_grids_six_contexts_emulation(emul_engine, emul_lib_path):
    check_six_contexts(emul_engine, emul_lib_path)
