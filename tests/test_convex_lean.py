"""k_clip_convex_lean (the Convex clip with small_clip + sc_park alone) and k_clip_convex as its second tier, against the oracle and
against the one-kernel arrangement (SURTR_CVX_LEAN=0 / 1, read by plan_event on every event).

Every case runs the same event with the switch at 0 and at 1, compares both with the CPU oracle and the two with each other
array by array, bit for bit.  surtr_queue_stats: [80] Convexes small_clip took, [81] handed on / started on the literal clipper,
[87] pairs the lean kernel gave up (what its second tier clipped).

  (a) the 2 562-vertex blob and its ACH x 64 cells: every pair finishes in the lean kernel;
  (b) a cube piece with a cell plane exactly through three corners of its Convex (coordinates exact in float): an in-plane vertex,
      so small_clip hands on (SC_FALLBACK) and the pair is the second tier's;
  (c) a Convex of 642 vertices (an icosphere) x 8 cells: beyond small_clip's solid, every pair given up;
  (d) a Convex whose rings list a neighbour twice (cdup): literal clipper first, through the second tier;
  (e) (a)- and (b)-type pieces in one event, with the Convex clip beside the pre-pass (SURTR_FRONT_PAR=1) and ahead of it (=0):
      both tiers write records and queue entries that the pre-pass and the clip kernels read;
  (f) a small event on six contexts in one process (tests/inflight_driver.py's arrangement).
The GPU tier runs all of them on the device; the CPU tier runs the same functions on the single-lane emulation."""
import contextlib
import os

import numpy as np
import pytest

from helpers import assert_event_equal, assert_event_equal_flagged
from surtr_amd import meshgen, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
Q_TOOK, Q_HANDED, Q_GAVE_UP = 80, 81, 87
E = 6


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


def _assert_identical(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), k


def _event(engine_mod, meshes, convexes, n_cells, lean, planes=None, pattern=None, front_par=None):
    """One event of all (cell, piece) pairs with the switch at `lean`; returns (counts, fragments, queue_stats, pair status)."""
    with _env(SURTR_CVX_LEAN=lean, SURTR_FRONT_PAR=front_par):
        eng = engine_mod.Engine(0)
        try:
            eng.upload_pieces(meshes, convexes)
            if planes is not None:
                eng.upload_planes(planes[0], planes[1])
            else:
                eng.upload_pattern(pattern["face_off"], pattern["v012"])
                eng.place_cells(pattern["scale"], pattern["translate"])
            c = eng.fracture_event(0, n_cells, flags=3)
            got = eng.download()
            qs = np.array(eng.queue_stats(), np.int64)
            ps = eng.pair_status(n_cells * len(meshes))
        finally:
            eng.close()
    return c, got, qs, ps


def _both(engine_mod, ref, meshes, convexes, n_cells, flagged=False, **kw):
    """The event with the switch at 0 and at 1: each against the oracle's `ref`, and the two against each other.  Returns the
    queue_stats of the two runs."""
    runs = [_event(engine_mod, meshes, convexes, n_cells, lean, **kw) for lean in (0, 1)]
    for c, got, qs, ps in runs:
        assert c.status == 0
        if flagged:
            g = dict(got)
            g["flagged_pairs"] = [(int(j) // len(meshes), int(j) % len(meshes)) for j in np.nonzero(ps)[0]]
            assert_event_equal_flagged(g, ref)
        else:
            assert c.n_failed == 0
            assert_event_equal(got, ref)
    _assert_identical(runs[0][1], runs[1][1])
    assert runs[0][3].tolist() == runs[1][3].tolist()
    assert runs[0][2][Q_GAVE_UP] == 0      # (the one-kernel arrangement has no list)
    # what small_clip took and handed on is counted once per pair in either arrangement
    assert runs[0][2][Q_TOOK] == runs[1][2][Q_TOOK] and runs[0][2][Q_HANDED] == runs[1][2][Q_HANDED]
    return runs[0][2], runs[1][2]


# ------------------------------------------------------------------------------------------------------------------ the scenes
_cache = {}


def _blob_scene(engine_mod, oracle):
    """(a): the blob, its ACH (built on the engine under test, as bench.py builds the flagship's) and 64 Voronoi cells."""
    sc = scenes.blob_scene(64)
    eng = engine_mod.Engine(0)
    try:
        sc["convex"], _ = scenes.ach_convex(eng, sc["mesh"]["pos"])
    finally:
        eng.close()
    key = ("blob", sc["convex"]["pos"].tobytes())
    if key not in _cache:
        planes = oracle.place_cells(sc["v012"], sc["scale"], sc["translate"])
        _cache[key] = oracle.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=True, render=True, threads=8)
    return sc, _cache[key]


def _box_cell(extra, lim=3.0):
    """A cell: the planes `extra` first, then the box |x|, |y|, |z| < lim.  (inside: n . x + w < 0)"""
    return list(extra) + [[1, 0, 0, -lim], [-1, 0, 0, -lim], [0, 1, 0, -lim], [0, -1, 0, -lim], [0, 0, 1, -lim], [0, 0, -1, -lim]]


def _cells(cells):
    off, planes = [0], []
    for c in cells:
        planes += c
        off.append(len(planes))
    return np.array(off, np.uint32), np.array(planes, np.float32)


def _cube_piece():
    """(b): the cube [-1, 1]^3 with the box [-2, 2]^3 as its Convex.  The plane x + y + z = 2 goes through the corners (2, 2, -2),
    (2, -2, 2), (-2, 2, 2) of the Convex, cuts (2, 2, 2) off and keeps the other four; every term of the plane distance is an
    integer, so the three are in the plane exactly.  No vertex of the cube is (x + y + z is odd there)."""
    from surtr_amd import engine
    v, t = meshgen.cube(1.0)
    return engine.neighbors_from_mesh(v, t), scenes.box_solid([2, 2, 2], [0, 0, 0])


DIAGONAL = [_box_cell([[1, 1, 1, -2]]), _box_cell([[-1, -1, -1, 2]])]
QUADRANTS = [_box_cell([[sx, 0, 0, -sx * 0.25], [0, sy, 0, -sy * 0.25]]) for sx in (1, -1) for sy in (1, -1)]


# ------------------------------------------------------------------------------------------------------------------- the cases
def check_all_lean(engine_mod, oracle):
    sc, ref = _blob_scene(engine_mod, oracle)
    assert sc["convex"]["pos"].shape[0] > 8      # (an ACH, not the box)
    q0, q1 = _both(engine_mod, ref, [sc["mesh"]], [sc["convex"]], 64, pattern=sc)
    assert q1[Q_GAVE_UP] == 0 and q1[Q_TOOK] == 64 and q1[Q_HANDED] == 0, (q1[Q_GAVE_UP], q1[Q_TOOK], q1[Q_HANDED])


def check_in_plane_vertex(engine_mod, oracle):
    mesh, conv = _cube_piece()
    off, planes = _cells(DIAGONAL)
    ref = oracle.event([mesh], [conv], off, planes, refit=True, render=True)
    assert ref["frag_ids"].shape[0] == 2
    q0, q1 = _both(engine_mod, ref, [mesh], [conv], 2, planes=(off, planes))
    assert q1[Q_GAVE_UP] >= 1 and q1[Q_HANDED] == q1[Q_GAVE_UP], (q1[Q_GAVE_UP], q1[Q_HANDED])


def check_beyond_capacity(engine_mod, oracle):
    from surtr_amd import engine
    v, t = meshgen.icosphere(3)
    v, t = meshgen._outward(v.astype(np.float32), t)
    solid = engine.neighbors_from_mesh(v, t)
    assert solid["pos"].shape[0] == 642
    sc = scenes.make_scene(v, t, 8)
    planes = oracle.place_cells(sc["v012"], sc["scale"], sc["translate"])
    ref = oracle.event([solid], [solid], sc["face_off"], planes, refit=True, render=True)
    q0, q1 = _both(engine_mod, ref, [solid], [solid], 8, pattern=sc)
    assert q1[Q_GAVE_UP] == 8 and q1[Q_TOOK] == 0 and q1[Q_HANDED] == 8, (q1[Q_GAVE_UP], q1[Q_TOOK], q1[Q_HANDED])


def check_doubled_neighbour(engine_mod, oracle):
    """tests/golden/sliver_convex_walk_bound.npz: a seven-vertex Convex with doubled neighbours, and the cell it met.  Cell 0 is that
    cell (no fragment, see test_literal_clip), cell 1 its first plane alone."""
    from helpers import solid_has_doubled_neighbour
    d = np.load(os.path.join(HERE, "golden", "sliver_convex_walk_bound.npz"))
    mesh = {"pos": d["mesh_pos"], "off": d["mesh_off"], "nbr": d["mesh_nbr"]}
    conv = {"pos": d["conv_pos"], "off": d["conv_off"], "nbr": d["conv_nbr"]}
    assert solid_has_doubled_neighbour(conv)
    pl = np.asarray(d["planes"], np.float32).reshape(-1, 4)
    off, planes = _cells([pl.tolist(), pl[:1].tolist()])
    ref = oracle.event([mesh], [conv], off, planes, refit=True, render=True)
    q0, q1 = _both(engine_mod, ref, [mesh], [conv], 2, planes=(off, planes), flagged=True)
    assert q1[Q_GAVE_UP] == 2 and q1[Q_TOOK] == 0 and q1[Q_HANDED] == 2, (q1[Q_GAVE_UP], q1[Q_TOOK], q1[Q_HANDED])


def check_mixed(engine_mod, oracle, front_par):
    from surtr_amd import engine
    cube_mesh, cube_conv = _cube_piece()
    v, t = meshgen.blob(scale=1.0)
    blob_mesh = engine.neighbors_from_mesh(v, t)
    eng = engine_mod.Engine(0)
    try:
        blob_conv, _ = scenes.ach_convex(eng, blob_mesh["pos"])
    finally:
        eng.close()
    meshes, convexes = [cube_mesh, blob_mesh], [cube_conv, blob_conv]
    off, planes = _cells(DIAGONAL + QUADRANTS)
    key = ("mixed", blob_conv["pos"].tobytes())
    if key not in _cache:
        _cache[key] = oracle.event(meshes, convexes, off, planes, refit=True, render=True, threads=8)
    q0, q1 = _both(engine_mod, _cache[key], meshes, convexes, 6, planes=(off, planes), front_par=front_par)
    # the cube's Convex has vertices in the diagonal plane of cells 0 and 1; the other ten pairs are regular
    assert 1 <= q1[Q_GAVE_UP] <= 2 and q1[Q_TOOK] == 12 - q1[Q_GAVE_UP], (q1[Q_GAVE_UP], q1[Q_TOOK])


def check_six_contexts(engine_mod, oracle, emul_lib):
    """bench.py's arrangement, small: bumpy_torus(100, 60) x 256 cells, six engines, two rounds, every blob against the event of one
    context alone (tests/inflight_driver.py, which checks that one against the oracle) -- with the lean arrangement; and that event
    with the switch at 0 and at 1."""
    import inflight_driver
    eng = engine_mod.Engine(0)
    try:
        sc = inflight_driver._bench_scene(engine_mod, scenes, meshgen, eng, (100, 60), 256)
    finally:
        eng.close()
    runs = [_event(engine_mod, [sc["mesh"]], [sc["convex"]], 256, lean, pattern=sc) for lean in (0, 1)]
    assert runs[0][0].status == 0 and runs[1][0].status == 0
    _assert_identical(runs[0][1], runs[1][1])
    assert runs[1][2][Q_TOOK] + runs[1][2][Q_HANDED] == 256 and runs[1][2][Q_GAVE_UP] == runs[1][2][Q_HANDED]
    with _env(SURTR_CVX_LEAN=1):
        rep = inflight_driver.run("whole", 2, E, emul_lib=emul_lib, torus=(100, 60), n_cells=256, threads=8)
    assert rep["error"] is None and not rep["bad"], (rep["error"], rep["bad"][:3])
    assert rep["events_checked"] == rep["events_ok"] == 2 * E and rep["pass_b"]["events_ok"] == 2 * E and rep["ok"]


# -------------------------------------------------------------------------------------------------------------------- GPU tier
@pytest.mark.gpu
def test_all_lean_gpu(gpu_engine, oracle):
    check_all_lean(gpu_engine, oracle)


@pytest.mark.gpu
def test_in_plane_vertex_second_tier_gpu(gpu_engine, oracle):
    check_in_plane_vertex(gpu_engine, oracle)


@pytest.mark.gpu
def test_beyond_capacity_second_tier_gpu(gpu_engine, oracle):
    check_beyond_capacity(gpu_engine, oracle)


@pytest.mark.gpu
def test_doubled_neighbour_second_tier_gpu(gpu_engine, oracle):
    check_doubled_neighbour(gpu_engine, oracle)


@pytest.mark.gpu
@pytest.mark.parametrize("front_par", [0, 1])
def test_mixed_event_both_tiers_gpu(gpu_engine, oracle, front_par):
    check_mixed(gpu_engine, oracle, front_par)


@pytest.mark.gpu
def test_six_contexts_gpu(gpu_engine, oracle):
    check_six_contexts(gpu_engine, oracle, None)


# -------------------------------------------------------------------------------------------------------------------- CPU tier
def test_all_lean_emulation(emul_engine, oracle):
    check_all_lean(emul_engine, oracle)


def test_in_plane_vertex_second_tier_emulation(emul_engine, oracle):
    check_in_plane_vertex(emul_engine, oracle)


def test_beyond_capacity_second_tier_emulation(emul_engine, oracle):
    check_beyond_capacity(emul_engine, oracle)


def test_doubled_neighbour_second_tier_emulation(emul_engine, oracle):
    check_doubled_neighbour(emul_engine, oracle)


@pytest.mark.parametrize("front_par", [0, 1])
def test_mixed_event_both_tiers_emulation(emul_engine, oracle, front_par):
    check_mixed(emul_engine, oracle, front_par)


def test_six_contexts_emulation(emul_engine, emul_lib_path, oracle):
    check_six_contexts(emul_engine, oracle, emul_lib_path)
