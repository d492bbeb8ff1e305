"""A failed device allocation leaves the context sound (CPU emulation).

The emulation's hipMalloc can fail on a chosen call (tests/emul/hip_emul.h).  The sweep fails every allocation of a fixed
sequence in turn -- an event with REFIT | RENDER and its download, regroup, build_cells, neighbors_from_mesh, clip_polyhedron and
extract_faces, so that every translation unit that allocates does so -- and checks for each: the failing call reports
SURTR_E_HIP, the same sequence on the same engine then gives the clean results (the event against the oracle), and closing the
engine frees every allocation with the red zones round it intact (surtr_emul_guard_check).  It runs once more with a small faces tier, so that the second tier of k_faces is swept too.

The sweep runs in a child process under a time limit: a crash there fails this test instead of ending pytest."""
import ctypes
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
if os.path.join(ROOT, "tests") not in sys.path:
    sys.path.insert(0, os.path.join(ROOT, "tests"))

# an octahedron as a triangle mesh (neighbors_from_mesh) and two planes through it (clip_polyhedron)
_OCTA_POS = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], np.float32)
_OCTA_TRIS = np.array([[0, 2, 4], [2, 1, 4], [1, 3, 4], [3, 0, 4], [2, 0, 5], [1, 2, 5], [3, 1, 5], [0, 3, 5]], np.int32)
_PLANES = np.array([[1, 0, 0, -0.1], [0, 1, 0, 0.05]], np.float32)


def _sequence(eng, sc):
    from surtr_amd import engine
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, sc["n_cells"], flags=engine.EVT_REFIT | engine.EVT_RENDER)
    out = {"event": eng.download()}
    out["regroup"] = eng.event_regroup()
    out["cells"] = eng.build_cells(sc["seeds"])
    out["neighbors"] = eng.neighbors_from_mesh(_OCTA_POS, _OCTA_TRIS)[0]
    out["clip"] = eng.clip_polyhedron(sc["mesh"], _PLANES)
    out["faces"] = eng.extract_faces(sc["mesh"])
    return out


def _same(a, b):
    if isinstance(a, dict):
        return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return np.array_equal(np.asarray(a), np.asarray(b))


def _sweep(lib_path):
    from surtr_amd import engine, scenes
    from oracle import oracle
    from helpers import assert_event_equal
    engine._use_library_for_tests(lib_path)
    L = ctypes.CDLL(lib_path)
    L.surtr_emul_live_allocs.restype = ctypes.c_long
    L.surtr_emul_alloc_calls.restype = ctypes.c_long
    L.surtr_emul_fail_alloc.argtypes = [ctypes.c_long]
    L.surtr_emul_guard_check.restype = ctypes.c_long      # (damaged red zones round the device blocks, freed ones included)
    sc = scenes.cube_scene(8)
    planes = oracle.place_cells(sc["v012"], sc["scale"], sc["translate"])
    ref = oracle.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=True, render=True)

    live0 = L.surtr_emul_live_allocs()
    L.surtr_emul_fail_alloc(-1)
    eng = engine.Engine(0)
    clean = _sequence(eng, sc)
    eng.close()
    n_alloc = L.surtr_emul_alloc_calls()
    assert_event_equal(clean["event"], ref)
    assert L.surtr_emul_live_allocs() == live0
    assert L.surtr_emul_guard_check() == 0
    for k in range(n_alloc):
        L.surtr_emul_fail_alloc(k)
        eng = None
        try:
            eng = engine.Engine(0)
            _sequence(eng, sc)
            raise AssertionError("allocation %d of %d failed and no call reported it" % (k, n_alloc))
        except engine.SurtrError as e:
            assert e.code == engine.E_HIP, (k, e)
        L.surtr_emul_fail_alloc(-1)
        if eng is None:
            eng = engine.Engine(0)      # (the failure was surtr_create's own)
        again = _sequence(eng, sc)
        assert_event_equal(again["event"], ref)
        assert _same({q: v for q, v in again.items() if q != "event"}, {q: v for q, v in clean.items() if q != "event"}), k
        eng.close()
        assert L.surtr_emul_live_allocs() == live0, (k, L.surtr_emul_live_allocs(), live0)
        assert L.surtr_emul_guard_check() == 0, k
    return n_alloc


def test_every_failed_allocation_is_reported_and_recovered(emul_lib_path, oracle):
    for tier in (None, "64"):
        env = dict(os.environ)
        env.pop("SURTR_FACES_TIER_HE", None)
        if tier:
            env["SURTR_FACES_TIER_HE"] = tier
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), emul_lib_path], cwd=ROOT, env=env, capture_output=True,
                               text=True, timeout=240)
        except subprocess.TimeoutExpired:
            raise AssertionError("the allocation sweep (faces tier %s) did not end within 240 s" % tier)
        assert r.returncode == 0, "faces tier %s: exit %d\n%s" % (tier, r.returncode, (r.stdout + r.stderr)[-3000:])
        assert "allocations swept" in r.stdout


if __name__ == "__main__":
    print("%d allocations swept" % _sweep(sys.argv[1]))
