"""FractureArgs::RefittingPointLimit above 4: the greedy limited hull on the device (csrc/refit_hull.h, k_refit_n) against
the oracle's restatement -- `check_*` on the single-lane emulation here, the same functions on the MI355X under
@pytest.mark.gpu, plus a configs[3]-sized event there.

The key-rule clouds (check_key_rule) are not closed solids, so they cannot be fragments: they go through the test entry
surtr_hull_normals_device, which runs the same device function (rh_build) that k_refit_n runs per fragment."""
import numpy as np
import pytest

from helpers import RTOL, TOPOLOGY_KEYS, fragment, solid_is_polyhedron
from surtr_amd import scenes

E_INVALID, E_CAPACITY = 1, 3
MAX_FACES = 63      # two slab planes per hull face, SURTR_MAXF = 127 planes per clip


def _blob_event(oracle, n_cells=12):
    """The un-refitted 12-cell blob event of tests/test_solid_ops.py."""
    sc = scenes.blob_scene(n_cells)
    planes = oracle.place_cells(sc["v012"], sc["scale"], sc["translate"])
    ev = oracle.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=False, render=False, threads=4)
    return sc, planes, ev


def _same_solid(got, ref, what):
    assert np.array_equal(got["off"], ref["off"]), ("off", what)
    assert np.array_equal(got["nbr"], ref["nbr"]), ("nbr", what)
    assert np.allclose(got["pos"], ref["pos"], rtol=RTOL, atol=1e-6), ("pos", what)


def _faces(oracle, mesh, limit):
    return oracle.hull_normals(mesh["pos"], min(mesh["pos"].shape[0], limit)).shape[0]


# ---- 1. single solids ---------------------------------------------------------------------------------------------------
def check_single_solids(E, oracle):
    sc, planes, ev = _blob_event(oracle)
    eng = E.Engine(0)
    try:
        assert eng.get_refit_point_limit() == 4
        for k in range(0, ev["frag_ids"].shape[0], 3):
            mesh, conv = fragment(ev, k, "mesh"), fragment(ev, k, "conv")
            for limit in (5, 8, 16, 20, 4):      # (4 after 20: the setting is state and must go back)
                eng.set_refit_point_limit(limit)
                assert eng.get_refit_point_limit() == limit
                _same_solid(eng.refit_solid(mesh, conv), oracle.refit(conv, mesh, limit), (k, limit))
    finally:
        eng.close()


# ---- 2. whole event -----------------------------------------------------------------------------------------------------
def _check_convexes(oracle, got, unrefitted, limit):
    n = unrefitted["frag_ids"].shape[0]
    assert got["frag_ids"].shape[0] == n
    for k in range(n):
        ref = oracle.refit(fragment(unrefitted, k, "conv"), fragment(unrefitted, k, "mesh"), limit)
        _same_solid(fragment(got, k, "conv"), ref, (k, limit))


def check_whole_event(E, oracle):
    sc, planes, ev = _blob_event(oracle)
    n = ev["frag_ids"].shape[0]
    assert n == 11
    meshes = [fragment(ev, k, "mesh") for k in range(n)]
    convs = [fragment(ev, k, "conv") for k in range(n)]
    rendered = oracle.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=False, render=True, threads=4)
    for limit in (8, 20):
        eng = E.Engine(0)
        try:
            eng.load_fragments(meshes, convs, ev["frag_ids"])
            eng.set_refit_point_limit(limit)
            eng.event_refit()
            got = eng.download()
            assert eng.event_counts().n_failed == 0
        finally:
            eng.close()
        assert not got["frag_status"].any()
        for key in ("frag_ids", "mesh_vert_off", "mesh_nbr_off", "mesh_nbr", "mesh_pos"):
            assert np.array_equal(got[key], ev[key]), key      # the Mesh arrays are untouched
        _check_convexes(oracle, got, ev, limit)
        # the same through an event with SURTR_EVT_REFIT
        eng = E.Engine(0)
        try:
            eng.set_refit_point_limit(limit)
            eng.upload_pieces([sc["mesh"]], [sc["convex"]])
            eng.upload_pattern(sc["face_off"], sc["v012"])
            eng.place_cells(sc["scale"], sc["translate"])
            c = eng.fracture_event(0, sc["n_cells"], flags=3)
            got = eng.download()
        finally:
            eng.close()
        assert c.status == 0 and c.n_failed == 0 and not got["frag_status"].any()
        for key in TOPOLOGY_KEYS:
            if not key.startswith("conv_"):
                assert np.array_equal(got[key], rendered[key]), key
        assert np.allclose(got["mesh_pos"], rendered["mesh_pos"], rtol=RTOL, atol=1e-6)
        assert np.allclose(got["vnc"], rendered["vnc"], rtol=RTOL, atol=1e-6)
        _check_convexes(oracle, got, rendered, limit)


# ---- 3. small fragments: min(n, limit) bites ------------------------------------------------------------------------------
def check_small_fragments(E, oracle):
    sc = scenes.cube_scene(8)
    planes = oracle.place_cells(sc["v012"], sc["scale"], sc["translate"])
    ev = oracle.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=False, render=False, threads=4)
    n = ev["frag_ids"].shape[0]
    meshes = [fragment(ev, k, "mesh") for k in range(n)]
    convs = [fragment(ev, k, "conv") for k in range(n)]
    assert max(m["pos"].shape[0] for m in meshes) <= 16
    for limit in (8, 16, 32):
        assert max(_faces(oracle, m, limit) for m in meshes) <= 36
        eng = E.Engine(0)
        try:
            eng.set_refit_point_limit(limit)
            eng.load_fragments(meshes, convs, ev["frag_ids"])
            eng.event_refit()
            got = eng.download()
        finally:
            eng.close()
        assert not got["frag_status"].any()
        _check_convexes(oracle, got, ev, limit)


# ---- 4. key rule --------------------------------------------------------------------------------------------------------
def key_rule_clouds():
    """200 clouds of 30 points; points 10..19 are copies of 0..9 displaced by 3e-7 (they print alike with "%f" as often as
    not); on every second cloud the coordinates are first rounded to multiples of 1/128 (exact ties of the rounding)."""
    rng = np.random.default_rng(7)
    out = []
    for c in range(200):
        p = rng.uniform(-1.0, 1.0, (30, 3))
        if c % 2 == 1:
            p = np.round(p * 128.0) / 128.0
        p[10:20] = p[0:10] + 3e-7
        out.append(np.ascontiguousarray(p, np.float32))
    return out


def check_key_rule(E, oracle):
    eng = E.Engine(0)
    try:
        for c, pts in enumerate(key_rule_clouds()):
            ref = oracle.hull_normals(pts, 12)
            assert 4 <= ref.shape[0] <= MAX_FACES      # the inputs are valid and within every cap,
            assert np.array_equal(E.hull_normals(pts, 12), ref), c      # and the two host readings of the reference agree on them
            got = eng.hull_normals_device(pts, 12)
            assert got.shape == ref.shape and np.array_equal(got, ref), c
    finally:
        eng.close()


def check_coord_key(E):
    # the sign of a value that rounds to zero: "-0.000000" against "0.000000"
    assert E.coord_key(np.float32(-1e-9)) == (1, 0)
    assert E.coord_key(np.float32(1e-9)) == (0, 0)
    assert E.coord_key(np.float32(-0.0)) == (1, 0) and E.coord_key(np.float32(0.0)) == (0, 0)
    # the tie at 1/128 = 0.0078125 exactly: half-to-even gives ...812, not ...813
    assert E.coord_key(np.float32(0.0078125)) == (0, 7812)
    assert E.coord_key(np.float32(3 * 0.0078125)) == (0, 23438)      # 0.0234375: the odd neighbour rounds up
    # against the C library's own "%f" on a sample of ordinary and extreme values
    rng = np.random.default_rng(11)
    xs = np.concatenate([rng.uniform(-3, 3, 2000), rng.uniform(-1e-5, 1e-5, 500), rng.integers(-384, 384, 500) / 128.0,
                         [1e-45, 16777216.0, 1.5e12, -123456.789]]).astype(np.float32)
    for x in xs:
        text = "%f" % float(x)
        want = (1 if text.startswith("-") else 0, int(text.lstrip("-").replace(".", "")))
        assert E.coord_key(x) == want, (x, text)
    with pytest.raises(E.SurtrError):
        E.coord_key(np.float32(np.inf))
    with pytest.raises(E.SurtrError):
        E.coord_key(np.float32(3e38))


# ---- 5. engine limit ----------------------------------------------------------------------------------------------------
def check_engine_limit(E, oracle):
    sc, planes, ev = _blob_event(oracle)
    n = ev["frag_ids"].shape[0]
    meshes = [fragment(ev, k, "mesh") for k in range(n)]
    convs = [fragment(ev, k, "conv") for k in range(n)]
    over = [_faces(oracle, m, 32) > MAX_FACES for m in meshes]
    assert 0 < sum(over) < n      # both sides are exercised
    eng = E.Engine(0)
    try:
        eng.set_refit_point_limit(32)
        eng.load_fragments(meshes, convs, ev["frag_ids"])
        eng.event_refit()
        got = eng.download()
        c = eng.event_counts()
        qs = eng.queue_stats()
        assert c.status == 0      # the event stands
        assert c.n_failed == sum(over) and int(qs[95]) == sum(over)
        for k in range(n):
            if over[k]:
                assert got["frag_status"][k] == E_CAPACITY, k
                kept = fragment(got, k, "conv")
                assert np.array_equal(kept["pos"], convs[k]["pos"]) and np.array_equal(kept["off"], convs[k]["off"]) \
                    and np.array_equal(kept["nbr"], convs[k]["nbr"]), k
            else:
                assert got["frag_status"][k] == 0, k
                _same_solid(fragment(got, k, "conv"), oracle.refit(convs[k], meshes[k], 32), k)
        # asked for that one solid, the call says so
        k = over.index(True)
        with pytest.raises(E.SurtrError) as err:
            eng.refit_solid(meshes[k], convs[k])
        assert err.value.code == E_CAPACITY
    finally:
        eng.close()


# ---- 6. arguments -------------------------------------------------------------------------------------------------------
def check_arguments(E):
    eng = E.Engine(0)
    try:
        eng.set_refit_point_limit(9)
        for bad in (0, 3, 33):
            with pytest.raises(E.SurtrError) as err:
                eng.set_refit_point_limit(bad)
            assert err.value.code == E_INVALID
            assert eng.get_refit_point_limit() == 9
        for good in (4, 32):
            eng.set_refit_point_limit(good)
            assert eng.get_refit_point_limit() == good
    finally:
        eng.close()


CASES = [check_single_solids, check_whole_event, check_small_fragments, check_key_rule, check_engine_limit]


@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__)
def test_refit_limit_emulated(emul_engine, oracle, case):
    case(emul_engine, oracle)


def test_refit_limit_arguments_emulated(emul_engine):
    check_arguments(emul_engine)


def test_coord_key(emul_engine):
    check_coord_key(emul_engine)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda f: f.__name__)
def test_refit_limit_gpu(gpu_engine, oracle, case):
    case(gpu_engine, oracle)


@pytest.mark.gpu
def test_refit_limit_arguments_gpu(gpu_engine):
    check_arguments(gpu_engine)
    check_coord_key(gpu_engine)


# ---- 7. GPU only: a configs[3]-sized event --------------------------------------------------------------------------------
@pytest.mark.gpu
def test_torus_4096_refit_at_limit_8(gpu_engine, oracle):
    """Torus, 4 096 cells (as tests/test_gpu_parity.py builds it), EVT_REFIT at RefittingPointLimit 8: the Convex of every
    fragment of 64 cells sampled by a fixed seed against oracle.refit of the un-refitted fragment.  A flagged fragment is
    accepted only where the oracle's hull has more than 63 faces or the oracle's own result is invalid; at most 1 % of the
    sampled fragments may be set aside that way."""
    limit = 8
    sc = scenes.torus_scene(4096)
    eng = gpu_engine.Engine(0)
    try:
        eng.set_refit_point_limit(limit)
        eng.upload_pieces([sc["mesh"]], [sc["convex"]])
        eng.upload_pattern(sc["face_off"], sc["v012"])
        eng.place_cells(sc["scale"], sc["translate"])
        c = eng.fracture_event(0, sc["n_cells"], flags=1)
        got = eng.download()
        raw = eng.fracture_event(0, sc["n_cells"], flags=0)
        unref = eng.download()
    finally:
        eng.close()
    assert c.status == 0 and raw.status == 0 and c.n_frag == raw.n_frag
    assert np.array_equal(got["frag_ids"], unref["frag_ids"])
    # (a third of the pattern's cells miss the torus: the 64 cells are drawn from those that hold a fragment)
    holding = np.unique(got["frag_ids"][:, 0])
    cells = set(np.random.default_rng(20261017).choice(holding, 64, replace=False).tolist())
    sample = [k for k in range(c.n_frag) if int(got["frag_ids"][k][0]) in cells]
    assert len(cells) == 64 and len(sample) >= 64
    aside = []
    for k in sample:
        mesh, conv = fragment(unref, k, "mesh"), fragment(unref, k, "conv")
        oracle.links_off_the_array(reset=True)
        ref = oracle.refit(conv, mesh, limit)
        undefined = oracle.links_off_the_array(reset=True) > 0
        if got["frag_status"][k] != 0:
            assert _faces(oracle, mesh, limit) > MAX_FACES or undefined or not solid_is_polyhedron(ref), ("flagged without cause", k)
            aside.append(k)
            continue
        _same_solid(fragment(got, k, "conv"), ref, k)
    print("sampled fragments %d, set aside %d, n_failed of the event %d of %d" % (len(sample), len(aside), c.n_failed, c.n_frag))
    assert len(aside) <= 0.01 * len(sample), aside
