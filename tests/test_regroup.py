"""Row f1 (the step right after the event): bind sets, MergeOutOfImpact, HandleConvexIsland, and the
regroup-then-refit order of Surtr::DoFracture (Src/Surtr.cpp:1921-1939).  Product host code vs the oracle."""
import numpy as np
import pytest

from helpers import assert_event_equal
from surtr_amd import meshgen, scenes


def _two_level(engine_mod, n_first, n_second, torus=False, seed=0):
    """First event on a blob (or the cfg4 torus) -> its fragments become the pieces of one compound hit by a second pattern.
    seed != 0: other Voronoi seeds for both patterns."""
    sc = scenes.torus_scene(n_first) if torus else scenes.blob_scene(n_first)
    if seed:
        sc = scenes.make_scene(*meshgen.blob(scale=70.0), n_first, seeds=scenes.uniform_seeds(n_first, scenes.SEED + 1000 * seed))
    eng = engine_mod.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, n_first, flags=1)
    first = eng.download()
    meshes, convexes = scenes.fragments_as_pieces(first)
    keep = [i for i, m in enumerate(meshes) if np.diff(m["off"].astype(np.int64)).min() >= 3 and convexes[i]["pos"].shape[0] >= 4]
    meshes, convexes = [meshes[i] for i in keep], [convexes[i] for i in keep]
    cells = engine_mod.voronoi_cells(scenes.uniform_seeds(n_second, scenes.SEED + 7 + seed))
    fo, v012 = engine_mod.pattern_from_cells(cells)
    eng.upload_pieces(meshes, convexes)
    eng.upload_pattern(fo, v012)
    eng.place_cells(sc["scale"], sc["translate"])
    return sc, eng, meshes, convexes, fo, v012


def _solids(ev, pre):
    out = []
    vo, no = ev[pre + "_vert_off"], ev[pre + "_nbr_off"]
    for k in range(ev["frag_ids"].shape[0]):
        a, b = int(vo[k]), int(vo[k + 1])
        out.append({"pos": ev[pre + "_pos"][a:b], "off": (no[a:b + 1] - no[a]).astype(np.uint32), "nbr": ev[pre + "_nbr"][int(no[a]):int(no[b])]})
    return out


SHORT_FACES = {"faces": 0, "short": 0}      # over the Convex solids of every event checked in this process


def _count_short_faces(engine_mod, solids):
    eng = engine_mod.Engine(0)       # (its own context: surtr_extract_faces replaces the fragments of the one it is given)
    for s in solids:
        fo, _ = eng.extract_faces(s)
        n = np.diff(fo.astype(np.int64))
        SHORT_FACES["faces"] += n.shape[0]
        SHORT_FACES["short"] += int((n < 3).sum())
    eng.close()


def check_regroup_and_refit_order(emul_engine, oracle, n_first=24, n_second=5, torus=False, seed=0):
    sc, eng, meshes, convexes, fo, v012 = _two_level(emul_engine, n_first, n_second, torus, seed)
    # event WITHOUT refit: the reference regroups on the un-refitted Convex solids
    c = eng.fracture_event(0, n_second, flags=2)
    ev = eng.download()
    conv = _solids(ev, "conv")
    _count_short_faces(emul_engine, conv)
    assert c.n_frag > 20
    co, cp = emul_engine.regroup(conv, ev["frag_ids"][:, 0])
    ro, rp = oracle.regroup(conv, ev["frag_ids"][:, 0])
    assert np.array_equal(co, ro) and np.array_equal(cp, rp)
    do, dp = eng.event_regroup()                       # the same as a device step on the resident fragments
    assert np.array_equal(do, ro) and np.array_equal(dp, rp)
    hit = np.unique(ev["frag_ids"][:, 0]).shape[0]    # (a cell may lie off the pieces and yield nothing)
    assert co.shape[0] - 1 >= (hit if seed else n_second) + 1           # bind 0 + one compound per cell (+ splits)
    assert sorted(cp.tolist()) == list(range(c.n_frag))
    # islands of compounds were actually found somewhere (pieces of one cell that do not touch)
    sizes = np.diff(co.astype(np.int64))
    assert sizes[0] == 0 and sizes.max() > 1
    # ...then Refitting + SetExtract (:1938-1939): same result as an event with refit on
    eng.event_refit()
    after = eng.download()
    planes = oracle.place_cells(v012, sc["scale"], sc["translate"])
    ref = oracle.event(meshes, convexes, fo, planes, refit=True, render=True, threads=4)
    assert_event_equal(after, ref)
    eng.close()


def check_partial_fracture_merges_out_of_impact(emul_engine, oracle, n_first=24, n_second=5, torus=False, seed=0):
    sc, eng, meshes, convexes, fo, v012 = _two_level(emul_engine, n_first, n_second, torus, seed)
    sphere, _ = meshgen.icosphere(2)
    impact = (sc["translate"] + np.float32([0.2, 0.1, 0.0]) * sc["scale"]).astype(np.float32)
    radius = float(0.2 * sc["scale"].max())
    cloud = (sphere.astype(np.float32) * np.float32(0.5) * np.float32(radius) + impact).astype(np.float32)
    # ApplyFracture(partial): pieces whose Convex is out of the sphere stay whole (:2107-2124)
    outside = np.array([emul_engine.convex_out_of_sphere(cv, cloud, impact, radius) for cv in convexes], np.uint8)
    assert all(bool(outside[i]) == oracle.convex_out_of_sphere(convexes[i], cloud, impact, radius) for i in range(len(convexes)))
    assert 0 < outside.sum() < len(convexes)
    c = eng.fracture_event(0, n_second, outside=outside, flags=2)
    ev = eng.download()
    assert not np.isin(ev["frag_ids"][:, 1], np.nonzero(outside)[0]).any()
    pieces = [convexes[i] for i in np.nonzero(outside)[0]] + _solids(ev, "conv")
    _count_short_faces(emul_engine, pieces)
    n_out = int(outside.sum())
    cell = np.concatenate([np.full(n_out, -1, np.int32), ev["frag_ids"][:, 0]])
    co, cp = emul_engine.regroup(pieces, cell, n_outside=n_out, partial=True, sphere_points=cloud, origin=impact, radius=radius)
    ro, rp = oracle.regroup(pieces, cell, n_outside=n_out, partial=True, sphere_points=cloud, origin=impact, radius=radius)
    assert np.array_equal(co, ro) and np.array_equal(cp, rp)
    # the outside compound only grows -- until HandleConvexIsland takes it apart like any other (its islands are appended):
    # whatever holds a kept piece holds, besides kept pieces, only fragments that are out of the sphere
    out = [True] * n_out + [emul_engine.convex_out_of_sphere(s, cloud, impact, radius) for s in pieces[n_out:]]
    groups = [cp[int(co[i]):int(co[i + 1])] for i in range(co.shape[0] - 1)]
    with_kept = [g for g in groups if g.size and g.min() < n_out]
    assert all(out[p] for g in with_kept for p in g) and sum(g.size for g in with_kept) >= n_out
    assert np.diff(co.astype(np.int64))[0] >= n_out or seed
    do, dp = eng.event_regroup(partial=True, sphere_points=cloud, origin=impact, radius=radius)
    assert np.array_equal(do, ro) and np.array_equal(dp, rp)
    eng.close()


def test_regroup_and_refit_order(emul_engine, oracle):
    check_regroup_and_refit_order(emul_engine, oracle)


def test_partial_fracture_merges_out_of_impact(emul_engine, oracle):
    check_partial_fracture_merges_out_of_impact(emul_engine, oracle)


SIZES = [(24, 5), (16, 8), (40, 4)]
SEEDS = range(1, 9)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n_first,n_second", SIZES)
def test_regroup_and_refit_order_random(emul_engine, oracle, n_first, n_second, seed):
    """Parity of host, oracle and device step on random two-level events (no plain reference: nothing bounds the margins of a
    random scene).  Counted once over the 50 events of this module (these 2 x 24 and the two above; SHORT_FACES): 26 588 faces of
    the un-refitted Convex solids and kept pieces, none of fewer than three points -- the reads of a third point in
    host_regroup.cpp and the oracle, which the reference makes unguarded, are guarded all the same."""
    check_regroup_and_refit_order(emul_engine, oracle, n_first, n_second, seed=seed)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("n_first,n_second", SIZES)
def test_partial_fracture_merges_out_of_impact_random(emul_engine, oracle, n_first, n_second, seed):
    check_partial_fracture_merges_out_of_impact(emul_engine, oracle, n_first, n_second, seed=seed)
