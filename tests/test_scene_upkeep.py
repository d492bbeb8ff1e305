"""Scene upkeep (upkeep_dev.hip): the world bounds of every body taken on the device, and the three edits that change the set of
bodies without a solid leaving HBM -- remove, append, cull.

References, none of which runs the code under test:
 * bounds -- a second engine with the same scene and poses after scene_apply_poses of every body (which existed before the bounds):
   numpy min / max over download_piece, per piece and per body, must EQUAL the records as numbers, both sets.  As a definition check
   the box must also hold the float64 image A x + b of every vertex within 8 * 2^-24 * (|lo| + |hi|) per axis: three float roundings
   per coordinate, with room;
 * edits -- a fresh engine given upload_pieces of the expected list (the survivors as download_piece gave them before the edit, plus
   the new pieces: a Python list of lists with erase and push_back), then scene_set_compounds and scene_set_poses.  Every resident
   piece bit for bit, every array of pieces_derived byte for byte, the table, the poses and src; then the edited engine and the
   fresh one must agree on a scene event on a surviving body, scene_raycast, scene_overlap and scene_mass;
 * cull -- the reasons follow in Python from scene_mass and the reference boxes; thresholds lie at least 1 % from every mass and
   keep-box faces at least 1e-3 L from every box face, asserted on the reference before the engine is asked.

Scenes: test_pick_queries.scene_d's 306 boxes in compounds of 1, 2, 61, 64, 65, 70 and 43 pieces under test_scene_poses' poses (wave
edges in the body stage, a body across piece 256, one body at the identity); test_scene.three_bodies (the blob's 2 562-vertex Mesh is
more than a workgroup) with a regular tetrahedron and pieces of 63, 64 and 65 vertices behind them (wave edges in the piece stage).

The CPU tier runs on the emulation library (conftest's emul_engine); the GPU tier runs the same functions in child processes under a
time limit (helpers.run_gpu_child), plus the _dev form on a second stream.  The uploads with wild links run on the CPU tier only, as
in test_pieces_derived.py: were a guard incomplete, a GPU twin would fault a shared device."""
import ctypes
import json
import os
import subprocess
import textwrap

import numpy as np
import pytest

from helpers import run_gpu_child
from surtr_amd import engine, scenes

import test_pick_queries as PQ
import test_pieces_derived as PD
import test_scene as TS
import test_scene_poses as TSP

EYE = np.eye(4, dtype=np.float32)
SIZES, TABLE = TSP.SIZES, TSP.TABLE


# ------------------------------------------------------------------ scenes
_CACHE = {}


def lattice_world(E):
    """The lattice as a list of compounds of pieces {'mesh', 'conv'} (read with download_piece) and test_scene_poses' poses."""
    if "lat" not in _CACHE:
        eng, n = PQ.scene_d(E)
        flat = [{"mesh": eng.download_piece(p, 0), "conv": eng.download_piece(p, 1)} for p in range(n)]
        eng.close()
        world = [flat[TABLE[c]:TABLE[c + 1]] for c in range(len(SIZES))]
        poses = []
        for c in range(len(SIZES)):
            cen = np.concatenate([np.asarray(p["conv"]["pos"], np.float64) for p in world[c]]).mean(0)
            poses.append(EYE if c == TSP.AT_REST else TSP.pose_about(TSP.rotation(TSP.AXES[c], TSP.ANGLES[c]), cen, TSP.OFFSETS[c]))
        _CACHE["lat"] = (world, np.asarray(poses, np.float32))
    world, poses = _CACHE["lat"]
    return [list(c) for c in world], poses.copy()


def shifted_piece(s, d):
    return {"mesh": TS.shifted(s, d), "conv": TS.shifted(s, d)}


def bodies_world(E):
    """three_bodies, then a tetrahedron and solids of 63, 64 and 65 vertices; every body but the first under a pose."""
    if "bod" not in _CACHE:
        b = TS.bodies(E)
        world = [[{"mesh": m, "conv": c}] for m, c in zip(b["meshes"], b["convexes"])]
        world.append([shifted_piece(PQ.regular_tetrahedron(), (0, -20, 0))])
        world.append([shifted_piece(PD.bipyramid(61), (0, -30, 0)), shifted_piece(PD.bipyramid(62), (4, -30, 0))])
        world.append([shifted_piece(PD.bipyramid(63), (0, -40, 0))])
        assert [p["mesh"]["pos"].shape[0] for c in world[3:] for p in c] == [4, 63, 64, 65]
        poses = [EYE, TSP.MOVE, TSP.pose_about(TSP.rotation((0, 0, 1), 0.3), TS.SHIFT_BLOB, (0, 40, 0)),
                 TSP.pose_about(TSP.rotation((1, 2, 3), 0.9), (0, -20, 0), (3, 0, 1)), TSP.pose_about(TSP.rotation((1, 0, 0), -0.8), (2, -30, 0), (0, 0, 7)),
                 TSP.pose_about(TSP.rotation((0, 1, 0), 2.2), (0, -40, 0), (-5, 0, 0))]
        _CACHE["bod"] = (world, np.asarray(poses, np.float32))
    world, poses = _CACHE["bod"]
    return [list(c) for c in world], poses.copy()


def engine_of(E, world, poses=None):
    """A fresh engine given the list: upload_pieces, scene_set_compounds, scene_set_poses -- calls that existed before the edits."""
    flat = [p for c in world for p in c]
    eng = E.Engine(0)
    eng.upload_pieces([p["mesh"] for p in flat], [p["conv"] for p in flat])
    eng.scene_set_compounds(np.cumsum([0] + [len(c) for c in world]))
    if poses is not None:
        eng.scene_set_poses(poses)
    return eng


# ------------------------------------------------------------------ bounds
def reference_boxes(E, world, poses, set):
    """Per piece and per body: numpy min / max of what scene_apply_poses leaves, on an engine of its own."""
    ref = engine_of(E, world, poses)
    ref.scene_apply_poses(list(range(len(world))))
    n = sum(len(c) for c in world)
    pos = [np.asarray(ref.download_piece(p, set)["pos"], np.float32).reshape(-1, 3) for p in range(n)]
    ref.close()
    piece = np.zeros(n, engine.BOUNDS_DTYPE)
    for p in range(n):
        piece[p] = (pos[p].min(0), pos[p].max(0), pos[p].shape[0], 0)
    table = np.cumsum([0] + [len(c) for c in world])
    body = np.zeros(len(world), engine.BOUNDS_DTYPE)
    for c in range(len(world)):
        body[c] = (piece["lo"][table[c]:table[c + 1]].min(0), piece["hi"][table[c]:table[c + 1]].max(0), piece["n_vertices"][table[c]:table[c + 1]].sum(), 0)
    return piece, body


def bounds_dev(eng, mem, n, nc, set):
    d_b, d_p = mem.zeros(nc * 32, 0xAB), mem.zeros(n * 32, 0xAB)
    mem.sync()
    eng.scene_bounds_dev(mem.ptr(d_b), nc * 32, dev_piece=mem.ptr(d_p), piece_capacity=n * 32, set=set)
    return mem.down(d_p).view(engine.BOUNDS_DTYPE), mem.down(d_b).view(engine.BOUNDS_DTYPE)


def same_records(got, want):
    return all((got[k] == want[k]).all() for k in ("lo", "hi", "n_vertices", "status"))      # equal as numbers (-0 == +0)


def check_bounds(E, mem, world, poses):
    n, nc = sum(len(c) for c in world), len(world)
    table = np.cumsum([0] + [len(c) for c in world])
    eng = engine_of(E, world, poses)
    for s in (0, 1):
        piece, body = reference_boxes(E, world, poses, s)
        got_p, got_b = bounds_dev(eng, mem, n, nc, s)
        assert same_records(got_p, piece), s
        assert same_records(got_b, body), s
        assert same_records(eng.scene_bounds(set=s), body), s
        # the definition: the box holds the float64 image of every vertex, within three float roundings with room
        tol = 8 * 2.0 ** -24 * (np.abs(got_b["lo"].astype(np.float64)) + np.abs(got_b["hi"].astype(np.float64)))
        for c in range(nc):
            A, b = TSP.split(poses[c])
            for q in world[c]:
                x = np.asarray(q["conv" if s else "mesh"]["pos"], np.float64).reshape(-1, 3) @ A.T + b
                assert (x >= got_b["lo"][c] - tol[c]).all() and (x <= got_b["hi"][c] + tol[c]).all(), (s, c)
        # a body at the identity: the box of its resident positions
        for c in range(nc):
            if (poses[c] == EYE).all():
                x = np.concatenate([np.asarray(q["conv" if s else "mesh"]["pos"], np.float32).reshape(-1, 3) for q in world[c]])
                assert (got_b["lo"][c] == x.min(0)).all() and (got_b["hi"][c] == x.max(0)).all()
    # without a pose table: the resident boxes, and a second call gives the same bytes
    eng.scene_set_compounds(table)
    plain = eng.scene_bounds(set=1)
    piece, body = reference_boxes(E, world, None, 1)
    assert same_records(plain, body) and eng.scene_bounds(set=1).tobytes() == plain.tobytes()
    eng.close()


def run_bounds_lattice(E, mem):
    world, poses = lattice_world(E)
    assert (poses[TSP.AT_REST] == EYE).all() and TABLE[5] < 256 < TABLE[6]
    check_bounds(E, mem, world, poses)


def run_bounds_bodies(E, mem):
    world, poses = bodies_world(E)
    assert world[2][0]["mesh"]["pos"].shape[0] > 1024
    check_bounds(E, mem, world, poses)


def with_inf(piece):
    out = {}
    for k in ("mesh", "conv"):
        pos = np.array(piece[k]["pos"], np.float32).reshape(-1, 3)
        pos[1, 0] = np.inf
        out[k] = dict(piece[k], pos=pos)
    return out


def run_nonfinite(E):
    """An infinite coordinate: SURTR_BOUNDS_NONFINITE, lo / hi over the finite ones; the cull leaves that body alone."""
    world, _ = bodies_world(E)
    world = [world[0], [with_inf(world[1][0])], world[3]]
    eng = engine_of(E, world)
    for s in (0, 1):
        got = eng.scene_bounds(set=s)
        assert list(got["status"]) == [0, engine.BOUNDS_NONFINITE, 0]
        x = np.asarray(world[1][0]["conv" if s else "mesh"]["pos"], np.float64).reshape(-1, 3)
        x = np.where(np.isfinite(x), x, np.nan)
        assert (got["lo"][1] == np.nanmin(x, 0)).all() and (got["hi"][1] == np.nanmax(x, 0)).all()
    # a keep box around body 0 only: body 2 is outside; body 1's finite box is outside too, but its record says it is not to be trusted
    mass = eng.scene_mass(set=1)
    assert mass["status"][0] == 0 and mass["status"][2] == 0 and mass["mass"][0] > 1e-3 and mass["mass"][2] > 1e-3
    before = TS.snapshot(eng)
    reason, removed = eng.scene_cull(min_mass=1e-6, keep_box=[-5, -5, -5, 5, 5, 5], apply=False)
    want_light = int(mass["status"][1] == 0 and mass["mass"][1] <= np.float32(1e-6))
    assert list(reason) == [0, want_light, engine.CULL_OUTSIDE] and removed == 0
    TS.assert_unchanged(eng, before)
    eng.close()


# ------------------------------------------------------------------ edits against a fresh engine
def assert_same_scene(a, b):
    ta, ga = TS.snapshot(a)
    tb, gb = TS.snapshot(b)
    assert list(ta) == list(tb) and len(ga) == len(gb)
    for k, ((m, c), (m0, c0)) in enumerate(zip(ga, gb)):
        assert TS.same_solid(m, m0) and TS.same_solid(c, c0), k
    for s in (0, 1):
        da, db = a.pieces_derived(s), b.pieces_derived(s)
        assert set(da) == set(db)
        for k in da:
            assert np.asarray(da[k]).tobytes() == np.asarray(db[k]).tobytes(), (s, k)
    assert a.scene_poses().tobytes() == b.scene_poses().tobytes()


def assert_agree(E, a, b, world, poses, target):
    """The edited engine and the fresh one answer alike: ray cast, overlap, mass, and an event on a surviving body."""
    rays, spheres = [], []
    rng = np.random.default_rng(17)
    for c in range(len(world)):
        A, t = TSP.split(poses[c])
        cen = A @ np.asarray(world[c][0]["conv"]["pos"], np.float64).reshape(-1, 3).mean(0) + t
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        rays.append(np.r_[cen - 50 * u, u, 1000.0]); spheres.append(np.r_[cen, 1.0])
    ra, rb = a.scene_raycast(np.asarray(rays, np.float32)), b.scene_raycast(np.asarray(rays, np.float32))
    assert ra.tobytes() == rb.tobytes() and (ra["piece"] >= 0).sum() >= max(1, len(world) - 1)
    oa, ob = a.scene_overlap(np.asarray(spheres, np.float32)), b.scene_overlap(np.asarray(spheres, np.float32))
    assert oa.tobytes() == ob.tobytes() and oa.any()
    for s in (0, 1):
        assert a.scene_mass(set=s).tobytes() == b.scene_mass(set=s).tobytes()
    cube = TS.bodies(E)["cube"]
    pos = np.concatenate([np.asarray(p["mesh"]["pos"], np.float32).reshape(-1, 3) for p in world[target]])
    lo, hi = pos.min(0), pos.max(0)
    place = ((hi - lo).astype(np.float32), ((hi.astype(np.float64) + lo.astype(np.float64)) / 2).astype(np.float32))
    evs = []
    for eng in (a, b):
        TS.install(eng, cube, place)
        c = eng.scene_fracture_event(target, 0, cube["n_cells"], flags=0)
        assert c.status == 0 and c.n_frag >= len(world[target])
        evs.append(eng.download())
    for k in TS.EVENT_KEYS + ("frag_ids",):
        assert np.asarray(evs[0][k]).tobytes() == np.asarray(evs[1][k]).tobytes(), k


REMOVALS = {"first": [0], "last": [6], "adjacent": [3, 2], "all_but_one": [6, 0, 4, 2, 5, 3]}


def run_remove(E, which):
    world, poses = lattice_world(E)
    gone = REMOVALS[which]
    eng = engine_of(E, world, poses)
    n, src = eng.scene_remove(gone)
    keep = [c for c in range(len(world)) if c not in gone]
    model = [world[c] for c in keep]                       # erase
    want_src = [p for c in keep for p in range(TABLE[c], TABLE[c + 1])]
    assert n == len(want_src) and list(src) == want_src
    fresh = engine_of(E, model, poses[keep])
    assert_same_scene(eng, fresh)
    assert eng.scene_poses().tobytes() == poses[keep].tobytes()
    assert_agree(E, eng, fresh, model, poses[keep], keep.index(1))
    eng.close(); fresh.close()


def run_append_one_body(E):
    """To a scene of one body without a pose table: bodies of 1 and 65 pieces; first without a pose (no table is made: the poses
    read as identities), then with one."""
    lat, _ = lattice_world(E)
    cube = TS.bodies(E)
    base = [[{"mesh": cube["meshes"][0], "conv": cube["convexes"][0]}]]
    tet = [shifted_piece(PQ.regular_tetrahedron(), (0, -20, 0))]
    many = lat[4]
    assert len(many) == 65
    for world_arg in (None, np.asarray([TSP.MOVE, EYE], np.float32)):
        eng = engine_of(E, base)
        assert eng.scene_append([tet, many], world=world_arg) == 1
        model = base + [tet, many]                         # push_back
        poses = np.asarray([EYE, EYE, EYE] if world_arg is None else [EYE, TSP.MOVE, EYE], np.float32)
        fresh = engine_of(E, model, None if world_arg is None else poses)
        assert_same_scene(eng, fresh)
        assert list(eng.scene_compounds()) == [0, 1, 2, 67]
        assert_agree(E, eng, fresh, model, poses, 0)
        eng.close(); fresh.close()


def run_append_to_posed(E):
    """Behind the posed bodies: the poses that were there stay, the new body gets its own."""
    world, poses = bodies_world(E)
    eng = engine_of(E, world[:5], poses[:5])
    assert eng.scene_append([world[5]], world=[poses[5]]) == 5
    fresh = engine_of(E, world, poses)
    assert_same_scene(eng, fresh)
    assert_agree(E, eng, fresh, world, poses, 3)
    # and with no pose given the new body is at the identity
    eng2 = engine_of(E, world[:5], poses[:5])
    assert eng2.scene_append([world[5]]) == 5
    assert eng2.scene_poses().tobytes() == np.concatenate([poses[:5], EYE[None]]).tobytes()
    eng.close(); fresh.close(); eng2.close()


def run_edit_after_event(E):
    """An edit straight after an event: the fragments stay downloadable, the commit is SURTR_E_STATE."""
    for edit in ("remove", "append"):
        eng, world = TS.three_bodies(E)
        cube = TS.bodies(E)["cube"]
        TS.install(eng, cube, (cube["scale"], (cube["translate"] + TS.SHIFT_B).astype(np.float32)))
        eng.scene_fracture_event(1, 0, 8, flags=0)
        co, cp = eng.event_regroup()
        ev = eng.download()
        if edit == "remove":
            eng.scene_remove([0])
            model = world[1:]
        else:
            eng.scene_append([world[0]])
            model = world + [world[0]]
        TS.assert_scene_is(eng, model)
        again = eng.download()
        for k in TS.EVENT_KEYS + ("frag_ids",):
            assert np.asarray(again[k]).tobytes() == np.asarray(ev[k]).tobytes(), (edit, k)
        with pytest.raises(engine.SurtrError) as e:
            eng.scene_commit(co, cp)
        assert e.value.code == engine.E_STATE
        TS.assert_scene_is(eng, model)
        eng.close()


def run_steady_size(E):
    """Remove the largest body and append it again: from the second round on neither call allocates."""
    world, poses = bodies_world(E)
    order = [0, 1, 3, 4, 5, 2]                             # the blob last: erased and pushed back, it is last again
    world, poses = [world[c] for c in order], poses[order]
    eng = engine_of(E, world, poses)
    allocs = []
    for k in range(3):
        eng.scene_remove([5])
        a = eng.upload_stats()[1]
        assert eng.scene_append([world[5]], world=[poses[5]]) == 5
        allocs.append((a, eng.upload_stats()[1]))
    print("allocations per round (remove, append):", allocs)
    assert allocs[1] == (0, 0) and allocs[2] == (0, 0), allocs
    fresh = engine_of(E, world, poses)
    assert_same_scene(eng, fresh)
    eng.close(); fresh.close()


# ------------------------------------------------------------------ cull
def run_cull(E):
    world, poses = lattice_world(E)
    nc = len(world)
    eng = engine_of(E, world, poses)
    mass = eng.scene_mass(set=1)                        # (existed before the cull)
    _, box = reference_boxes(E, world, poses, 1)
    assert not mass["status"].any()
    ms = np.sort(mass["mass"])
    min_mass = float(np.float32(np.sqrt(ms[1] * ms[2])))
    assert (np.abs(mass["mass"] - min_mass) >= 0.01 * mass["mass"]).all() and ms[1] < min_mass < ms[2]
    L = float(np.linalg.norm(box["hi"].max(0).astype(np.float64) - box["lo"].min(0)))
    # a keep box that cuts off body 0 (24 units down the x axis) and body 4 (24 units up the y axis)
    keep = np.r_[box["lo"].min(0) - 1.0, box["hi"].max(0) + 1.0].astype(np.float32)
    others = [c for c in range(nc) if c != 0]
    keep[0] = np.float32((box["hi"][0][0] + box["lo"][others, 0].min()) / 2)
    others = [c for c in range(nc) if c != 4]
    keep[4] = np.float32((box["lo"][4][1] + box["hi"][others, 1].max()) / 2)
    for k in range(3):
        for face in (keep[k], keep[3 + k]):
            assert (np.abs(box["lo"][:, k] - face) >= 1e-3 * L).all() and (np.abs(box["hi"][:, k] - face) >= 1e-3 * L).all(), (k, face)
    light = mass["mass"] <= np.float32(min_mass)
    outside = ((box["hi"] < keep[:3]) | (box["lo"] > keep[3:])).any(1)
    want = (light * engine.CULL_LIGHT + outside * engine.CULL_OUTSIDE).astype(np.uint8)
    assert list(np.nonzero(outside)[0]) == [0, 4] and light.sum() == 2 and 0 < (want != 0).sum() < nc
    before = TS.snapshot(eng)
    reason, removed = eng.scene_cull(min_mass=min_mass, keep_box=keep, apply=False)
    assert list(reason) == list(want) and removed == 0
    TS.assert_unchanged(eng, before)
    assert eng.scene_poses().tobytes() == poses.tobytes()
    assert list(eng.scene_cull(min_mass=min_mass, apply=False)[0]) == list(light * engine.CULL_LIGHT)       # no keep box: nothing is outside
    # every body marked: nothing is removed, the reasons are filled
    with pytest.raises(engine.SurtrError) as e:
        eng.scene_cull(min_mass=float(ms[-1] * 2), keep_box=keep)
    assert e.value.code == engine.E_INVALID and list(e.value.reason) == list((np.ones(nc) * engine.CULL_LIGHT + outside * engine.CULL_OUTSIDE).astype(np.uint8))
    TS.assert_unchanged(eng, before)
    assert eng.scene_poses().tobytes() == poses.tobytes()
    # applied: the marked bodies are erased
    reason, removed = eng.scene_cull(min_mass=min_mass, keep_box=keep)
    kept = [c for c in range(nc) if not want[c]]
    assert list(reason) == list(want) and removed == nc - len(kept)
    fresh = engine_of(E, [world[c] for c in kept], poses[kept])
    assert_same_scene(eng, fresh)
    eng.close(); fresh.close()


# ------------------------------------------------------------------ errors
def run_errors(E):
    L_ = E.lib()
    world, poses = bodies_world(E)
    world, good = world[:3], poses[:3]
    fresh = E.Engine(0)
    for call in (lambda: fresh.scene_bounds(), lambda: fresh.scene_remove([0]), lambda: fresh.scene_append([world[0]]), lambda: fresh.scene_cull()):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == engine.E_STATE
    fresh.close()
    eng = engine_of(E, world, good)
    before = TS.snapshot(eng)

    def refused(code, call):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == code, e.value
        TS.assert_unchanged(eng, before)
        assert eng.scene_poses().tobytes() == good.tobytes()

    refused(engine.E_INVALID, lambda: eng.scene_remove([3]))
    refused(engine.E_INVALID, lambda: eng.scene_remove([1, 1]))
    refused(engine.E_INVALID, lambda: eng.scene_remove([2, 0, 1]))
    scaled = TSP.MOVE.copy(); scaled[:3, :3] *= np.float32(1.01)
    nan = TSP.MOVE.copy(); nan[1, 3] = np.nan
    for bad in (scaled, nan):
        refused(engine.E_INVALID, lambda: eng.scene_append([world[0]], world=[bad]))
    refused(engine.E_INVALID, lambda: eng.scene_append([world[0], []]))
    refused(engine.E_INVALID, lambda: eng.scene_bounds(set=2))
    refused(engine.E_INVALID, lambda: eng.scene_cull(keep_box=[0, 0, np.nan, 1, 1, 1]))
    # capacity one short (the emulation's device memory is host memory; on the GPU these calls return before they touch the pointers)
    n = ctypes.c_uint32(2)
    rec = np.full(2, 7, np.uint8).repeat(32)
    assert L_.surtr_scene_bounds(eng._h, ctypes.c_int(1), ctypes.byref(n), ctypes.c_void_p(rec.ctypes.data)) == engine.E_CAPACITY and n.value == 3 and (rec == 7).all()
    one = ctypes.c_void_p(1)          # never read: the capacities are checked first
    assert L_.surtr_scene_bounds_dev(eng._h, ctypes.c_int(1), one, ctypes.c_size_t(3 * 32 - 1), None, ctypes.c_size_t(0)) == engine.E_CAPACITY
    assert L_.surtr_scene_bounds_dev(eng._h, ctypes.c_int(1), one, ctypes.c_size_t(3 * 32), one, ctypes.c_size_t(3 * 32 - 1)) == engine.E_CAPACITY
    n = ctypes.c_uint32(2)
    why, removed = np.full(2, 0xAB, np.uint8), ctypes.c_uint32(9)
    assert L_.surtr_scene_cull(eng._h, ctypes.c_int(1), ctypes.c_float(10), ctypes.c_float(1e9), None, ctypes.c_int(1), ctypes.byref(n),
                               ctypes.c_void_p(why.ctypes.data), ctypes.byref(removed)) == engine.E_CAPACITY and n.value == 3 and (why == 0xAB).all()
    TS.assert_unchanged(eng, before)
    assert eng.scene_poses().tobytes() == good.tobytes()
    eng.close()


BAD_CASES = PD.BAD_CASES


def corrupt(s, case):
    """The faults test_pieces_derived.py uploads: wild links, wild and decreasing offsets, short rings."""
    off, nbr = np.array(s["off"], np.uint32), np.array(s["nbr"], np.int32)
    m = np.asarray(s["pos"]).reshape(-1, 3).shape[0]
    if case.startswith("link_"):
        nbr[5] = {"link_minus_one": -1, "link_m": m, "link_1_shl_30": 1 << 30, "link_int32_min": -2 ** 31}[case]
    elif case == "offset_1_shl_28":
        off[3] = 1 << 28
    elif case == "offsets_decrease":
        off[2] = off[4]
        assert off[3] < off[2] and off[-1] >= off[0]
    else:
        keep = int(case[-1])
        rings = [nbr[off[v]:off[v + 1]] for v in range(m)]
        rings[2] = rings[2][:keep]
        off = np.cumsum([0] + [len(r) for r in rings]).astype(np.uint32); nbr = np.concatenate(rings).astype(np.int32)
    return dict(s, off=off, nbr=nbr)


def run_append_faults(E):
    """Each fault is refused with the code the upload gives it (taken from an upload on an engine of its own), and the scene, the
    poses and the table stay as they were."""
    world, poses = bodies_world(E)
    world, good = world[:3], poses[:3]
    eng = engine_of(E, world, good)
    before = TS.snapshot(eng)
    cube = world[0][0]
    scratch = E.Engine(0)
    for case in BAD_CASES:
        for which in ("mesh", "conv"):
            bad = dict(cube, **{which: corrupt(cube[which], case)})
            with pytest.raises(engine.SurtrError) as up:
                scratch.upload_pieces([cube["mesh"], bad["mesh"]], [cube["conv"], bad["conv"]])
            assert up.value.code in (engine.E_INVALID, engine.E_TOPOLOGY)
            with pytest.raises(engine.SurtrError) as ap:
                eng.scene_append([[cube, bad]], world=[TSP.MOVE])
            assert ap.value.code == up.value.code, (case, which, ap.value.code, up.value.code)
            TS.assert_unchanged(eng, before)
            assert eng.scene_poses().tobytes() == good.tobytes()
    # the context is usable: the same append with sound pieces goes through
    assert eng.scene_append([[cube, cube]], world=[TSP.MOVE]) == 3
    fresh = engine_of(E, world + [[cube, cube]], np.concatenate([good, TSP.MOVE[None]]))
    assert_same_scene(eng, fresh)
    eng.close(); fresh.close(); scratch.close()


# ------------------------------------------------------------------ CPU tier (emulation)
def test_bounds_of_the_posed_lattice(emul_engine):
    run_bounds_lattice(emul_engine, TSP.HostMem())


def test_bounds_of_large_and_wave_edge_pieces(emul_engine):
    run_bounds_bodies(emul_engine, TSP.HostMem())


def test_nonfinite_coordinate_is_flagged_and_not_culled(emul_engine):
    run_nonfinite(emul_engine)


@pytest.mark.parametrize("which", sorted(REMOVALS))
def test_remove_equals_a_fresh_engine(emul_engine, which):
    run_remove(emul_engine, which)


def test_append_to_a_one_body_scene(emul_engine):
    run_append_one_body(emul_engine)


def test_append_behind_posed_bodies(emul_engine):
    run_append_to_posed(emul_engine)


def test_edit_after_an_event_keeps_the_fragments_and_bars_the_commit(emul_engine):
    run_edit_after_event(emul_engine)


def test_steady_size_edits_do_not_allocate(emul_engine):
    run_steady_size(emul_engine)


def test_cull_marks_and_removes_what_the_reference_says(emul_engine):
    run_cull(emul_engine)


def test_errors_leave_the_scene_unchanged(emul_engine):
    run_errors(emul_engine)


def test_append_refuses_what_an_upload_refuses(emul_engine):
    run_append_faults(emul_engine)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_scene_poses as TSP
    import test_scene_upkeep as T
    case = sys.argv[1]
    if case in ("bounds_lattice", "bounds_bodies"):
        getattr(T, "run_" + case)(engine, TSP.TorchMem(torch))
    elif case.startswith("remove_"):
        T.run_remove(engine, case[7:])
    elif case == "dev_forms":
        T.run_dev_forms(engine, torch)
    elif case == "harness":
        T.check_harness(engine, %(root)r)
    else:
        getattr(T, "run_" + case)(engine)
    print("ok", case)
""")


def run_dev_forms(E, torch):
    """surtr_scene_bounds_dev on a stream of its own with the in-flight hint at 6, from two contexts: the host form's bytes; and an
    edit on such a context leaves what it leaves on a plain one."""
    world, poses = lattice_world(E)
    n, nc = int(TABLE[-1]), len(SIZES)
    eng = engine_of(E, world, poses)
    want = [eng.scene_bounds(set=s) for s in (0, 1)]
    results = []
    ctxs = []
    for k in range(2):
        ctx = engine_of(E, world, poses)
        st = torch.cuda.Stream()
        ctx.set_stream(st.cuda_stream)
        ctx.set_events_in_flight(6)
        with torch.cuda.stream(st):
            out = []
            for s in (0, 1):
                d_b = torch.zeros(nc * 32, dtype=torch.uint8, device="cuda")
                d_p = torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
                st.synchronize()
                ctx.scene_bounds_dev(d_b.data_ptr(), d_b.numel(), dev_piece=d_p.data_ptr(), piece_capacity=d_p.numel(), set=s)
                st.synchronize()
                out.append((d_b.cpu().numpy().tobytes(), d_p.cpu().numpy().tobytes()))
        results.append(out)
        ctxs.append((ctx, st))
    assert results[0] == results[1]
    for s in (0, 1):
        assert same_records(np.frombuffer(results[0][s][0], engine.BOUNDS_DTYPE), want[s])
    ctx, st = ctxs[0]
    eng.scene_remove([3, 2])
    with torch.cuda.stream(st):
        ctx.scene_remove([3, 2])
        st.synchronize()
    assert_same_scene(ctx, eng)
    for s in (0, 1):
        assert ctx.scene_bounds(set=s).tobytes() == eng.scene_bounds(set=s).tobytes()
    for c, _ in ctxs:
        c.close()
    eng.close()


def check_harness(E, root, exe=None):
    """surtr_harness --body-clicks ... --bounds --cull-mass M --keep-box ... (FractureEngine::CullBodies and BodyBounds after every
    click) against the same clicks, cull and bounds through the Python calls.  The keep box ends below the body that test_scene_poses'
    harness scene parks 20 units up the z axis: the first cull removes it."""
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    clicks = [([-10.0, 6.3, 0.2], [1.0, 0.0, 0.0]), ([0.3, 0.2, 10.0], [0.0, 0.0, -1.0])]
    arg = ";".join(",".join("%r" % x for x in o + d) for o, d in clicks)
    pose_arg = ";".join("%d:" % c + ",".join("%r" % float(x) for x in W.reshape(-1)) for c, W in ((1, TSP.HARNESS_POSE), (3, TSP.HARNESS_FAR)))
    keep = [-50.0, -50.0, -50.0, 50.0, 50.0, 10.0]
    cmd = [exe, "--mesh", "cube", "--cells", "8", "--scene-poses", pose_arg, "--body-clicks", arg, "--impact-radius", "4.0", "--bounds",
           "--cull-mass", "0.0001", "--keep-box", ",".join("%r" % x for x in keep)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [json.loads(x) for x in p.stdout.strip().splitlines() if x.startswith('{"upkeep"')]
    assert len(lines) == len(clicks)
    sc = scenes.cube_scene(8)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, 8)
    n = eng.pieces_from_event()
    eng.scene_set_compounds(list(range(0, n, 2)) + [n])
    poses = np.tile(EYE, ((n + 1) // 2, 1, 1))
    poses[1], poses[3] = TSP.HARNESS_POSE, TSP.HARNESS_FAR
    eng.scene_set_poses(poses)
    removed_total = 0
    for k, (o, d) in enumerate(clicks):
        TSP.python_body_click(eng, o, d, 4.0, 8, False)
        reason, removed = eng.scene_cull(min_mass=1e-4, keep_box=keep)
        removed_total += removed
        b = eng.scene_bounds(set=1)
        assert lines[k]["upkeep"] == k and lines[k]["reasons"] == [int(x) for x in reason]
        assert lines[k]["table"] == [int(x) for x in eng.scene_compounds()]
        got = np.asarray(lines[k]["bounds"], np.float64)
        assert got.shape == (b.shape[0], 8)
        assert (got[:, :3].astype(np.float32) == b["lo"]).all() and (got[:, 3:6].astype(np.float32) == b["hi"]).all()
        assert (got[:, 6] == b["n_vertices"]).all() and (got[:, 7] == b["status"]).all()
        if k == 0:
            assert engine.CULL_OUTSIDE in [int(x) for x in reason] and removed >= 1
    assert removed_total >= 1
    eng.close()


@pytest.mark.gpu
def test_gpu_harness_upkeep():
    run_gpu_child(GPU_CHILD, "harness", 150)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["bounds_lattice", "bounds_bodies", "nonfinite", "remove_first", "remove_last", "remove_adjacent", "remove_all_but_one",
                                  "append_one_body", "append_to_posed", "edit_after_event", "steady_size", "cull", "errors", "dev_forms"])
def test_gpu_scene_upkeep(case):
    run_gpu_child(GPU_CHILD, case, 120)
