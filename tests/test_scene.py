"""The resident pieces as a scene of several bodies (scene_dev.hip): the event on one body of many, and the commit that does
ExecuteFractureRoutine's bookkeeping (Src/Surtr.cpp:1829-1883) on the device.

Two references, neither of which runs the code under test:
 (a) geometry -- a second engine is given ONLY the target compound's pieces (read with download_piece before the event) and runs
     the calls the engine had before the scene existed: the same placement, fracture_event with the restricted mask,
     event_regroup, event_refit.  Solids must be bit-identical, compounds equal (the piece numbers of the two regroupings are the
     same by construction: the compound's skipped pieces ascending, then the fragments; frag_ids differ by the compound's first
     resident piece);
 (b) bookkeeping -- a plain Python list of lists, CompoundVec with erase and push_back.

Scenes: three bodies (the golden cube, a copy of it 10 units along x, the 64-cell blob's mesh with its ACH Convex moved 300 units
along y: 2 562 Mesh vertices, more than a workgroup has threads).  Click 1 breaks the MIDDLE body with the 8-cell pattern, partial,
with a sphere that leaves five fragments to bind 0 and three compounds beside it; click 2 picks a piece of a compound click 1 made
with pieces_raycast, masks another piece of that compound and breaks the rest with the 64-cell pattern: more than 64 resident
pieces.  The fixture of the 8-cell cube event is tests/golden/cube8.npz (tests/golden/digests.json holds no cube; its blob64 record
is checked as well).

A compound of nothing that can be kept: regroup's bind 0 of an event without a mask and without a sphere is empty (the error
test commits such compounds), and the fragment of tests/golden/nonterminating_faces_fragment.npz whose faces cannot be extracted
is flagged by a render event; committed with every piece in a compound of its own, that fragment's compound is not created.  The
expectation is built from reference (a)'s download, and that something was left out is asserted.

The CPU tier runs on the one emulation library of tests/emul (conftest's emul_engine); the GPU tier runs the same scenes on the
MI355X in child processes under a time limit (helpers.run_gpu_child)."""
import hashlib
import json
import os
import subprocess
import textwrap

import numpy as np
import pytest

from helpers import run_gpu_child
from surtr_amd import engine, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EVENT_KEYS = ("mesh_vert_off", "mesh_pos", "mesh_nbr_off", "mesh_nbr", "conv_vert_off", "conv_pos", "conv_nbr_off", "conv_nbr", "frag_status")
SHIFT_B = np.float32([10, 0, 0])
SHIFT_BLOB = np.float32([0, 300, 0])


# ------------------------------------------------------------------ helpers
def shifted(solid, d):
    return dict(solid, pos=(np.asarray(solid["pos"], np.float32).reshape(-1, 3) + np.asarray(d, np.float32)).astype(np.float32))


def same_solid(a, b):
    return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() and np.asarray(a[k]).shape == np.asarray(b[k]).shape for k in ("pos", "off", "nbr"))


def sphere_cloud(origin, radius, n=64):
    """A Fibonacci sphere, scaled by the radius and moved to the impact (DoFracture, Src/Surtr.cpp:1898-1905)."""
    k = np.arange(n) + 0.5
    phi, th = np.arccos(1 - 2 * k / n), np.pi * (1 + 5 ** 0.5) * k
    u = np.c_[np.cos(th) * np.sin(phi), np.sin(th) * np.sin(phi), np.cos(phi)]
    return (u * radius + np.asarray(origin, np.float64)).astype(np.float32)


_BODIES = {}


def bodies(E):
    """(meshes, convexes) of the three bodies, and the two patterns; computed once."""
    if not _BODIES:
        cube, blob = scenes.cube_scene(8), scenes.blob_scene(64)
        tmp = E.Engine(0)
        ach, _ = scenes.ach_convex(tmp, blob["mesh"]["pos"])
        tmp.close()
        _BODIES["meshes"] = [cube["mesh"], shifted(cube["mesh"], SHIFT_B), shifted(blob["mesh"], SHIFT_BLOB)]
        _BODIES["convexes"] = [cube["convex"], shifted(cube["convex"], SHIFT_B), shifted(ach, SHIFT_BLOB)]
        _BODIES["cube"], _BODIES["blob"] = cube, blob
    return _BODIES


def three_bodies(E):
    """-> (engine, world): world is reference (b), a list of compounds, each a list of pieces {'mesh', 'conv'}."""
    b = bodies(E)
    eng = E.Engine(0)
    eng.upload_pieces(b["meshes"], b["convexes"])
    assert list(eng.scene_compounds()) == [0, 3]          # one compound holding every piece
    eng.scene_set_compounds([0, 1, 2, 3])
    world = [[{"mesh": m, "conv": c}] for m, c in zip(b["meshes"], b["convexes"])]
    assert b["meshes"][2]["pos"].shape[0] > 1024           # a copied piece larger than a workgroup
    return eng, world


def snapshot(eng):
    """Everything resident, read back: (table, [(mesh, conv), ...])."""
    table = eng.scene_compounds()
    return table, [(eng.download_piece(p, 0), eng.download_piece(p, 1)) for p in range(int(table[-1]))]


def assert_scene_is(eng, world):
    """Every resident piece, both sets, bit for bit against the model, and the compound table."""
    table, got = snapshot(eng)
    assert list(table) == list(np.cumsum([0] + [len(c) for c in world])), (table, [len(c) for c in world])
    flat = [p for c in world for p in c]
    assert len(got) == len(flat)
    for k, (p, (m, c)) in enumerate(zip(flat, got)):
        assert same_solid(m, p["mesh"]), ("mesh", k)
        assert same_solid(c, p["conv"]), ("conv", k)


def assert_unchanged(eng, before):
    table, got = snapshot(eng)
    assert list(table) == list(before[0]) and len(got) == len(before[1])
    for (m, c), (m0, c0) in zip(got, before[1]):
        assert same_solid(m, m0) and same_solid(c, c0)


def install(eng, pattern, place):
    if "planes" in pattern:
        eng.upload_planes(pattern["face_off"], pattern["planes"])
    else:
        eng.upload_pattern(pattern["face_off"], pattern["v012"])
        eng.place_cells(*place)


def reference_a(E, pieces, pattern, place, mask, regroup_kw, flags=0):
    """Reference (a): the target compound's pieces alone through the calls that do not know of a scene.
    -> (compound_off, compound_piece, downloaded event after the refit)."""
    ref = E.Engine(0)
    ref.upload_pieces([p["mesh"] for p in pieces], [p["conv"] for p in pieces])
    install(ref, pattern, place)
    ref.fracture_event(0, pattern["n_cells"], outside=mask, flags=flags)
    ro, rp = ref.event_regroup(**regroup_kw)
    if not flags & engine.EVT_REFIT:
        ref.event_refit()
    rev = ref.download()
    ref.close()
    return ro, rp, rev


def expected_compounds(pieces, mask, ro, rp, rev):
    """What the returned compounds become: skipped pieces as they stand, fragments that are solids and not flagged, no empty
    compound.  -> (list of compounds, src values relative to the compound's first piece as ('old', local) / ('frag', f))."""
    skipped = [k for k in range(len(pieces)) if mask is not None and mask[k]]
    fm, fc = scenes.fragments_as_pieces(rev)
    out, src, left_out = [], [], 0
    for c in range(len(ro) - 1):
        comp = []
        for q in rp[ro[c]:ro[c + 1]]:
            if q < len(skipped):
                comp.append(pieces[skipped[q]]); src.append(("old", skipped[q]))
                continue
            f = int(q) - len(skipped)
            if fm[f]["pos"].shape[0] < 4 or fc[f]["pos"].shape[0] < 4 or rev["frag_status"][f] != 0:
                left_out += 1
                continue
            comp.append({"mesh": fm[f], "conv": fc[f]}); src.append(("frag", f))
        if comp:
            out.append(comp)
    return out, src, left_out


def click(E, eng, world, target, pattern, place, mask, regroup_kw, conditions=None, use_async=False, flags=0, singletons=False):
    """One click on compound `target`, checked against (a) and (b).  Returns what scene_commit returned.
    singletons: commit with every piece in a compound of its own instead of the regrouping's compounds."""
    p0 = sum(len(c) for c in world[:target])
    pieces = world[target]
    # (the model's pieces are what is resident: the reference is given what download_piece reads)
    for k, p in enumerate(pieces):
        assert same_solid(eng.download_piece(p0 + k, 0), p["mesh"]) and same_solid(eng.download_piece(p0 + k, 1), p["conv"])
    ro, rp, rev = reference_a(E, pieces, pattern, place, mask, regroup_kw, flags)
    if conditions is not None:
        conditions(ro, rp, rev)                            # on the reference alone, before the scene is looked at
    # the scene
    install(eng, pattern, place)
    if use_async:
        eng.scene_fracture_event_async(target, 0, pattern["n_cells"], outside=mask, flags=flags)
        c = eng.event_counts()
    else:
        c = eng.scene_fracture_event(target, 0, pattern["n_cells"], outside=mask, flags=flags)
    n_unmasked = len(pieces) - (0 if mask is None else int(np.count_nonzero(mask)))
    assert c.n_pairs == pattern["n_cells"] * len(pieces) and c.status == 0      # pieces of other compounds produce no pair
    co, cp = eng.event_regroup(**regroup_kw)
    assert list(co) == list(ro) and list(cp) == list(rp), (co, ro, cp, rp)
    if not flags & engine.EVT_REFIT:
        eng.event_refit()
    ev = eng.download()
    if singletons:
        co = ro = np.arange(int(co[-1]) + 1, dtype=np.uint32)
        cp = rp = np.arange(int(co[-1]), dtype=np.int32)
    new, src_exp, left_out = expected_compounds(pieces, mask, ro, rp, rev)
    for k in EVENT_KEYS:
        assert np.asarray(ev[k]).tobytes() == np.asarray(rev[k]).tobytes(), k
    ids, rids = ev["frag_ids"].reshape(-1, 3), rev["frag_ids"].reshape(-1, 3)
    assert (ids[:, 0] == rids[:, 0]).all() and (ids[:, 2] == rids[:, 2]).all() and (ids[:, 1] == rids[:, 1] + p0).all()
    assert n_unmasked == 0 or set(ids[:, 1]) <= set(range(p0, p0 + len(pieces)))
    # (b): erase, push_back
    model = [list(c_) for c_ in world]
    del model[target]
    first_new = len(model)
    model.extend(new)
    n, first, n_new, src = eng.scene_commit(co, cp)
    assert (n, first, n_new) == (sum(len(c_) for c_ in model), first_new, len(new)), (n, first, n_new, first_new, len(new))
    others = [p for p in range(sum(len(c_) for c_ in world)) if not p0 <= p < p0 + len(pieces)]
    want_src = others + [p0 + k if kind == "old" else -(k + 1) for kind, k in src_exp]
    assert list(src) == want_src, (list(src), want_src)
    assert_scene_is(eng, model)
    world[:] = model
    return n, first, n_new, src, left_out


def compound_of(table, piece):
    return int(np.searchsorted(np.asarray(table), piece, side="right")) - 1


CLICK1_ORIGIN = (SHIFT_B + np.float32([1.5, 1.0, 0.5])).astype(np.float32)
CLICK1_KW = dict(partial=True, sphere_points=sphere_cloud(CLICK1_ORIGIN, 1.0), origin=CLICK1_ORIGIN, radius=1.0)


def click_one(E, eng, world, use_async=False):
    cube = bodies(E)["cube"]

    def conditions(ro, rp, rev):
        # MergeOutOfImpact moved at least one fragment to bind 0 (nothing was masked: every member of bind 0 is a fragment),
        # and at least one compound besides bind 0 remains
        assert ro[1] - ro[0] >= 1 and len(ro) - 1 >= 2, (ro, rp)
    place = (cube["scale"], (cube["translate"] + SHIFT_B).astype(np.float32))
    return click(E, eng, world, 1, cube, place, None, CLICK1_KW, conditions, use_async)


def click_two(E, eng, world, first_new):
    """pieces_raycast picks a piece of a compound click 1 made; another piece of that compound is masked; the 64-cell pattern."""
    table = eng.scene_compounds()
    made = [c for c in range(first_new, len(world)) if len(world[c]) >= 2]
    assert made
    aim = np.asarray(world[made[0]][0]["conv"]["pos"], np.float64).mean(0)
    d = np.array([0.0, 0.0, -1.0])
    hit = eng.pieces_raycast([list(aim - 20 * d) + list(d) + [100.0]])[0]
    assert hit["piece"] >= 0
    target = compound_of(table, int(hit["piece"]))
    assert target >= first_new and len(world[target]) >= 2, (target, first_new, [len(c) for c in world])
    local = int(hit["piece"]) - int(table[target])
    mask = np.zeros(len(world[target]), np.uint8)
    mask[(local + 1) % len(mask)] = 1
    pos = np.concatenate([p["mesh"]["pos"] for k, p in enumerate(world[target]) if not mask[k]])
    lo, hi = pos.min(0), pos.max(0)
    place = ((hi - lo).astype(np.float32), ((hi.astype(np.float64) + lo.astype(np.float64)) / 2).astype(np.float32))
    origin = (hit["pos"] + np.float32([0, 0, -0.5])).astype(np.float32)
    kw = dict(partial=True, sphere_points=sphere_cloud(origin, 1.5), origin=origin, radius=1.5)

    def conditions(ro, rp, rev):
        assert rp[0] == 0 and ro[1] >= 1                    # the skipped piece is piece 0, in bind 0
    out = click(E, eng, world, target, bodies(E)["blob"], place, mask, kw, conditions)
    assert out[0] > 64
    return out


def check_queries_against_fresh_engine(E, eng, world):
    """pieces_mass, pieces_raycast and pieces_overlap on the committed scene equal the same calls on a fresh engine given the
    downloaded pieces."""
    table, got = snapshot(eng)
    fresh = E.Engine(0)
    fresh.upload_pieces([m for m, _ in got], [c for _, c in got])
    for s in (0, 1):
        assert eng.pieces_mass(set=s).tobytes() == fresh.pieces_mass(set=s).tobytes()
    cen = np.asarray([np.asarray(c["pos"], np.float64).mean(0) for _, c in got])
    rng = np.random.default_rng(3)
    pick = rng.choice(len(got), 24)
    dirs = rng.normal(size=(24, 3)); dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    rays = np.c_[cen[pick] - 50 * dirs, dirs, np.full(24, 1000.0)].astype(np.float32)
    a, b = eng.pieces_raycast(rays), fresh.pieces_raycast(rays)
    assert a.tobytes() == b.tobytes() and (a["piece"] >= 0).any()
    spheres = np.c_[cen[pick[:8]], np.linspace(0.1, 4.0, 8)].astype(np.float32)
    mass = eng.pieces_mass(set=1)
    ma, mb = eng.pieces_overlap(spheres, mass=mass, min_mass=float(np.median(mass["mass"]))), fresh.pieces_overlap(spheres, mass=mass, min_mass=float(np.median(mass["mass"])))
    assert ma.tobytes() == mb.tobytes() and ma.any()
    fresh.close()


def run_two_clicks(E, use_async=False):
    eng, world = three_bodies(E)
    n, first, n_new, src, _ = click_one(E, eng, world, use_async)
    assert first == 2 and n_new >= 2 and list(src[:2]) == [0, 2]       # the body above the target moved down by one
    n2, first2, n_new2, src2, _ = click_two(E, eng, world, first)
    check_queries_against_fresh_engine(E, eng, world)
    eng.close()
    return n, n2


def run_transform(E):
    """scene_transform_compound leaves the untouched bodies' bits alone and equals transform_pieces with identity for the rest."""
    eng, world = three_bodies(E)
    other, _ = three_bodies(E)
    ang = 0.3
    W = np.eye(4, dtype=np.float32)
    W[:3, :3] = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]], np.float32)
    W[:3, 3] = [0.5, -2.0, 1.25]
    before = snapshot(eng)
    eng.scene_transform_compound(1, [W])
    other.transform_pieces([np.eye(4, dtype=np.float32), W, np.eye(4, dtype=np.float32)])
    table, got = snapshot(eng)
    _, want = snapshot(other)
    assert list(table) == [0, 1, 2, 3]
    for p in (0, 2):
        assert same_solid(got[p][0], before[1][p][0]) and same_solid(got[p][1], before[1][p][1])
    for s in (0, 1):
        assert same_solid(got[1][s], want[1][s]) and not same_solid(got[1][s], before[1][1][s])
    # the derived data was rebuilt: the queries see the moved body
    rays = np.asarray([[10.5, -2.0, 40, 0, 0, -1, 100], [0, 0, 40, 0, 0, -1, 100], [0, 300, 200, 0, 0, -1, 1000]], np.float32)
    assert eng.pieces_raycast(rays).tobytes() == other.pieces_raycast(rays).tobytes()
    assert list(eng.pieces_raycast(rays)["piece"]) == [1, 0, 2]
    for bad in (lambda: eng.scene_transform_compound(3, [W]), lambda: eng.scene_transform_compound(1, [W, W])):
        with pytest.raises(engine.SurtrError) as e:
            bad()
        assert e.value.code == engine.E_INVALID
    eng.close(); other.close()


def run_existing_behaviour(E):
    """A context that never had a scene call: the 8-cell cube event is the fixture's, a masked event regroups as the host
    regrouping (surtr_regroup) of its solids does, and blob64 has the digest of tests/golden/digests.json."""
    g = np.load(os.path.join(GOLDEN, "cube8.npz"))
    b = bodies(E)
    cube = b["cube"]
    eng = E.Engine(0)
    eng.upload_pieces(b["meshes"][:2], b["convexes"][:2])
    eng.upload_planes(g["face_off"], g["planes"])
    c = eng.fracture_event(0, 8, outside=[0, 1], flags=3)       # (the fixture's event: refit + render)
    assert c.n_pairs == 16
    ev = eng.download()
    for k in ("mesh_vert_off", "mesh_pos", "mesh_nbr_off", "mesh_nbr", "conv_vert_off", "conv_pos", "conv_nbr_off", "conv_nbr", "idx_off", "idx"):
        assert np.array_equal(ev[k].reshape(-1), g["out_" + k].reshape(-1)), k
    assert np.array_equal(ev["frag_ids"], g["out_frag_ids"].reshape(-1, 3))
    co, cp = eng.event_regroup(**dict(CLICK1_KW, origin=CLICK1_ORIGIN - SHIFT_B, sphere_points=sphere_cloud(CLICK1_ORIGIN - SHIFT_B, 1.0)))
    _, fc = scenes.fragments_as_pieces(ev)
    ho, hp = engine.regroup([b["convexes"][1]] + fc, [-1] + list(ev["frag_ids"][:, 0]), n_outside=1, partial=True,
                            sphere_points=sphere_cloud(CLICK1_ORIGIN - SHIFT_B, 1.0), origin=CLICK1_ORIGIN - SHIFT_B, radius=1.0)
    assert list(co) == list(ho) and list(cp) == list(hp) and cp[0] == 0
    eng.close()
    want = json.load(open(os.path.join(GOLDEN, "digests.json")))["blob64"]
    blob = b["blob"]
    eng = E.Engine(0)
    eng.upload_pieces([blob["mesh"]], [blob["convex"]])
    eng.upload_pattern(blob["face_off"], blob["v012"])
    eng.place_cells(blob["scale"], blob["translate"])
    c = eng.fracture_event(0, 64, outside=[0])
    ev = eng.download()
    assert c.n_frag == want["n_frag"]
    for k in ("frag_ids", "mesh_vert_off", "mesh_pos", "mesh_nbr_off", "mesh_nbr", "conv_vert_off", "conv_pos", "conv_nbr_off", "conv_nbr", "idx_off", "idx"):
        assert hashlib.sha256(np.ascontiguousarray(ev[k]).tobytes()).hexdigest() == want[k], k
    eng.close()


def run_errors(E):
    eng, world = three_bodies(E)
    cube = bodies(E)["cube"]
    before = snapshot(eng)
    co1, cp1 = np.array([0, 0, 1], np.uint32), np.array([0], np.int32)

    def refused(code, call):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == code, e.value
        assert_unchanged(eng, before)
    # tables that are no tables
    for bad in ([0, 1, 3, 2], [1, 2, 3], [0, 1, 2], [0, 1, 1, 3], [0, 1, 2, 4], [0]):
        refused(engine.E_INVALID, lambda: eng.scene_set_compounds(bad))
    refused(engine.E_STATE, lambda: eng.scene_fracture_event(1, 0, 8))         # no planes yet
    # no scene event: nothing yet, then an ordinary event
    refused(engine.E_STATE, lambda: eng.scene_commit(co1, cp1))
    eng.upload_pattern(cube["face_off"], cube["v012"])
    eng.place_cells(cube["scale"], (cube["translate"] + SHIFT_B).astype(np.float32))
    refused(engine.E_INVALID, lambda: eng.scene_fracture_event(3, 0, 8))
    refused(engine.E_INVALID, lambda: eng.scene_fracture_event(1, 0, 9))
    refused(engine.E_INVALID, lambda: eng.scene_fracture_event(1, 0, 8, outside=[0, 0]))
    eng.fracture_event(0, 8, outside=[1, 0, 1], flags=0)
    co, cp = eng.event_regroup()
    refused(engine.E_STATE, lambda: eng.scene_commit(co, cp))
    # an event that failed: an arena too small for its fragments
    eng.set_arena(64, 256, 64)
    with pytest.raises(engine.SurtrError) as e:
        eng.scene_fracture_event(1, 0, 8, flags=0)
    assert e.value.code == engine.E_CAPACITY
    refused(engine.E_STATE, lambda: eng.scene_commit(co, cp))
    eng.set_arena(0, 0, 0)
    # transformed, replaced, or given another table since the event
    for spoil in (lambda: eng.scene_transform_compound(0, [np.eye(4, dtype=np.float32)]),
                  lambda: eng.upload_pieces(bodies(E)["meshes"], bodies(E)["convexes"]) or eng.scene_set_compounds([0, 1, 2, 3]),
                  lambda: eng.scene_set_compounds([0, 1, 2, 3])):
        eng.scene_fracture_event(1, 0, 8, flags=0)
        co, cp = eng.event_regroup()
        spoil()
        refused(engine.E_STATE, lambda: eng.scene_commit(co, cp))
    # compounds that do not cover the pieces exactly once
    c = eng.scene_fracture_event(1, 0, 8, flags=0)
    co, cp = eng.event_regroup()
    assert co[1] == 0 and co[-1] == c.n_frag == 8          # bind 0 is empty: that compound must not be created
    dup = cp.copy(); dup[1] = dup[0]
    high = cp.copy(); high[0] = 8
    for bco, bcp in ((co[:-1], cp), (co, dup), (co, high), (np.r_[co[:-1], co[-1] + 1].astype(np.uint32), np.r_[cp, 0].astype(np.int32))):
        refused(engine.E_INVALID, lambda: eng.scene_commit(bco, bcp))
    # ... and the good ones still commit, once
    n, first, n_new, src = eng.scene_commit(co, cp)
    assert (n, first, n_new) == (10, 2, len(co) - 2) and list(src) == [0, 2] + [-(int(f) + 1) for f in cp]
    assert list(eng.scene_compounds()) == [0, 1] + [2 + int(x) for x in co[1:]]
    after = snapshot(eng)
    before = after
    refused(engine.E_STATE, lambda: eng.scene_commit(co, cp))
    eng.close()


def run_unsolid(E):
    """The fragment of tests/golden/nonterminating_faces_fragment.npz whose faces cannot be extracted is flagged by a render
    event: it is left out, and with every piece in a compound of its own, its compound is not created."""
    d = np.load(os.path.join(GOLDEN, "nonterminating_faces_fragment.npz"))
    piece = {"mesh": {"pos": d["mesh_pos"], "off": d["mesh_off"], "nbr": d["mesh_nbr"]}, "conv": {"pos": d["conv_pos"], "off": d["conv_off"], "nbr": d["conv_nbr"]}}
    b = bodies(E)
    far = {"mesh": shifted(b["meshes"][0], [1000, 0, 0]), "conv": shifted(b["convexes"][0], [1000, 0, 0])}
    world = [[far], [piece]]
    eng = E.Engine(0)
    eng.upload_pieces([far["mesh"], piece["mesh"]], [far["conv"], piece["conv"]])
    eng.scene_set_compounds([0, 1, 2])
    fo = d["fo"].astype(np.uint32)
    pattern = {"face_off": fo, "planes": d["planes"], "n_cells": len(fo) - 1}

    def conditions(ro, rp, rev):
        assert np.count_nonzero(rev["frag_status"]) == 1 and rev["frag_ids"].shape[0] >= 4
    n, first, n_new, src, left_out = click(E, eng, world, 1, pattern, None, None, {}, conditions, flags=3, singletons=True)
    c = eng.event_counts()
    assert left_out == 1 and n_new == c.n_frag - 1 and n == c.n_frag and first == 1
    eng.close()


def run_steady_allocations(E):
    """The same scene committed again: no allocation from the second commit on."""
    eng, world = three_bodies(E)
    b, cube = bodies(E), bodies(E)["cube"]
    allocs = []
    for _ in range(3):
        eng.upload_pieces(b["meshes"], b["convexes"])
        eng.scene_set_compounds([0, 1, 2, 3])
        eng.upload_pattern(cube["face_off"], cube["v012"])
        eng.place_cells(cube["scale"], (cube["translate"] + SHIFT_B).astype(np.float32))
        eng.scene_fracture_event(1, 0, 8, flags=0)
        co, cp = eng.event_regroup(**CLICK1_KW)
        eng.event_refit()
        eng.scene_commit(co, cp)
        allocs.append(eng.upload_stats()[1])
    assert allocs[0] > 0 and allocs[1:] == [0, 0], allocs
    eng.close()


# ------------------------------------------------------------------ CPU tier (emulation)
def test_two_clicks_against_both_references(emul_engine):
    n, n2 = run_two_clicks(emul_engine)
    print("resident pieces after click 1:", n, "after click 2:", n2)


def test_untouched_bodies_keep_their_bits(emul_engine):
    run_transform(emul_engine)


def test_existing_behaviour_without_a_scene_call(emul_engine):
    run_existing_behaviour(emul_engine)


def test_errors_leave_the_scene_unchanged(emul_engine):
    run_errors(emul_engine)


def test_flagged_fragment_and_its_compound_are_left_out(emul_engine):
    run_unsolid(emul_engine)


def test_steady_commits_do_not_allocate(emul_engine):
    run_steady_allocations(emul_engine)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_scene as T
    case = sys.argv[1]
    if case == "clicks":
        print(T.run_two_clicks(engine))
    elif case == "async":
        T.run_async(engine, torch)
    elif case == "harness":
        T.check_harness(engine, %(root)r)
    else:
        getattr(T, "run_" + case)(engine)
    print("ok", case)
""")


def run_async(E, torch):
    """The _async event on a stream of its own, with the lean arrangement of six events in flight: click 1 against (a) and (b)."""
    st = torch.cuda.Stream()
    eng, world = three_bodies(E)
    eng.set_stream(st.cuda_stream)
    eng.set_events_in_flight(6)
    with torch.cuda.stream(st):
        click_one(E, eng, world, use_async=True)
    st.synchronize()
    eng.close()


def lattice_cloud():
    """The 26 directions of the 3 x 3 x 3 lattice, unit length: the sphere point cloud of surtr_harness --scene-clicks."""
    v = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], np.float64)
    return (v / np.sqrt((v * v).sum(1))[:, None]).astype(np.float32)


def python_click(eng, o, d, r, n_cells):
    """OnMouseDown (single mode, partial) through the Python calls, in float as the host layer computes it."""
    hit = eng.pieces_raycast([list(o) + list(d) + [1000.0]])[0]
    assert hit["piece"] >= 0
    r32 = np.float32(r)
    impact = (hit["pos"] + np.asarray(d, np.float32) * np.float32(0.01)).astype(np.float32)
    table = eng.scene_compounds()
    comp = compound_of(table, int(hit["piece"]))
    cloud = (lattice_cloud() * r32 + impact).astype(np.float32)
    mask = [engine.convex_out_of_sphere(eng.download_piece(p, 1), cloud, impact, float(r32)) for p in range(int(table[comp]), int(table[comp + 1]))]
    eng.place_cells([r32 * np.float32(2)] * 3, impact)
    eng.scene_fracture_event(comp, 0, n_cells, outside=np.asarray(mask, np.uint8) if any(mask) else None, flags=0)
    co, cp = eng.event_regroup(partial=True, sphere_points=cloud, origin=impact, radius=float(r32))
    eng.event_refit()
    n, first, n_new, _ = eng.scene_commit(co, cp)
    table = eng.scene_compounds()
    mass = engine.combine_mass(table, np.arange(n, dtype=np.int32), eng.pieces_mass(set=1))["mass"]
    return dict(click=None, hit_piece=int(hit["piece"]), compounds_hit=[comp], compounds_made=list(range(first, first + n_new)),
                table=[int(x) for x in table], mass=[float(x) for x in mass])


def check_harness(E, root, exe=None):
    """surtr_harness --scene-clicks (FractureEngine::OnMouseDown) against the same clicks through the Python calls."""
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    clicks = [([-10.0, 0.3, 0.2], [1.0, 0.0, 0.0]), ([0.3, 0.2, 10.0], [0.0, 0.0, -1.0])]
    arg = ";".join(",".join("%r" % x for x in o + d) for o, d in clicks)
    p = subprocess.run([exe, "--mesh", "cube", "--cells", "8", "--scene-clicks", arg, "--impact-radius", "2.0"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [json.loads(x) for x in p.stdout.strip().splitlines() if x.startswith('{"click"')]
    assert len(lines) == len(clicks)
    sc = scenes.cube_scene(8)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, 8)
    n = eng.pieces_from_event()
    eng.scene_set_compounds(list(range(0, n, 2)) + [n])
    for k, (o, d) in enumerate(clicks):
        want = dict(python_click(eng, o, d, 2.0, 8), click=k)
        assert lines[k] == want, (lines[k], want)
        assert len(want["compounds_made"]) >= 1 and want["table"][-1] > n
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["clicks", "transform", "existing_behaviour", "errors", "unsolid", "steady_allocations", "async"])
def test_gpu_scene(case):
    run_gpu_child(GPU_CHILD, case, 120)


@pytest.mark.gpu
def test_gpu_harness_scene_clicks():
    run_gpu_child(GPU_CHILD, "harness", 150)
