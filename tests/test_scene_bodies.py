"""One click, several bodies: scene_outside (k_scene_outside), scene_apply_poses, scene_fracture_bodies, event_regroup_bodies and the
one scene_commit after them (scene_dev.hip, regroup_dev.hip).

THE REFERENCE IS THE ONE-BODY CODE.  A second engine is given the same scene and runs the calls that existed before, per target in
descending compound number: scene_apply_pose, download_piece + engine.convex_out_of_sphere (the host mask), scene_fracture_event,
event_regroup, event_refit, scene_commit.  Everything is compared bit for bit and without a tolerance: every resident piece of both
sets, the compound table, the poses, scene_mass, and src after composing the sequential commits' src arrays.  The compounds of
event_regroup_bodies are compared body by body with the reference's event_regroup outputs (the piece numbers are translated: the
bodies call numbers the skipped pieces of all targets ascending, then all fragments target after target).

Scene: test_scene.three_bodies, then its click 1, which leaves [cube], [blob with its ACH Convex], a compound of five fragments and
three compounds of one fragment each.  The click under test is a radial one with the 8-cell pattern on compounds 4, 2 and 0: not
adjacent in number, a one-piece body (0) and a five-piece compound (2) two of whose pieces the device mask keeps out.

The CPU tier runs on the emulation library (conftest's emul_engine); the GPU tier runs the same cases on the MI355X in child
processes under a time limit (helpers.run_gpu_child)."""
import json
import os
import subprocess
import textwrap

import numpy as np
import pytest

import test_pick_queries as PQ
import test_scene as TS
import test_scene_poses as TP
from helpers import run_gpu_child
from surtr_amd import engine, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)

# the click under test: between the cube at the origin and what click 1 left of the cube at x = 10
# (found on the CPU tier: of compound 2's five pieces two stay out of the sphere, four of compound 4's fragments move to its bind 0, and
# all three targets produce fragments -- asserted on the sequential reference in click_conditions)
CLICK_ORIGIN = np.float32([6.0, 0.0, 0.7])
CLICK_RADIUS = 4.0
CLICK_TARGETS = [4, 2, 0]
# a second click on the same targets, for the rules that hold PER BODY (found on the CPU tier as well): here it is compound 2, the SECOND
# target, that has a fragment moved to its own bind 0 and whose binds HandleConvexIsland splits into extra groups -- a regrouping
# that sent either to the first body would differ from the reference (asserted on the sequential reference in click_conditions)
OWNER_ORIGIN = np.float32([8.0, 1.0, 0.0])
OWNER_RADIUS = 5.5
# (origin, radius) of the mask test: the click's own sphere, one between the cubes, two small ones inside the broken cube, one that swallows both cubes, one
# inside the blob (no vertex near: a cloud point decides)
MASK_SPHERES = [((6.0, 0.0, 0.7), 4.0), ((5.0, 0.0, 0.0), 5.5), ((9.0, 0.5, 0.3), 1.2), ((10.5, 0.2, 0.1), 0.8), ((8.5, 0.0, 0.0), 9.2), ((10.0, 300.0, 0.0), 1.0)]


# the pattern stretched along x and moved off the cubes' centres: some cell is long enough to reach into both cubes
BOUNDARY_PLACE = (np.float32([48.0, 12.0, 12.0]), np.float32([-7.0, 0.5, 0.5]))


# ------------------------------------------------------------------ helpers
def scene_after_click_one(E, poses=None):
    """-> engine holding three_bodies after test_scene's click 1 (table [0, 1, 2, 7, 8, 9, 10])."""
    eng, world = TS.three_bodies(E)
    TS.click_one(E, eng, world)
    assert [len(c) for c in world] == [1, 1, 5, 1, 1, 1], [len(c) for c in world]
    if poses is not None:
        eng.scene_set_poses(poses)
    return eng


def twin(E, eng):
    """A second engine with the same resident bits, table and poses (given what download_piece reads)."""
    table, got = TS.snapshot(eng)
    other = E.Engine(0)
    other.upload_pieces([m for m, _ in got], [c for _, c in got])
    other.scene_set_compounds(table)
    other.scene_set_poses(eng.scene_poses())
    return other


def place_click(eng, cube, origin, radius):
    """The placement of OnMouseDown: the pattern scaled to the impact's diameter, centred on the impact."""
    eng.upload_pattern(cube["face_off"], cube["v012"])
    eng.place_cells([np.float32(radius) * np.float32(2)] * 3, np.asarray(origin, np.float32))


def host_mask(eng, compounds, cloud, origin, radius):
    table = eng.scene_compounds()
    return np.asarray([engine.convex_out_of_sphere(eng.download_piece(p, 1), cloud, origin, radius)
                       for c in compounds for p in range(int(table[c]), int(table[c + 1]))], np.uint8)


def sequential(ref, targets, cells, partial, cloud, origin, radius):
    """The reference: the one-body calls per target, descending.  -> per target dict(mask, co, cp, n_frag, cells), and `origin_of`:
    for every piece of the final scene ('old', piece of the scene before the click) or ('frag', target index, fragment)."""
    assert list(targets) == sorted(targets, reverse=True)
    origin_of = [("old", p) for p in range(int(ref.scene_compounds()[-1]))]
    out = []
    kw = dict(partial=True, sphere_points=cloud, origin=origin, radius=radius) if partial else {}
    for k, t in enumerate(targets):
        ref.scene_apply_pose(t)
        mask = host_mask(ref, [t], cloud, origin, radius) if partial else None
        c = ref.scene_fracture_event(t, cells[0], cells[1], outside=mask if mask is not None and mask.any() else None, flags=0)
        co, cp = ref.event_regroup(**kw)
        ref.event_refit()
        ids = ref.download()["frag_ids"].reshape(-1, 3)
        n, first, n_new, src = ref.scene_commit(co, cp)
        origin_of = [origin_of[s] if s >= 0 else ("frag", k, -int(s) - 1) for s in src]
        out.append(dict(mask=np.zeros(0, np.uint8) if mask is None else mask, co=co, cp=cp, n_frag=int(c.n_frag), cells=ids[:, 0].copy(),
                        n_skip=0 if mask is None else int(np.count_nonzero(mask))))
    return out, origin_of


def assert_same_scene(eng, ref):
    (ta, ga), (tb, gb) = TS.snapshot(eng), TS.snapshot(ref)
    assert list(ta) == list(tb), (ta, tb)
    for p, ((m, c), (m0, c0)) in enumerate(zip(ga, gb)):
        assert TS.same_solid(m, m0), ("mesh", p)
        assert TS.same_solid(c, c0), ("conv", p)
    assert eng.scene_poses().tobytes() == ref.scene_poses().tobytes()
    for s in (0, 1):
        assert eng.scene_mass(set=s).tobytes() == ref.scene_mass(set=s).tobytes()


def bodies_click(E, eng, ref, targets, cells, partial, cloud, origin, radius, conditions=None, use_async=False):
    """The click on `eng` through the new calls, on `ref` through the one-body calls; everything compared.  -> (seq, made)."""
    table0 = [int(x) for x in eng.scene_compounds()]
    seq, origin_of = sequential(ref, targets, cells, partial, cloud, origin, radius)
    if conditions is not None:
        conditions(seq)                                    # on the reference alone
    eng.scene_apply_poses(targets)
    mask = eng.scene_outside(targets, cloud, origin, radius) if partial else None
    if partial:
        assert mask.tobytes() == np.concatenate([s["mask"] for s in seq]).tobytes()
    if use_async:
        eng.scene_fracture_bodies_async(targets, cells[0], cells[1], outside=mask, flags=0)
        c = eng.event_counts()
    else:
        c = eng.scene_fracture_bodies(targets, cells[0], cells[1], outside=mask, flags=0)
    assert c.status == 0 and c.n_frag == sum(s["n_frag"] for s in seq)
    assert c.n_pairs == (cells[1] - cells[0]) * sum(table0[t + 1] - table0[t] for t in targets)
    ids = eng.download()["frag_ids"].reshape(-1, 3)
    # frag_ids: resident piece numbers, target-major, and per target the cells of its own event
    frag_off = np.cumsum([0] + [s["n_frag"] for s in seq])
    for k, t in enumerate(targets):
        mine = ids[frag_off[k]:frag_off[k + 1]]
        assert ((mine[:, 1] >= table0[t]) & (mine[:, 1] < table0[t + 1])).all() and list(mine[:, 0]) == list(seq[k]["cells"])
    kw = dict(partial=True, sphere_points=cloud, origin=origin, radius=radius) if partial else {}
    co, cp, bo = eng.event_regroup_bodies(**kw)
    co1, cp1 = eng.event_regroup(**kw)
    assert list(co1) == list(co) and list(cp1) == list(cp)
    # body by body against the reference's event_regroup: translate the piece numbers
    skipped = [p for t in sorted(targets) for j, p in enumerate(range(table0[t], table0[t + 1]))
               if partial and seq[targets.index(t)]["mask"][j]]
    assert len(bo) == len(targets) + 1 and bo[0] == 0 and bo[-1] == len(co) - 1
    for k, t in enumerate(targets):
        mine = [q for q, p in enumerate(skipped) if table0[t] <= p < table0[t + 1]]
        assert len(mine) == seq[k]["n_skip"]

        def local(q):
            if q < len(skipped):
                return mine.index(q)
            f = q - len(skipped)
            assert frag_off[k] <= f < frag_off[k + 1], (k, q)
            return seq[k]["n_skip"] + f - int(frag_off[k])
        got = [[local(int(q)) for q in cp[co[i]:co[i + 1]]] for i in range(int(bo[k]), int(bo[k + 1]))]
        want = [[int(q) for q in seq[k]["cp"][seq[k]["co"][i]:seq[k]["co"][i + 1]]] for i in range(len(seq[k]["co"]) - 1)]
        assert got == want, (k, got, want)
    eng.event_refit()
    n, first, n_new, src = eng.scene_commit(co, cp)
    assert first == len(table0) - 1 - len(targets) and n == int(ref.scene_compounds()[-1]) and first + n_new == len(ref.scene_compounds()) - 1
    got_origin = [("old", int(s)) if s >= 0 else ("frag", int(np.searchsorted(frag_off, -int(s) - 1, side="right")) - 1, None) for s in src]
    got_origin = [o if o[0] == "old" else ("frag", o[1], -int(s) - 1 - int(frag_off[o[1]])) for o, s in zip(got_origin, src)]
    assert got_origin == origin_of
    assert_same_scene(eng, ref)
    return seq, list(range(first, first + n_new))


# ------------------------------------------------------------------ 1. the mask
def run_mask(E, torch=None):
    eng = scene_after_click_one(E)
    table = eng.scene_compounds()
    nc = len(table) - 1
    every, subset = list(range(nc)), [5, 3, 0]
    convs = [eng.download_piece(p, 1) for p in range(int(table[-1]))]
    halves = [int(np.asarray(c["nbr"]).shape[0]) for c in convs]
    assert min(halves) <= 64 and halves[0] == 24 and max(halves) > 64 and halves[1] > 64, halves      # the cube; the blob's ACH Convex
    seen, by_vertex, by_cloud = set(), 0, 0
    for origin, radius in MASK_SPHERES:
        origin = np.float32(origin)
        for ns in (0, 1, 64, 100):
            cloud = TS.sphere_cloud(origin, radius, ns) if ns else np.zeros((0, 3), np.float32)
            want = np.asarray([engine.convex_out_of_sphere(c, cloud, origin, radius) for c in convs], np.uint8)
            far = [bool((np.sqrt(((c["pos"].astype(np.float64) - origin) ** 2).sum(1)) > radius * (1 + 1e-5)).all()) for c in convs]
            near = [bool((np.sqrt(((c["pos"].astype(np.float64) - origin) ** 2).sum(1)) < radius * (1 - 1e-5)).any()) for c in convs]
            seen |= set(int(w) for w in want)
            by_vertex += sum(1 for w, v in zip(want, near) if not w and v)
            by_cloud += sum(1 for w, v in zip(want, far) if not w and v)
            got = eng.scene_outside(every, cloud, origin, radius)
            assert got.dtype == np.uint8 and got.tobytes() == want.tobytes(), (origin, radius, ns, got, want)
            sub = eng.scene_outside(subset, cloud, origin, radius)
            pick = np.concatenate([np.arange(table[c], table[c + 1]) for c in subset])
            assert sub.tobytes() == want[pick].tobytes(), (origin, radius, ns)
            if torch is None:            # the _dev form on the emulation: its "device" memory is the host's
                d_c = np.ascontiguousarray(cloud) if ns else np.zeros(3, np.float32)
                d_o = np.full(len(want) + 3, 7, np.uint8)
                eng.scene_outside_dev(every, ns, d_c.ctypes.data, origin, radius, d_o.ctypes.data, len(want))
                assert d_o[:len(want)].tobytes() == want.tobytes() and (d_o[len(want):] == 7).all()
                with pytest.raises(engine.SurtrError) as e:
                    eng.scene_outside_dev(every, ns, d_c.ctypes.data, origin, radius, d_o.ctypes.data, len(want) - 1)
                assert e.value.code == engine.E_CAPACITY and (d_o[len(want):] == 7).all()
            else:                        # the _dev form: cloud and mask in device memory
                d_c = torch.from_numpy(np.ascontiguousarray(cloud)).cuda() if ns else torch.zeros(3, dtype=torch.float32, device="cuda")
                d_o = torch.full((len(want) + 3,), 7, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                eng.scene_outside_dev(every, ns, d_c.data_ptr(), origin, radius, d_o.data_ptr(), len(want))
                torch.cuda.synchronize()
                back = d_o.cpu().numpy()
                assert back[:len(want)].tobytes() == want.tobytes() and (back[len(want):] == 7).all()
    assert seen == {0, 1} and by_vertex >= 1 and by_cloud >= 1, (seen, by_vertex, by_cloud)
    eng.close()


# ------------------------------------------------------------------ 2. the click
def moved_to_bind0(s):
    """Fragments in bind 0 (the first compound) of one target's event_regroup: MergeOutOfImpact moved them there."""
    return sum(1 for q in s["cp"][s["co"][0]:s["co"][1]] if int(q) >= s["n_skip"])


def island_groups(s):
    """Extra groups HandleConvexIsland made in one target's event_regroup: compounds after bind 0 that hold a skipped piece (split off
    bind 0), and compounds beyond the first that hold fragments of one cell (split off that cell's bind)."""
    n, per_cell = 0, {}
    for i in range(1, len(s["co"]) - 1):
        members = [int(q) for q in s["cp"][s["co"][i]:s["co"][i + 1]]]
        if any(q < s["n_skip"] for q in members):
            n += 1
            continue
        for c in set(int(s["cells"][q - s["n_skip"]]) for q in members):
            per_cell[c] = per_cell.get(c, 0) + 1
    return n + sum(v - 1 for v in per_cell.values() if v > 1)


def click_conditions(partial, later_body=False):
    def check(seq):
        assert sum(1 for s in seq if s["n_frag"] > 0) >= 2
        if later_body:      # a target that is not the first: a fragment moved to ITS bind 0, and an extra island group of ITS binds
            assert any(moved_to_bind0(s) > 0 for s in seq[1:]), [moved_to_bind0(s) for s in seq]
            assert any(island_groups(s) > 0 for s in seq[1:]), [island_groups(s) for s in seq]
            return
        if partial:
            assert any(s["n_skip"] > 0 for s in seq)                                        # a target keeps a skipped piece
            assert any(0 < s["n_skip"] < len(s["mask"]) for s in seq if len(s["mask"]) > 1)   # some pieces of a multi-piece compound masked
            # a fragment moved to bind 0: bind 0 (the first compound) holds a piece that is no skipped one
            assert any(any(int(q) >= s["n_skip"] for q in s["cp"][s["co"][0]:s["co"][1]]) for s in seq)
    return check


def run_click(E, partial=True, use_async=False, later_body=False):
    eng = scene_after_click_one(E)
    ref = twin(E, eng)
    cube = TS.bodies(E)["cube"]
    origin, radius = (OWNER_ORIGIN, OWNER_RADIUS) if later_body else (CLICK_ORIGIN, CLICK_RADIUS)
    cloud = TS.sphere_cloud(origin, radius)
    for e in (eng, ref):
        place_click(e, cube, origin, radius)
    table = eng.scene_compounds()
    sizes = [int(table[t + 1] - table[t]) for t in CLICK_TARGETS]
    assert len(CLICK_TARGETS) >= 3 and 1 in sizes and max(sizes) > 1 and all(a - b > 1 for a, b in zip(CLICK_TARGETS, CLICK_TARGETS[1:]))
    seq, made = bodies_click(E, eng, ref, CLICK_TARGETS, (0, 8), partial, cloud, origin, radius, click_conditions(partial, later_body), use_async)
    eng.close(); ref.close()
    return [s["n_frag"] for s in seq], len(made)


def run_click_later_body(E):
    return run_click(E, partial=True, later_body=True)


# ------------------------------------------------------------------ 3. equal cells at a body boundary
def run_boundary(E):
    """Two one-piece targets, one cell that cuts both: the last cell of the first body is the first cell of the second."""
    b = TS.bodies(E)
    cube = b["cube"]
    eng, ref = E.Engine(0), E.Engine(0)
    for e in (eng, ref):
        e.upload_pieces(b["meshes"], b["convexes"])
        e.scene_set_compounds([0, 1, 2, 3])
        e.upload_pattern(cube["face_off"], cube["v012"])
        e.place_cells(*BOUNDARY_PLACE)
    hits = [cell for cell in range(8) if all(ref.scene_fracture_event(t, cell, cell + 1, flags=0).n_frag > 0 for t in (1, 0))]
    assert hits, "no cell of the placement cuts both cubes"
    cell = hits[0]

    def conditions(seq):
        assert all(s["n_frag"] >= 1 and set(s["cells"]) == {cell} for s in seq)      # both targets produced a fragment of that cell
    seq, made = bodies_click(E, eng, ref, [1, 0], (cell, cell + 1), False, None, None, None, conditions)
    # the two bodies' fragments ended in different compounds
    table = eng.scene_compounds()
    assert len(made) >= 2 and int(table[-1]) - int(table[made[0]]) == sum(s["n_frag"] for s in seq)
    eng.close(); ref.close()


# ------------------------------------------------------------------ 4. one target
def run_one_target(E):
    cube = TS.bodies(E)["cube"]
    cloud = TS.sphere_cloud(CLICK_ORIGIN, CLICK_RADIUS)
    kw = dict(partial=True, sphere_points=cloud, origin=CLICK_ORIGIN, radius=CLICK_RADIUS)
    for target in (2, 0):
        eng = scene_after_click_one(E)
        ref = twin(E, eng)
        for e in (eng, ref):
            place_click(e, cube, CLICK_ORIGIN, CLICK_RADIUS)
        mask = host_mask(ref, [target], cloud, CLICK_ORIGIN, CLICK_RADIUS)
        ca = eng.scene_fracture_bodies([target], 0, 8, outside=mask, flags=0)
        cb = ref.scene_fracture_event(target, 0, 8, outside=mask, flags=0)
        assert bytes(ca) == bytes(cb)
        co, cp, bo = eng.event_regroup_bodies(**kw)
        co1, cp1 = eng.event_regroup(**kw)
        ro, rp = ref.event_regroup(**kw)
        assert list(co) == list(ro) == list(co1) and list(cp) == list(rp) == list(cp1) and list(bo) == [0, len(ro) - 1]
        eng.event_refit(); ref.event_refit()
        ea, eb = eng.download(), ref.download()
        for k in TS.EVENT_KEYS + ("frag_ids",):
            assert np.asarray(ea[k]).tobytes() == np.asarray(eb[k]).tobytes(), k
        a, b = eng.scene_commit(co, cp), ref.scene_commit(ro, rp)
        assert a[:3] == b[:3] and list(a[3]) == list(b[3])
        assert_same_scene(eng, ref)
        # after a one-body event event_regroup_bodies returns event_regroup's compounds and one body
        ref.scene_fracture_event(0, 0, 8, flags=0)
        ro, rp = ref.event_regroup(**kw)
        co, cp, bo = ref.event_regroup_bodies(**kw)
        assert list(co) == list(ro) and list(cp) == list(rp) and list(bo) == [0, len(ro) - 1]
        eng.close(); ref.close()


# ------------------------------------------------------------------ 5. poses
def run_poses(E):
    move4 = TP.pose_about(TP.rotation((0, 0, 1), 0.05), (10.0, 0.0, 0.0), (0.02, -0.03, 0.01))
    move0 = TP.pose_about(TP.rotation((1, 1, 0), -0.04), (0.0, 0.0, 0.0), (-0.05, 0.02, 0.0))
    far1 = PQ.world(np.eye(3), (0.0, 25.0, 0.0))         # the bystander: the blob, moved but not clicked
    up5 = PQ.world(np.eye(3), (0.0, 0.0, 40.0))          # a body above the targets, out of the way
    poses = [move0, far1, EYE, EYE, move4, up5]
    eng = scene_after_click_one(E, poses)
    ref = twin(E, eng)
    third = twin(E, eng)
    # scene_apply_poses == scene_apply_pose per body, on pieces and poses (and a compound at the identity among them)
    third.scene_apply_poses([0, 4, 2])
    for c in (4, 2, 0):
        ref.scene_apply_pose(c)
    assert_same_scene(third, ref)
    want = np.asarray(poses, np.float32).copy(); want[[0, 4]] = EYE
    assert third.scene_poses().tobytes() == want.tobytes()
    before, moved = TS.snapshot(eng), TS.snapshot(third)
    table = eng.scene_compounds()
    for c in range(len(table) - 1):
        for p in range(int(table[c]), int(table[c + 1])):
            assert TS.same_solid(before[1][p][1], moved[1][p][1]) == (c not in (0, 4)), (c, p)
    third.close(); ref.close()
    # the click on posed targets, against the sequential route and the Python model of the poses
    ref = twin(E, eng)
    cube = TS.bodies(E)["cube"]
    cloud = TS.sphere_cloud(CLICK_ORIGIN, CLICK_RADIUS)
    for e in (eng, ref):
        place_click(e, cube, CLICK_ORIGIN, CLICK_RADIUS)
    seq, made = bodies_click(E, eng, ref, CLICK_TARGETS, (0, 8), True, cloud, CLICK_ORIGIN, CLICK_RADIUS)
    model = [p for c, p in enumerate(poses) if c not in CLICK_TARGETS] + [EYE] * len(made)      # erase, push_back; the others moved down
    got = eng.scene_poses()
    assert got.tobytes() == np.asarray(model, np.float32).tobytes()
    assert got[0].tobytes() == far1.tobytes() and got[2].tobytes() == up5.tobytes() and (got[3:] == EYE).all() and len(made) >= 3
    eng.close(); ref.close()
    # all-identity poses: scene_apply_poses does nothing at all, and a pending event stays committable
    eng = scene_after_click_one(E, [EYE, far1, EYE, EYE, EYE, EYE])
    place_click(eng, cube, CLICK_ORIGIN, CLICK_RADIUS)
    eng.scene_fracture_bodies(CLICK_TARGETS, 0, 8, flags=0)
    co, cp, _ = eng.event_regroup_bodies()
    snap = TS.snapshot(eng)
    eng.scene_apply_poses(CLICK_TARGETS)
    TS.assert_unchanged(eng, snap)
    n, first, n_new, _ = eng.scene_commit(co, cp)
    assert first == 3 and n_new >= 3 and eng.scene_poses()[0].tobytes() == far1.tobytes()
    # any other pose forgets the event, as scene_apply_pose does
    eng.scene_fracture_bodies([1, 0], 0, 8, flags=0)
    co, cp, _ = eng.event_regroup_bodies()
    eng.scene_apply_poses([2, 0])
    with pytest.raises(engine.SurtrError) as e:
        eng.scene_commit(co, cp)
    assert e.value.code == engine.E_STATE
    eng.close()


# ------------------------------------------------------------------ 6. errors
def run_errors(E):
    eng = scene_after_click_one(E, [EYE] * 5 + [PQ.world(np.eye(3), (0.0, 0.0, 40.0))])
    cube = TS.bodies(E)["cube"]
    place_click(eng, cube, CLICK_ORIGIN, CLICK_RADIUS)
    cloud = TS.sphere_cloud(CLICK_ORIGIN, CLICK_RADIUS)
    before, poses = TS.snapshot(eng), eng.scene_poses().tobytes()

    def refused(code, call):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == code, e.value
        TS.assert_unchanged(eng, before)
        assert eng.scene_poses().tobytes() == poses
    for bad in ([0, 2, 4], [4, 2, 2], [2, 2], [6, 2], [4, 2, 0, 0], [0xFFFFFFFF]):      # ascending, duplicate, out of range
        refused(engine.E_INVALID, lambda: eng.scene_fracture_bodies(bad, 0, 8, flags=0))
        refused(engine.E_INVALID, lambda: eng.scene_fracture_bodies_async(bad, 0, 8, flags=0))
    refused(engine.E_INVALID, lambda: eng.scene_fracture_bodies([], 0, 8, flags=0))      # n_targets == 0
    refused(engine.E_INVALID, lambda: eng.scene_fracture_bodies([4, 2], 0, 9, flags=0))
    refused(engine.E_INVALID, lambda: eng.scene_fracture_bodies([4, 2], 0, 8, outside=[0] * 5, flags=0))
    refused(engine.E_INVALID, lambda: eng.scene_outside([6], cloud, CLICK_ORIGIN, CLICK_RADIUS))
    refused(engine.E_INVALID, lambda: eng.scene_outside([], cloud, CLICK_ORIGIN, CLICK_RADIUS))
    refused(engine.E_INVALID, lambda: eng.scene_apply_poses([2, 6]))
    refused(engine.E_CAPACITY, lambda: eng.scene_outside([4, 2, 0], cloud, CLICK_ORIGIN, CLICK_RADIUS, capacity=6))      # seven pieces
    # the refused events changed nothing: no scene event is pending
    refused(engine.E_STATE, lambda: eng.scene_commit(np.array([0, 0], np.uint32), np.zeros(1, np.int32)))
    # a commit after scene_set_compounds, or after a transform, since the event
    for spoil in (lambda: eng.scene_set_compounds(before[0]) or eng.scene_set_poses(np.frombuffer(poses, np.float32).reshape(-1, 4, 4)),
                  lambda: eng.scene_transform_compound(1, [EYE])):
        eng.scene_fracture_bodies(CLICK_TARGETS, 0, 8, flags=0)
        co, cp, _ = eng.event_regroup_bodies()
        spoil()
        refused(engine.E_STATE, lambda: eng.scene_commit(co, cp))
    # compounds that do not cover the pieces exactly once
    eng.scene_fracture_bodies(CLICK_TARGETS, 0, 8, flags=0)
    co, cp, bo = eng.event_regroup_bodies()
    dup = cp.copy(); dup[1] = dup[0]
    refused(engine.E_INVALID, lambda: eng.scene_commit(co, dup))
    refused(engine.E_INVALID, lambda: eng.scene_commit(co[:-1], cp))
    # ... the good ones commit, once
    n, first, n_new, src = eng.scene_commit(co, cp)
    assert first == 3 and n_new >= 3
    before, poses = TS.snapshot(eng), eng.scene_poses().tobytes()
    refused(engine.E_STATE, lambda: eng.scene_commit(co, cp))
    eng.close()


def run_capacity(E):
    """A Convex of more than 4096 half-edges (the blob's Mesh taken as its Convex): SURTR_E_CAPACITY for a list that names it,
    nothing changed, and the context answers for the other body as before."""
    b = TS.bodies(E)
    eng = E.Engine(0)
    eng.upload_pieces([b["meshes"][0], b["meshes"][2]], [b["convexes"][0], b["meshes"][2]])
    eng.scene_set_compounds([0, 1, 2])
    assert np.asarray(eng.download_piece(1, 1)["nbr"]).shape[0] > 4096
    origin, radius = np.float32([2.0, 0.0, 0.0]), 1.5
    cloud = TS.sphere_cloud(origin, radius)
    before = TS.snapshot(eng)
    for bad in ([1], [1, 0], [0, 1]):
        with pytest.raises(engine.SurtrError) as e:
            eng.scene_outside(bad, cloud, origin, radius)
        assert e.value.code == engine.E_CAPACITY, e.value
        TS.assert_unchanged(eng, before)
    got = eng.scene_outside([0], cloud, origin, radius)
    assert list(got) == [int(engine.convex_out_of_sphere(eng.download_piece(0, 1), cloud, origin, radius))] == [0]
    eng.close()


# ------------------------------------------------------------------ CPU tier (emulation)
def test_device_mask_equals_the_host_mask(emul_engine):
    run_mask(emul_engine)


@pytest.mark.parametrize("partial", [True, False])
def test_bodies_click_equals_sequential_clicks(emul_engine, partial):
    print(run_click(emul_engine, partial))


def test_bind0_and_island_groups_stay_with_their_own_body(emul_engine):
    print(run_click_later_body(emul_engine))


def test_equal_cells_at_a_body_boundary(emul_engine):
    run_boundary(emul_engine)


def test_one_target_equals_the_one_body_event(emul_engine):
    run_one_target(emul_engine)


def test_apply_poses_and_the_click_on_posed_bodies(emul_engine):
    run_poses(emul_engine)


def test_errors_leave_table_poses_and_pieces_unchanged(emul_engine):
    run_errors(emul_engine)


def test_a_convex_too_large_for_the_mask_is_refused(emul_engine):
    run_capacity(emul_engine)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_scene_bodies as T
    case = sys.argv[1]
    if case == "mask":
        T.run_mask(engine, torch)
    elif case == "click_full":
        T.run_click(engine, partial=False)
    elif case == "async":
        T.run_async(engine, torch)
    elif case == "harness":
        T.check_harness(engine, %(root)r)
    else:
        getattr(T, "run_" + case)(engine)
    print("ok", case)
""")


def run_async(E, torch):
    """The _async event and scene_outside_dev on a stream of their own, with the lean arrangement of six events in flight."""
    st = torch.cuda.Stream()
    eng = scene_after_click_one(E)
    ref = twin(E, eng)
    cube = TS.bodies(E)["cube"]
    cloud = TS.sphere_cloud(CLICK_ORIGIN, CLICK_RADIUS)
    for e in (eng, ref):
        place_click(e, cube, CLICK_ORIGIN, CLICK_RADIUS)
    eng.set_stream(st.cuda_stream)
    eng.set_events_in_flight(6)
    with torch.cuda.stream(st):
        d_c = torch.from_numpy(cloud).cuda()
        d_o = torch.zeros(16, dtype=torch.uint8, device="cuda")
        st.synchronize()
        eng.scene_outside_dev(CLICK_TARGETS, cloud.shape[0], d_c.data_ptr(), CLICK_ORIGIN, CLICK_RADIUS, d_o.data_ptr(), d_o.numel())
        st.synchronize()
        assert d_o.cpu().numpy()[:7].tobytes() == host_mask(ref, CLICK_TARGETS, cloud, CLICK_ORIGIN, CLICK_RADIUS).tobytes()
        bodies_click(E, eng, ref, CLICK_TARGETS, (0, 8), True, cloud, CLICK_ORIGIN, CLICK_RADIUS, click_conditions(True), use_async=True)
    st.synchronize()
    eng.close(); ref.close()


def python_one_event_click(eng, o, d, r, n_cells):
    """OnMouseDownBodies(radial, oneEvent) through the Python calls, in float as the host layer computes it."""
    hit = eng.scene_raycast([list(o) + list(d) + [1000.0]])[0]
    assert hit["piece"] >= 0
    r32 = np.float32(r)
    impact = (hit["pos"] + np.asarray(d, np.float32) * np.float32(0.01)).astype(np.float32)
    mass = eng.scene_mass(set=1)
    body = eng.scene_overlap([list(impact) + [float(r32 / np.float32(2))]], body_mass=mass, min_mass=1e-4)[0]
    picked = sorted((int(c) for c in np.nonzero(body == 1)[0]), reverse=True)
    cloud = (TS.lattice_cloud() * r32 + impact).astype(np.float32)
    eng.scene_apply_poses(picked)
    eng.place_cells([r32 * np.float32(2)] * 3, impact)
    mask = eng.scene_outside(picked, cloud, impact, float(r32))
    eng.scene_fracture_bodies(picked, 0, n_cells, outside=mask if mask.any() else None, flags=0)
    co, cp, _ = eng.event_regroup_bodies(partial=True, sphere_points=cloud, origin=impact, radius=float(r32))
    eng.event_refit()
    n, first, n_new, _ = eng.scene_commit(co, cp)
    table = eng.scene_compounds()
    return dict(hit_piece=int(hit["piece"]), hit_compound=int(hit["compound"]), body_mask=[int(x) for x in body], compounds_hit=sorted(picked),
                compounds_made=list(range(first, first + n_new)), table=[int(x) for x in table], mass=[float(x) for x in eng.scene_mass(set=1)["mass"]])


def check_harness(E, root, exe=None):
    """surtr_harness --body-clicks ... --radial --one-event against the run without --one-event and against the Python calls."""
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    clicks = [([-10.0, 6.3, 0.2], [1.0, 0.0, 0.0]), ([0.3, 0.2, 10.0], [0.0, 0.0, -1.0])]
    arg = ";".join(",".join("%r" % x for x in o + d) for o, d in clicks)
    pose_arg = ";".join("%d:" % c + ",".join("%r" % float(x) for x in W.reshape(-1)) for c, W in ((1, TP.HARNESS_POSE), (3, TP.HARNESS_FAR)))
    cmd = [exe, "--mesh", "cube", "--cells", "8", "--scene-poses", pose_arg, "--body-clicks", arg, "--impact-radius", "4.0", "--radial"]
    runs = []
    for extra in ([], ["--one-event"]):
        p = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        runs.append([json.loads(x) for x in p.stdout.strip().splitlines() if x.startswith('{"body_click"')])
    assert len(runs[0]) == len(clicks) and runs[0] == runs[1], (runs[0], runs[1])
    sc = scenes.cube_scene(8)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, 8)
    n = eng.pieces_from_event()
    eng.scene_set_compounds(list(range(0, n, 2)) + [n])
    poses = np.tile(EYE, ((n + 1) // 2, 1, 1))
    poses[1], poses[3] = TP.HARNESS_POSE, TP.HARNESS_FAR
    eng.scene_set_poses(poses)
    for k, (o, d) in enumerate(clicks):
        want = dict(python_one_event_click(eng, o, d, 4.0, 8), body_click=k)
        line = dict(runs[1][k])
        got_poses = np.asarray(line.pop("poses"), np.float32).reshape(-1, 4, 4)
        assert line == want, (line, want)
        assert got_poses.tobytes() == eng.scene_poses().tobytes()
    assert len(want["compounds_hit"]) == 2
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["mask", "click", "click_full", "click_later_body", "boundary", "one_target", "poses", "errors", "capacity", "async"])
def test_gpu_scene_bodies(case):
    run_gpu_child(GPU_CHILD, case, 120)


@pytest.mark.gpu
def test_gpu_harness_body_clicks_one_event():
    run_gpu_child(GPU_CHILD, "harness", 150)
