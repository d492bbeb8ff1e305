"""Several impacts in one frame: place_cells_impacts (k_place_cells_impacts), scene_outside_impacts (k_scene_outside_impacts),
scene_fracture_impacts, event_regroup_impacts (k_rg_faces with a sphere per piece) and the one scene_commit after them.

THE REFERENCE IS THE EXISTING CODE.  A twin engine runs the impacts one after the other, in the order given, through the calls
that were there before: scene_apply_poses, place_cells, scene_outside, scene_fracture_bodies, event_regroup_bodies, event_refit,
scene_commit, the later impacts' compound numbers moved down by the commits before them.  Everything is compared without a tolerance:
the masks, the counts, the refitted event (fragment after fragment), frag_ids (cell modulo n_cells, the instance being the impact;
piece numbers translated to the scene before the frame), the compounds body by body, the composed src, every resident Mesh and
Convex, the table, the poses and scene_mass of both sets.

Scene: test_scene_bodies' (six compounds after click 1: the cube at the origin, the blob, a compound of five fragments of the cube at
x = 10 and three of one fragment each) with the 8-cell cube pattern.

The CPU tier runs on the emulation library (conftest's emul_engine); the GPU tier runs the same cases on the MI355X in child processes
under a time limit (helpers.run_gpu_child)."""
import json
import os
import subprocess
import textwrap

import numpy as np
import pytest

import test_pick_queries as PQ
import test_scene as TS
import test_scene_bodies as TB
import test_scene_poses as TP
from helpers import run_gpu_child
from surtr_amd import engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.eye(4, dtype=np.float32)
N_CELLS = 8


def impact(origin, radius, targets, n_cloud=64, scale=None, translate=None):
    """An impact: origin, radius, the placement of OnMouseDown unless given (the pattern scaled to the diameter, centred on the
    impact), a Fibonacci cloud of n_cloud points, and its targets (compound numbers of the scene before the frame)."""
    origin = np.asarray(origin, np.float32)
    return dict(origin=origin, radius=float(radius), targets=list(targets),
                scale=np.asarray([np.float32(radius) * np.float32(2)] * 3 if scale is None else scale, np.float32),
                translate=origin if translate is None else np.asarray(translate, np.float32),
                cloud=TS.sphere_cloud(origin, radius, n_cloud) if n_cloud else np.zeros((0, 3), np.float32))


# Two impacts with different radii and placements on targets that interleave in number: impact 1's compound 2 lies between impact
# 0's 4 and 0.  Impact 0 is test_scene_bodies' click sphere.  Its second sphere, (8, 1, 0) r 5.5, does not meet the conditions below on
# the CPU tier in either assignment: on compound 2 it masks no piece, and on {4, 0} no fragment moves to a bind 0 under it.  Impact 1
# is therefore (11, 0.5, 0.3) r 2, found on the CPU tier by a search over a grid of origins and radii on the sequential reference
# alone: it masks piece 0 of compound 2, which impact 0's sphere would not; under either sphere a fragment moves to its body's bind 0
# that the other sphere would leave; a body has island groups (all asserted on the reference in run_main / main_conditions).
MAIN = [impact((6.0, 0.0, 0.7), 4.0, [4, 0]), impact((11.0, 0.5, 0.3), 2.0, [2])]


# ------------------------------------------------------------------ the sequential reference
def regroup_kw(im, partial):
    return dict(partial=True, sphere_points=im["cloud"], origin=im["origin"], radius=im["radius"]) if partial else {}


def sequential_impacts(ref, cube, impacts, cells, partial, other_sphere=None):
    """The reference: today's calls, impact after impact.  -> per impact dict(mask, n_frag, n_pairs, ev, ids (cell, ORIGINAL resident
    piece), co, cp, bo, skipped (original piece numbers, ascending), moved (fragments in their body's bind 0, per body), and with
    other_sphere[i] the same set under that sphere), and origin_of per piece of the final scene."""
    table0 = [int(x) for x in ref.scene_compounds()]
    now = list(range(len(table0) - 1))                 # current number of every compound of the scene before the frame
    piece_orig = list(range(table0[-1]))               # original number of every current resident piece (None: made by the frame)
    origin_of = [("old", p) for p in range(table0[-1])]
    ref.upload_pattern(cube["face_off"], cube["v012"])
    out = []
    for i, im in enumerate(impacts):
        targets = [now[c] for c in im["targets"]]
        assert None not in targets
        ref.scene_apply_poses(targets)
        ref.place_cells(im["scale"], im["translate"])
        planes = ref.download_planes()
        table = [int(x) for x in ref.scene_compounds()]
        mask = ref.scene_outside(targets, im["cloud"], im["origin"], im["radius"]) if partial else None
        c = ref.scene_fracture_bodies(targets, cells[0], cells[1], outside=mask, flags=0)
        co, cp, bo = ref.event_regroup_bodies(**regroup_kw(im, partial))
        skipped = [piece_orig[p] for t in sorted(targets) for j, p in enumerate(range(table[t], table[t + 1]))
                   if partial and mask[sum(table[u + 1] - table[u] for u in targets[:targets.index(t)]) + j]]
        moved = moved_fragments(co, cp, bo, len(skipped))
        moved_other = None
        if other_sphere is not None and partial:
            o = other_sphere[i]
            co2, cp2, bo2 = ref.event_regroup_bodies(partial=True, sphere_points=o["cloud"], origin=o["origin"], radius=o["radius"])
            moved_other = moved_fragments(co2, cp2, bo2, len(skipped))
        ref.event_refit()
        ev = ref.download()
        ids = ev["frag_ids"].reshape(-1, 3).copy()
        ids[:, 1] = [piece_orig[p] for p in ids[:, 1]]
        n, first, n_new, src = ref.scene_commit(co, cp)
        origin_of = [origin_of[s] if s >= 0 else ("frag", i, -int(s) - 1) for s in src]
        piece_orig = [piece_orig[s] if s >= 0 else None for s in src]
        gone = sorted(targets)
        now = [None if (k is None or k in gone) else k - sum(1 for g in gone if g < k) for k in now]
        out.append(dict(mask=np.zeros(0, np.uint8) if mask is None else mask, n_frag=int(c.n_frag), n_pairs=int(c.n_pairs), ev=ev, ids=ids, co=co, cp=cp,
                        bo=bo, skipped=skipped, moved=moved, moved_other=moved_other, planes=planes))
    return out, origin_of


def moved_fragments(co, cp, bo, n_skip):
    """Per body: the fragments (numbered from 0) MergeOutOfImpact moved to the body's bind 0."""
    return [sorted(int(q) - n_skip for q in cp[co[bo[b]]:co[bo[b] + 1]] if int(q) >= n_skip) for b in range(len(bo) - 1)]


def body_compounds(s):
    """One impact of the reference, body by body, in the shape test_scene_bodies.island_groups reads (local piece numbers)."""
    return [[[int(q) for q in s["cp"][s["co"][i]:s["co"][i + 1]]] for i in range(int(s["bo"][b]), int(s["bo"][b + 1]))] for b in range(len(s["bo"]) - 1)]


def has_island_groups(s):
    """Some body of this impact has more compounds than its bind 0 and one per cell: HandleConvexIsland split a bind."""
    n_skip, cells = len(s["skipped"]), s["ids"][:, 0]
    for comps in body_compounds(s):
        per_cell = {}
        for k, members in enumerate(comps[1:]):
            if any(q < n_skip for q in members):
                return True                                  # split off bind 0
            for c in set(int(cells[q - n_skip]) for q in members):
                per_cell[c] = per_cell.get(c, 0) + 1
        if any(v > 1 for v in per_cell.values()):
            return True
    return False


# ------------------------------------------------------------------ the frame through the new calls, everything compared
def impacts_frame(E, eng, ref, impacts, cells=(0, N_CELLS), partial=True, conditions=None, use_async=False, other_sphere=None, place=True):
    cube = TS.bodies(E)["cube"]
    table0 = [int(x) for x in eng.scene_compounds()]
    seq, origin_of = sequential_impacts(ref, cube, impacts, cells, partial, other_sphere)
    if conditions is not None:
        conditions(seq)                                    # on the reference alone
    K = len(impacts)
    targets = [im["targets"] for im in impacts]
    flat = [t for ts in targets for t in ts]
    if place:
        eng.upload_pattern(cube["face_off"], cube["v012"])
    eng.scene_apply_poses(flat)
    eng.place_cells_impacts([im["scale"] for im in impacts], [im["translate"] for im in impacts])
    # every instance's planes are place_cells' for that scale and translate
    planes = eng.download_planes(impacts=True).reshape(K, -1, 4)
    for i in range(K):
        assert planes[i].tobytes() == seq[i]["planes"].tobytes(), ("planes", i)
    clouds, origins, radii = [im["cloud"] for im in impacts], [im["origin"] for im in impacts], [im["radius"] for im in impacts]
    mask = eng.scene_outside_impacts(targets, clouds, origins, radii) if partial else None
    if partial:
        assert mask.dtype == np.uint8 and mask.tobytes() == np.concatenate([s["mask"] for s in seq]).tobytes(), (mask, [s["mask"] for s in seq])
    if use_async:
        eng.scene_fracture_impacts_async(targets, cells[0], cells[1], outside=mask, flags=0)
        c = eng.event_counts()
    else:
        c = eng.scene_fracture_impacts(targets, cells[0], cells[1], outside=mask, flags=0)
    assert c.status == 0 and c.n_frag == sum(s["n_frag"] for s in seq) and c.n_pairs == sum(s["n_pairs"] for s in seq)
    frag_off = np.cumsum([0] + [s["n_frag"] for s in seq])
    kw = dict(partial=True, sphere_points=clouds, origins=origins, radii=radii) if partial else dict(n_impacts=K)
    co, cp, bo = eng.event_regroup_impacts(**kw)
    # ---- the compounds, body by body: the frame numbers the skipped pieces of all targets ascending, then all fragments
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
        for b, want in enumerate(body_compounds(s)):
            g = int(body0[i]) + b
            got = [[local(int(q)) for q in cp[co[k]:co[k + 1]]] for k in range(int(bo[g]), int(bo[g + 1]))]
            assert got == want, (i, b, got, want)
    eng.event_refit()
    # ---- the refitted event: fragment after fragment the sequential events', impact after impact
    ev = eng.download()
    ids = ev["frag_ids"].reshape(-1, 3)
    n_cells = N_CELLS
    for i, s in enumerate(seq):
        mine = ids[frag_off[i]:frag_off[i + 1]]
        assert (mine[:, 0] // n_cells == i).all() and list(mine[:, 0] % n_cells) == list(s["ids"][:, 0]), (i, mine[:, 0])
        assert list(mine[:, 1]) == list(s["ids"][:, 1]) and list(mine[:, 2]) == list(s["ids"][:, 2]), (i, mine, s["ids"])
    for key in TS.EVENT_KEYS:
        if key.endswith("_off"):
            assert list(np.diff(ev[key].astype(np.int64))) == [int(d) for s in seq for d in np.diff(s["ev"][key].astype(np.int64))], key
        else:
            assert np.asarray(ev[key]).tobytes() == b"".join(np.asarray(s["ev"][key]).tobytes() for s in seq), key
    # ---- one commit
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
    return seq, list(range(first, first + n_new))


def fresh(E, poses=None):
    eng = TB.scene_after_click_one(E, poses)
    return eng, TB.twin(E, eng)


# ------------------------------------------------------------------ 1. two impacts, interleaving targets
def swap_targets(impacts):
    """The other impact's sphere for every impact of a pair."""
    return [impacts[1], impacts[0]]


def main_conditions(seq):
    assert all(s["n_frag"] > 0 for s in seq), [s["n_frag"] for s in seq]                      # both impacts produce fragments
    assert any(set(a) - set(b) for s in seq for a, b in zip(s["moved"], s["moved_other"])), \
        [(s["moved"], s["moved_other"]) for s in seq]                                         # a move to bind 0 only the own sphere makes
    assert any(has_island_groups(s) for s in seq)                                             # one body has island groups


def run_main(E, use_async=False):
    eng, ref = fresh(E)
    table = [int(x) for x in eng.scene_compounds()]
    assert table == [0, 1, 2, 7, 8, 9, 10]
    a, b = MAIN
    assert a["radius"] != b["radius"] and a["scale"].tobytes() != b["scale"].tobytes() and b["targets"][0] in range(a["targets"][1] + 1, a["targets"][0])
    # a piece of the multi-piece target that its own impact's sphere masks out and the other's would not: on the reference alone,
    # before anything runs (scene_outside changes nothing)
    own = ref.scene_outside(b["targets"], b["cloud"], b["origin"], b["radius"])
    other = ref.scene_outside(b["targets"], a["cloud"], a["origin"], a["radius"])
    assert len(own) > 1 and any(o == 1 and x == 0 for o, x in zip(own, other)), (own, other)
    seq, made = impacts_frame(E, eng, ref, MAIN, conditions=main_conditions, use_async=use_async, other_sphere=swap_targets(MAIN))
    eng.close(); ref.close()
    return [s["n_frag"] for s in seq], len(made)


# ------------------------------------------------------------------ 2. a cloud that straddles a wave; small and large Convex
def run_clouds(E):
    eng, ref = fresh(E)
    halves = [int(np.asarray(eng.download_piece(p, 1)["nbr"]).shape[0]) for p in (0, 1)]
    assert halves[0] == 24 and halves[1] > 64, halves      # the cube; the blob's ACH Convex
    # no cloud at all on the cube, 100 points (one wave and a part of the next) inside the blob, where no vertex is near and a
    # cloud point decides; then the same with the clouds exchanged
    for n0, n1 in ((0, 100), (100, 0)):
        frame = [impact((0.4, 0.2, 0.1), 0.8, [0], n_cloud=n0), impact((0.0, 300.0, 0.0), 1.0, [1], n_cloud=n1)]
        got = eng.scene_outside_impacts([im["targets"] for im in frame], [im["cloud"] for im in frame], [im["origin"] for im in frame], [im["radius"] for im in frame])
        want = np.concatenate([ref.scene_outside(im["targets"], im["cloud"], im["origin"], im["radius"]) for im in frame])
        assert got.tobytes() == want.tobytes(), (n0, n1, got, want)
    frame = [impact((0.4, 0.2, 0.1), 0.8, [0], n_cloud=0), impact((0.0, 300.0, 0.0), 1.0, [1], n_cloud=100)]
    seq, made = impacts_frame(E, eng, ref, frame)
    eng.close(); ref.close()


# ------------------------------------------------------------------ 3. an impact that touches nothing, between two that do
def run_miss(E):
    eng, ref = fresh(E)
    frame = [impact((6.0, 0.0, 0.7), 4.0, [4]), impact((30.0, 40.0, 0.0), 1.0, [2]), impact((0.4, 0.2, 0.1), 0.8, [0])]

    def conditions(seq):
        assert seq[0]["n_frag"] > 0 and seq[2]["n_frag"] > 0 and seq[1]["n_frag"] == 0
        assert seq[1]["mask"].all() and len(seq[1]["mask"]) == 5 and len(seq[1]["co"]) == 2      # the whole body in its bind 0
    seq, made = impacts_frame(E, eng, ref, frame, conditions=conditions)
    eng.close(); ref.close()


# ------------------------------------------------------------------ 4. one impact == scene_fracture_bodies / event_regroup_bodies
def run_one_impact(E):
    cube = TS.bodies(E)["cube"]
    im = impact(TB.CLICK_ORIGIN, TB.CLICK_RADIUS, TB.CLICK_TARGETS)
    eng, ref = fresh(E)
    for e in (eng, ref):
        TB.place_click(e, cube, im["origin"], im["radius"])
    eng.place_cells_impacts([im["scale"]], [im["translate"]])
    assert eng.download_planes(impacts=True).tobytes() == ref.download_planes().tobytes() == eng.download_planes().tobytes()
    mask = ref.scene_outside(im["targets"], im["cloud"], im["origin"], im["radius"])
    assert eng.scene_outside_impacts([im["targets"]], [im["cloud"]], [im["origin"]], [im["radius"]]).tobytes() == mask.tobytes() and mask.any()
    ca = eng.scene_fracture_impacts([im["targets"]], 0, N_CELLS, outside=mask, flags=0)
    cb = ref.scene_fracture_bodies(im["targets"], 0, N_CELLS, outside=mask, flags=0)
    assert bytes(ca) == bytes(cb)
    kw = dict(partial=True, sphere_points=im["cloud"], origin=im["origin"], radius=im["radius"])
    co, cp, bo = eng.event_regroup_impacts(partial=True, sphere_points=[im["cloud"]], origins=[im["origin"]], radii=[im["radius"]])
    ro, rp, rb = ref.event_regroup_bodies(**kw)
    co1, cp1, bo1 = eng.event_regroup_bodies(**kw)      # the single-sphere calls after an impacts event: unchanged in result
    co2, cp2 = eng.event_regroup(**kw)
    assert list(co) == list(ro) == list(co1) == list(co2) and list(cp) == list(rp) == list(cp1) == list(cp2) and list(bo) == list(rb) == list(bo1)
    eng.event_refit(); ref.event_refit()
    ea, eb = eng.download(), ref.download()
    for k in TS.EVENT_KEYS + ("frag_ids",):
        assert np.asarray(ea[k]).tobytes() == np.asarray(eb[k]).tobytes(), k
    a, b = eng.scene_commit(co, cp), ref.scene_commit(ro, rp)
    assert a[:3] == b[:3] and list(a[3]) == list(b[3])
    TB.assert_same_scene(eng, ref)
    eng.close(); ref.close()


# ------------------------------------------------------------------ 5. posed targets
def run_poses(E):
    move4 = TP.pose_about(TP.rotation((0, 0, 1), 0.05), (10.0, 0.0, 0.0), (0.02, -0.03, 0.01))
    move0 = TP.pose_about(TP.rotation((1, 1, 0), -0.04), (0.0, 0.0, 0.0), (-0.05, 0.02, 0.0))
    far1 = PQ.world(np.eye(3), (0.0, 25.0, 0.0))         # the bystander: the blob, moved but not hit
    up5 = PQ.world(np.eye(3), (0.0, 0.0, 40.0))          # a body above the targets, out of the way
    poses = [move0, far1, EYE, EYE, move4, up5]
    eng, ref = fresh(E, poses)
    seq, made = impacts_frame(E, eng, ref, MAIN)
    model = [p for c, p in enumerate(poses) if c not in (4, 2, 0)] + [EYE] * len(made)      # erase, push_back; the others moved down
    got = eng.scene_poses()
    assert got.tobytes() == np.asarray(model, np.float32).tobytes()
    assert got[0].tobytes() == far1.tobytes() and got[2].tobytes() == up5.tobytes() and (got[3:] == EYE).all() and len(made) >= 3
    eng.close(); ref.close()


# ------------------------------------------------------------------ 6. errors
def run_errors(E):
    eng = TB.scene_after_click_one(E, [EYE] * 5 + [PQ.world(np.eye(3), (0.0, 0.0, 40.0))])
    cube = TS.bodies(E)["cube"]
    a, b = MAIN
    clouds, origins, radii = [a["cloud"], b["cloud"]], [a["origin"], b["origin"]], [a["radius"], b["radius"]]
    eng.upload_pattern(cube["face_off"], cube["v012"])
    before, poses = TS.snapshot(eng), eng.scene_poses().tobytes()

    def refused(code, call):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == code, e.value
        TS.assert_unchanged(eng, before)
        assert eng.scene_poses().tobytes() == poses
    # an event call without an impacts placement (a plain placement is none), or with another K than was placed
    TB.place_click(eng, cube, a["origin"], a["radius"])
    refused(engine.E_STATE, lambda: eng.scene_fracture_impacts([[4, 0], [2]], 0, N_CELLS, flags=0))
    refused(engine.E_INVALID, lambda: eng.place_cells_impacts(np.zeros((0, 3)), np.zeros((0, 3))))
    eng.place_cells_impacts([a["scale"], b["scale"]], [a["translate"], b["translate"]])
    for call in (eng.scene_fracture_impacts, eng.scene_fracture_impacts_async):
        refused(engine.E_STATE, lambda: call([[4, 2, 0]], 0, N_CELLS, flags=0))
        refused(engine.E_STATE, lambda: call([[4], [2], [0]], 0, N_CELLS, flags=0))
        refused(engine.E_INVALID, lambda: call([], 0, N_CELLS, flags=0))                              # K = 0
        for bad in ([[4, 0], []], [[], [2]],                                                      # an impact without targets
                    [[4, 0], [6]], [[0xFFFFFFFF], [2]],                                           # out of range
                    [[4, 4], [2]], [[4, 0], [0]], [[2], [4, 2]],                                  # twice: inside one impact, under two
                    [[0, 4], [2]], [[2], [0, 4]]):                                                # not strictly descending inside an impact
            refused(engine.E_INVALID, lambda: call(bad, 0, N_CELLS, flags=0))
        refused(engine.E_INVALID, lambda: call([[4, 0], [2]], 0, N_CELLS + 1, flags=0))
        refused(engine.E_INVALID, lambda: call([[4, 0], [2]], 0, N_CELLS, outside=[0] * 5, flags=0))
    for bad in ([], [[4, 0], []], [[4, 0], [6]], [[4, 4], [2]], [[4, 0], [0]], [[0, 4], [2]]):
        refused(engine.E_INVALID, lambda: eng.scene_outside_impacts(bad, clouds[:len(bad)], origins[:len(bad)], radii[:len(bad)]))
    refused(engine.E_CAPACITY, lambda: eng.scene_outside_impacts([[4, 0], [2]], clouds, origins, radii, capacity=6))      # seven pieces
    # the refused events changed nothing: no scene event is pending, and there is no impacts event to regroup
    refused(engine.E_STATE, lambda: eng.scene_commit(np.array([0, 0], np.uint32), np.zeros(1, np.int32)))
    refused(engine.E_STATE, lambda: eng.event_regroup_impacts(partial=True, sphere_points=clouds, origins=origins, radii=radii))
    # a current event stays as it was through a refused call: it still regroups and commits
    eng.scene_fracture_impacts([[4, 0], [2]], 0, N_CELLS, flags=0)
    co, cp, bo = eng.event_regroup_impacts(n_impacts=2)
    refused(engine.E_INVALID, lambda: eng.scene_fracture_impacts([[4, 4], [2]], 0, N_CELLS, flags=0))
    refused(engine.E_STATE, lambda: eng.event_regroup_impacts(n_impacts=3))
    refused(engine.E_STATE, lambda: eng.event_regroup_impacts(partial=True, sphere_points=clouds[:1], origins=origins[:1], radii=radii[:1]))
    co1, cp1, bo1 = eng.event_regroup_impacts(n_impacts=2)
    assert list(co1) == list(co) and list(cp1) == list(cp) and list(bo1) == list(bo)
    eng.event_refit()
    n, first, n_new, src = eng.scene_commit(co, cp)
    assert first == 3 and n_new >= 3
    before, poses = TS.snapshot(eng), eng.scene_poses().tobytes()
    refused(engine.E_STATE, lambda: eng.scene_commit(co, cp))
    # a bodies event is no impacts event
    TB.place_click(eng, cube, a["origin"], a["radius"])
    eng.scene_fracture_bodies([1, 0], 0, N_CELLS, flags=0)
    refused(engine.E_STATE, lambda: eng.event_regroup_impacts(n_impacts=2))
    eng.close()


# ------------------------------------------------------------------ 7. a plain click after an impacts event
def run_plain_after(E):
    """place_cells + scene_fracture_bodies after an impacts frame give what they give on a fresh twin of that scene."""
    eng, ref = fresh(E)
    impacts_frame(E, eng, ref, MAIN)
    ref.close()
    ref = TB.twin(E, eng)
    cube = TS.bodies(E)["cube"]
    origin, radius = np.float32([9.0, 0.5, 0.3]), 3.0
    cloud = TS.sphere_cloud(origin, radius)
    ref.upload_pattern(cube["face_off"], cube["v012"])
    for e in (eng, ref):      # (eng keeps the pattern and the instances of the frame: only the plain placement is made)
        e.place_cells([np.float32(radius) * np.float32(2)] * 3, origin)
    assert eng.download_planes().tobytes() == ref.download_planes().tobytes()
    table = [int(x) for x in eng.scene_compounds()]
    hit = [c for c in range(len(table) - 2, -1, -1) if not eng.scene_outside([c], cloud, origin, radius).all()][:3]
    assert len(hit) >= 2, hit
    out = []
    for e in (eng, ref):
        mask = e.scene_outside(hit, cloud, origin, radius)
        c = e.scene_fracture_bodies(hit, 0, N_CELLS, outside=mask, flags=0)
        co, cp, bo = e.event_regroup_bodies(partial=True, sphere_points=cloud, origin=origin, radius=radius)
        e.event_refit()
        ev = e.download()
        out.append((mask.tobytes(), bytes(c), list(co), list(cp), list(bo), [np.asarray(ev[k]).tobytes() for k in TS.EVENT_KEYS + ("frag_ids",)],
                    [list(x) if hasattr(x, "__len__") else x for x in e.scene_commit(co, cp)]))
    assert out[0] == out[1] and out[0][1] != bytes(engine.Counts())
    TB.assert_same_scene(eng, ref)
    eng.close(); ref.close()


def run_async(E):
    return run_main(E, use_async=True)


def run_full(E):
    """Without a sphere: no mask, no move to bind 0 (event_regroup_impacts with partial=False reads no sphere)."""
    eng, ref = fresh(E)
    seq, made = impacts_frame(E, eng, ref, MAIN, partial=False)
    assert all(s["n_frag"] > 0 for s in seq)
    eng.close(); ref.close()


# ------------------------------------------------------------------ CPU tier (emulation)
def test_two_impacts_on_interleaving_targets_equal_sequential_impacts(emul_engine):
    print(run_main(emul_engine))


def test_two_impacts_without_spheres(emul_engine):
    run_full(emul_engine)


def test_clouds_of_0_and_100_points_on_a_small_and_a_large_convex(emul_engine):
    run_clouds(emul_engine)


def test_an_impact_that_touches_nothing_between_two_that_break(emul_engine):
    run_miss(emul_engine)


def test_one_impact_equals_the_bodies_event(emul_engine):
    run_one_impact(emul_engine)


def test_impacts_on_posed_targets(emul_engine):
    run_poses(emul_engine)


def test_errors_leave_scene_table_poses_and_event_unchanged(emul_engine):
    run_errors(emul_engine)


def test_a_plain_click_after_an_impacts_event(emul_engine):
    run_plain_after(emul_engine)


def test_async_event_then_event_counts(emul_engine):
    print(run_async(emul_engine))


def test_outside_impacts_dev_on_the_emulation(emul_engine):
    """The _dev form on the emulation, whose "device" memory is the host's (CPU tier only: on the GPU see run_dev)."""
    eng, ref = fresh(emul_engine)
    a, b = MAIN
    want = np.concatenate([ref.scene_outside(im["targets"], im["cloud"], im["origin"], im["radius"]) for im in MAIN])
    d_c = np.ascontiguousarray(np.concatenate([a["cloud"], b["cloud"]]))
    d_o = np.full(len(want) + 3, 7, np.uint8)
    args = ([a["targets"], b["targets"]], [0, len(a["cloud"]), len(a["cloud"]) + len(b["cloud"])], d_c.ctypes.data, [a["origin"], b["origin"]], [a["radius"], b["radius"]])
    eng.scene_outside_impacts_dev(*args, d_o.ctypes.data, len(want))
    assert d_o[:len(want)].tobytes() == want.tobytes() and (d_o[len(want):] == 7).all()
    with pytest.raises(engine.SurtrError) as e:
        eng.scene_outside_impacts_dev(*args, d_o.ctypes.data, len(want) - 1)
    assert e.value.code == engine.E_CAPACITY and (d_o[len(want):] == 7).all()
    eng.close(); ref.close()


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_scene_impacts as T
    case = sys.argv[1]
    if case == "dev":
        T.run_dev(engine, torch)
    else:
        getattr(T, "run_" + case)(engine)
    print("ok", case)
""")


def run_dev(E, torch):
    """scene_outside_impacts_dev and the _async event on a stream of their own."""
    st = torch.cuda.Stream()
    eng, ref = fresh(E)
    a, b = MAIN
    want = np.concatenate([ref.scene_outside(im["targets"], im["cloud"], im["origin"], im["radius"]) for im in MAIN])
    eng.set_stream(st.cuda_stream)
    with torch.cuda.stream(st):
        d_c = torch.from_numpy(np.concatenate([a["cloud"], b["cloud"]])).cuda()
        d_o = torch.full((len(want) + 3,), 7, dtype=torch.uint8, device="cuda")
        st.synchronize()
        args = ([a["targets"], b["targets"]], [0, len(a["cloud"]), len(a["cloud"]) + len(b["cloud"])], d_c.data_ptr(), [a["origin"], b["origin"]], [a["radius"], b["radius"]])
        eng.scene_outside_impacts_dev(*args, d_o.data_ptr(), len(want))
        st.synchronize()
        back = d_o.cpu().numpy()
        assert back[:len(want)].tobytes() == want.tobytes() and (back[len(want):] == 7).all()
        with pytest.raises(engine.SurtrError) as e:
            eng.scene_outside_impacts_dev(*args, d_o.data_ptr(), len(want) - 1)
        assert e.value.code == engine.E_CAPACITY
        impacts_frame(E, eng, ref, MAIN, conditions=main_conditions, use_async=True, other_sphere=swap_targets(MAIN))
    st.synchronize()
    eng.close(); ref.close()


def run_harness(E, exe=None):
    """surtr_harness --impacts ... --one-event against the same line without --one-event (the loop of existing routines), text for
    text.  The scene is --body-clicks' (four bodies of two pieces, body 1 posed, body 3 far away).  The first sphere reaches the
    posed body 1 alone, the second bodies 0 and 2 (so that impact 0's target lies between impact 1's), the third body 2 only, which
    the second has taken: it is dropped (found with scene_overlap on the CPU tier)."""
    exe = exe or os.path.join(ROOT, "surtr_amd", "host", "surtr_harness")
    pose_arg = ";".join("%d:" % c + ",".join("%r" % float(x) for x in W.reshape(-1)) for c, W in ((1, TP.HARNESS_POSE), (3, TP.HARNESS_FAR)))
    cmd = [exe, "--mesh", "cube", "--cells", "8", "--scene-poses", pose_arg, "--impacts", "-1.0,6.3,0.2,5.0;0.3,0.2,3.2,4.0;-2.5,2.5,0.0,3.0"]
    runs = []
    for extra in ([], ["--one-event"]):
        p = subprocess.run(cmd + extra, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        runs.append([x for x in p.stdout.strip().splitlines() if x.startswith('{"impacts"')])
    assert len(runs[0]) == 1 and runs[0] == runs[1], (runs[0], runs[1])
    line = json.loads(runs[1][0])
    assert line["impacts"] == 2 and line["compounds_hit"] == [[1], [0, 2]] and len(line["compounds_made"]) >= 3, line
    poses = np.asarray(line["poses"], np.float32).reshape(-1, 4, 4)
    assert poses[0].tobytes() == TP.HARNESS_FAR.tobytes() and (poses[1:] == EYE).all()      # the bystander kept its pose, and moved down


@pytest.mark.gpu
def test_gpu_harness_impacts_one_event():
    run_gpu_child(GPU_CHILD, "harness", 150)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["main", "full", "clouds", "miss", "one_impact", "poses", "errors", "plain_after", "async", "dev"])
def test_gpu_scene_impacts(case):
    run_gpu_child(GPU_CHILD, case, 120)
