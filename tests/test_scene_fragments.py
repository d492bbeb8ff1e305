"""Resident bodies as device fragments for InitCompound: scene_fragments (surtr_scene_fragments, k_frags_from_pieces in scene_dev.hip).

THE REFERENCE NEVER RUNS THE NEW CALL.  A second engine is given download_piece of exactly those pieces through load_fragments (host),
then event_triangulate(render_convex), then download().  Every array of the download is compared bit for bit and without a tolerance:
offsets, positions, rings, vnc, idx_off, idx, frag_status; frag_ids is checked against (compound, resident piece, 0).  With
render_convex the reference is given the Convex in both slots.

Scene: test_scene.three_bodies, then its click 1 (table [0, 1, 2, 7, 8, 9, 10]): an 8-vertex cube, a piece larger than a workgroup
whose Convex has more than 64 half-edges (the blob, 2 562 vertices), a compound of five pieces, and fragments with caps.

SURTR_E_CAPACITY "for more fragments than cap_frags" cannot be provoked: the fragment table is grown with the arena to four times the
fragments asked for plus 1 024, so the check only trips beyond 2^31 - 1 pieces.  The other errors are all exercised (run_errors).

The CPU tier runs on the emulation library (conftest's emul_engine); the GPU tier runs the same cases on the MI355X in child processes
under a time limit (helpers.run_gpu_child)."""
import ctypes
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
ARRAYS = ("mesh_vert_off", "mesh_pos", "mesh_nbr_off", "mesh_nbr", "conv_vert_off", "conv_pos", "conv_nbr_off", "conv_nbr", "vnc", "idx_off", "idx",
          "frag_status")
SOLID_ARRAYS = ARRAYS[:8]
TABLE = [0, 1, 2, 7, 8, 9, 10]
EYE = np.eye(4, dtype=np.float32)


# ------------------------------------------------------------------ helpers
def scene_after_click_one(E):
    eng, world = TS.three_bodies(E)
    TS.click_one(E, eng, world)
    assert list(eng.scene_compounds()) == TABLE
    return eng, world


def pieces_of(table, compounds):
    """-> [(compound, resident piece), ...] in list order, and inside a compound in piece order."""
    return [(int(c), p) for c in compounds for p in range(int(table[c]), int(table[c + 1]))]


def reference(E, eng, ids, render_convex=False, triangulate=True, keep=False):
    """The reference: download_piece of exactly those pieces -> load_fragments (host) -> event_triangulate -> download, on an engine of
    its own.  -> the download (and the engine when keep)."""
    meshes = [eng.download_piece(p, 1 if render_convex else 0) for _, p in ids]
    convs = [eng.download_piece(p, 1) for _, p in ids]
    ref = E.Engine(0)
    ref.load_fragments(meshes, convs)
    if triangulate:
        ref.event_triangulate(render_convex)
    out = ref.download()
    if keep:
        return out, ref
    ref.close()
    return out


def assert_same_event(got, want, ids, arrays=ARRAYS):
    for k in arrays:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), k
    assert got["frag_ids"].reshape(-1, 3).tolist() == [[c, p, 0] for c, p in ids]


def check_call(E, eng, compounds, render_convex=False):
    """scene_fragments(compounds) against the reference -> (the download, the pieces)."""
    table = eng.scene_compounds()
    ids = pieces_of(table, range(len(table) - 1) if compounds is None else compounds)
    want = reference(E, eng, ids, render_convex)
    c = eng.scene_fragments(compounds, render_convex=render_convex)
    got = eng.download()
    assert c.status == 0 and c.n_frag == len(ids) == c.n_pairs and c.n_idx == want["idx"].shape[0] and c.n_idx > 0
    assert_same_event(got, want, ids)
    return got, ids


# ------------------------------------------------------------------ 1-5: what comes out
def run_all_and_list(E):
    """Cases 1, 2, 5: every compound; the list [5, 2, 0] in the order given; flags = 0 and a triangulation afterwards."""
    eng, _ = scene_after_click_one(E)
    sizes = [eng.download_piece(p, 0)["pos"].shape[0] for p in range(TABLE[-1])]
    halves = [eng.download_piece(p, 1)["nbr"].shape[0] for p in range(TABLE[-1])]
    assert sizes[0] == 8 and sizes[1] == 2562 and halves[1] > 64        # the cube; the blob: larger than a workgroup, beyond k_faces' LDS staging
    all1, ids = check_call(E, eng, None)
    assert [c for c, _ in ids] == [0, 1, 2, 2, 2, 2, 2, 3, 4, 5] and [p for _, p in ids] == list(range(10))
    got, ids = check_call(E, eng, [5, 2, 0])
    assert [p for _, p in ids] == [9, 2, 3, 4, 5, 6, 0]
    # flags = 0: the same solids, no triangles; event_triangulate then gives the bytes of the call with EVT_RENDER
    c = eng.scene_fragments(None, flags=0)
    bare = eng.download()
    assert c.n_idx == 0 and c.n_frag == 10 and bare["idx"].shape[0] == 0 and not bare["idx_off"].any()
    assert_same_event(bare, all1, pieces_of(TABLE, range(6)), SOLID_ARRAYS + ("frag_status",))
    eng.event_triangulate()
    assert_same_event(eng.download(), all1, pieces_of(TABLE, range(6)))
    eng.close()


def run_render_convex(E):
    """Cases 3, 4: render_convex on all (the fan; the Mesh slot holds the Convex), and one piece of each kind against
    Engine.triangulate of the downloaded piece, for both settings."""
    eng, _ = scene_after_click_one(E)
    solo = E.Engine(0)
    for rc in (True, False):
        got, ids = check_call(E, eng, None, render_convex=rc)
        if rc:
            for k in ("vert_off", "pos", "nbr_off", "nbr"):
                assert got["mesh_" + k].tobytes() == got["conv_" + k].tobytes(), k
        for f in (0, 1, 4):        # the cube, the blob, a fragment of click 1 with a cap
            piece = eng.download_piece(ids[f][1], 1 if rc else 0)
            vnc, idx = solo.triangulate(piece, is_convex=rc)
            a, b = int(got["mesh_vert_off"][f]), int(got["mesh_vert_off"][f + 1])
            i0, i1 = int(got["idx_off"][f]), int(got["idx_off"][f + 1])
            assert got["vnc"][a:b].tobytes() == vnc.tobytes() and got["idx"][i0:i1].tobytes() == idx.tobytes(), (rc, f)
            if rc:      # the fan (Src/Poly.cpp:696-706): a face of k corners gives k - 2 triangles, H - 2 F = 2 V - 4 in all by V - H / 2 + F = 2
                assert i1 - i0 == 3 * (2 * (b - a) - 4), (f, i1 - i0)
    solo.close(); eng.close()


# ------------------------------------------------------------------ 6: after a second commit
def run_after_commit(E):
    eng, world = scene_after_click_one(E)
    n, first, n_new, src, _ = TS.click_two(E, eng, world, 2)
    made = list(range(first, first + n_new))
    got, ids = check_call(E, eng, made)
    assert len(ids) >= 2 and n > 64
    resident = np.concatenate([eng.download_piece(p, 0)["pos"] for _, p in ids])
    assert got["vnc"][:, :3].tobytes() == resident.tobytes()
    eng.close()


# ------------------------------------------------------------------ 7: poses
def run_poses(E):
    eng, _ = scene_after_click_one(E)
    eng.scene_fragments(None)
    plain = eng.download()
    move = TP.pose_about(TP.rotation((0, 0, 1), 0.05), (10.0, 0.0, 0.0), (0.02, -0.03, 0.01))
    eng.scene_set_poses([EYE, PQ.world(np.eye(3), (0.0, 25.0, 0.0)), move, EYE, EYE, EYE])
    eng.scene_fragments(None)
    assert_same_event(eng.download(), plain, pieces_of(TABLE, range(6)))        # the resident frame: a pose changes nothing
    eng.scene_apply_pose(2)
    got, ids = check_call(E, eng, None)                                            # the reference reads the baked pieces
    a, b = int(got["mesh_vert_off"][2]), int(got["mesh_vert_off"][7])
    assert got["mesh_pos"][:a].tobytes() == plain["mesh_pos"][:a].tobytes() and got["mesh_pos"][b:].tobytes() == plain["mesh_pos"][b:].tobytes()
    assert got["mesh_pos"][a:b].tobytes() != plain["mesh_pos"][a:b].tobytes()
    eng.close()


# ------------------------------------------------------------------ 8: refit and mass of the presented fragments
def run_refit_mass(E):
    eng, _ = scene_after_click_one(E)
    ids = pieces_of(TABLE, [2, 0, 1])
    want, ref = reference(E, eng, ids, keep=True)
    eng.scene_fragments([2, 0, 1])
    for e in (eng, ref):
        e.event_refit()
    assert eng.event_mass(set=1).tobytes() == ref.event_mass(set=1).tobytes()
    assert eng.event_mass(set=0).tobytes() == ref.event_mass(set=0).tobytes()
    assert_same_event(eng.download(), ref.download(), ids)
    ref.close(); eng.close()


# ------------------------------------------------------------------ 9, 10: the scene is untouched; state
def run_untouched_and_state(E):
    eng, _ = scene_after_click_one(E)
    eng.scene_set_poses([EYE, PQ.world(np.eye(3), (0.0, 25.0, 0.0)), EYE, EYE, EYE, EYE])
    ray = [[0.3, 0.2, 40.0, 0.0, 0.0, -1.0, 1000.0], [0.0, 325.0, 200.0, 0.0, 0.0, -1.0, 1000.0]]
    before, poses, hit = TS.snapshot(eng), eng.scene_poses().tobytes(), eng.scene_raycast(ray).tobytes()
    eng.scene_fragments(None)
    eng.scene_fragments([3, 1], render_convex=True)
    TS.assert_unchanged(eng, before)
    assert eng.scene_poses().tobytes() == poses and eng.scene_raycast(ray).tobytes() == hit
    # a pending scene event is gone after the call: its commit is SURTR_E_STATE and changes nothing
    cube = TS.bodies(E)["cube"]
    eng.upload_pattern(cube["face_off"], cube["v012"])
    eng.place_cells(cube["scale"], cube["translate"])
    eng.scene_fracture_event(0, 0, 8, flags=0)
    co, cp = eng.event_regroup()
    eng.scene_fragments([0])
    with pytest.raises(engine.SurtrError) as e:
        eng.scene_commit(co, cp)
    assert e.value.code == engine.E_STATE
    TS.assert_unchanged(eng, before)
    assert eng.scene_poses().tobytes() == poses
    eng.close()
    # the arena is left sound: the fixture's event right after the call
    g = np.load(os.path.join(GOLDEN, "cube8.npz"))
    b = TS.bodies(E)
    eng = E.Engine(0)
    eng.upload_pieces(b["meshes"][:2], b["convexes"][:2])
    eng.upload_planes(g["face_off"], g["planes"])
    eng.scene_fragments(None)
    c = eng.fracture_event(0, 8, outside=[0, 1], flags=3)
    assert c.n_pairs == 16
    ev = eng.download()
    for k in ("mesh_vert_off", "mesh_pos", "mesh_nbr_off", "mesh_nbr", "conv_vert_off", "conv_pos", "conv_nbr_off", "conv_nbr", "idx_off", "idx"):
        assert np.array_equal(ev[k].reshape(-1), g["out_" + k].reshape(-1)), k
    assert np.array_equal(ev["frag_ids"], g["out_frag_ids"].reshape(-1, 3))
    eng.close()


# ------------------------------------------------------------------ 11: a piece the face walk flags
def run_flagged(E):
    d = np.load(os.path.join(GOLDEN, "nonterminating_faces_fragment.npz"))
    # the solid whose faces cannot be extracted: the fragment that a render event over the fixture's piece flags
    setup = E.Engine(0)
    setup.upload_pieces([{"pos": d["mesh_pos"], "off": d["mesh_off"], "nbr": d["mesh_nbr"]}], [{"pos": d["conv_pos"], "off": d["conv_off"], "nbr": d["conv_nbr"]}])
    setup.upload_planes(d["fo"].astype(np.uint32), d["planes"])
    setup.fracture_event(0, len(d["fo"]) - 1, flags=3)
    ev = setup.download()
    setup.close()
    bad = [int(f) for f in np.nonzero(ev["frag_status"])[0]]
    assert len(bad) == 1
    fm, fc = scenes.fragments_as_pieces(ev)
    b = TS.bodies(E)
    eng = E.Engine(0)
    eng.upload_pieces([b["meshes"][0], fm[bad[0]]], [b["convexes"][0], fc[bad[0]]])
    eng.scene_set_compounds([0, 1, 2])
    ids = pieces_of([0, 1, 2], [0, 1])
    want = reference(E, eng, ids)
    assert want["frag_status"][0] == 0 and want["frag_status"][1] != 0          # the reference flags it, and only it
    c = eng.scene_fragments(None)
    got = eng.download()
    assert c.n_failed == 1 and c.status == 0
    assert_same_event(got, want, ids)
    assert got["idx_off"].tolist() == [0, 36, 36]                               # the cube's fragment stands: 12 triangles
    eng.close()


# ------------------------------------------------------------------ 12: errors
def run_errors(E):
    bare = E.Engine(0)
    for call in (lambda: bare.scene_fragments(None), lambda: bare.scene_fragments_async([0])):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == engine.E_STATE                                   # no resident pieces
    bare.close()
    eng, _ = scene_after_click_one(E)
    cube = TS.bodies(E)["cube"]
    eng.upload_pattern(cube["face_off"], cube["v012"])
    eng.place_cells(cube["scale"], cube["translate"])
    eng.scene_fracture_event(0, 0, 8, flags=3)
    co, cp = eng.event_regroup()
    before, event, counts = TS.snapshot(eng), eng.download(), bytes(eng.event_counts())

    def refused(code, call):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == code, e.value
        TS.assert_unchanged(eng, before)
        assert bytes(eng.event_counts()) == counts
        now = eng.download()
        for k in ARRAYS + ("frag_ids",):
            assert np.asarray(now[k]).tobytes() == np.asarray(event[k]).tobytes(), k
    for form in (eng.scene_fragments, eng.scene_fragments_async):
        for bad in ([6], [0, 6], [0xFFFFFFFF], [2, 2], [0, 1, 0], []):        # out of range, listed twice, an empty list
            refused(engine.E_INVALID, lambda: form(bad))
        for flags in (engine.EVT_REFIT, engine.EVT_REFIT | engine.EVT_RENDER, 4, 0x80000002):
            refused(engine.E_INVALID, lambda: form(None, flags=flags))
            refused(engine.E_INVALID, lambda: form([1], flags=flags))
    # n_targets == 0 with a non-NULL list, through the C ABI itself
    one = np.zeros(1, np.uint32)
    refused(engine.E_INVALID, lambda: eng._ck(engine.lib().surtr_scene_fragments_async(eng._h, ctypes.c_uint32(0), ctypes.c_void_p(one.ctypes.data),
                                                                                     ctypes.c_int(0), ctypes.c_uint32(2))))
    # the refused calls left the scene event pending: it still commits
    n, first, n_new, _ = eng.scene_commit(co, cp)
    assert first == 5 and n_new >= 1
    eng.close()


# ------------------------------------------------------------------ CPU tier (emulation)
def test_all_compounds_a_list_and_no_render(emul_engine):
    run_all_and_list(emul_engine)


def test_render_convex_and_single_pieces(emul_engine):
    run_render_convex(emul_engine)


def test_compounds_of_a_second_commit(emul_engine):
    run_after_commit(emul_engine)


def test_poses_change_nothing_until_baked(emul_engine):
    run_poses(emul_engine)


def test_refit_and_mass_of_the_presented_fragments(emul_engine):
    run_refit_mass(emul_engine)


def test_scene_untouched_and_state_rules(emul_engine):
    run_untouched_and_state(emul_engine)


def test_flagged_piece_keeps_its_status(emul_engine):
    run_flagged(emul_engine)


def test_errors_leave_scene_and_event_unchanged(emul_engine):
    run_errors(emul_engine)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_scene_fragments as T
    case = sys.argv[1]
    if case == "async":
        T.run_async(engine, torch)
    elif case == "harness":
        T.check_harness(engine, %(root)r)
    else:
        getattr(T, "run_" + case)(engine)
    print("ok", case)
""")


def run_async(E, torch):
    """Case 13: the _async form on a stream of its own with six events in flight, against the synchronous result."""
    eng, _ = scene_after_click_one(E)
    results = []
    for compounds, rc in ((None, False), ([5, 2, 0], True)):
        eng.scene_fragments(compounds, render_convex=rc)
        results.append((bytes(eng.event_counts()), eng.download()))
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    eng.set_events_in_flight(6)
    with torch.cuda.stream(st):
        for (compounds, rc), (counts, want) in zip(((None, False), ([5, 2, 0], True)), results):
            eng.scene_fragments_async(compounds, render_convex=rc)
            eng.scene_fragments_async(compounds, render_convex=rc)        # twice: the staging tables are refilled with the first still queued
            assert bytes(eng.event_counts()) == counts
            got = eng.download()
            for k in ARRAYS + ("frag_ids",):
                assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    st.synchronize()
    eng.close()


def fnv1a(*arrays):
    h = 0xCBF29CE484222325
    for a in arrays:
        for byte in np.ascontiguousarray(a).tobytes():
            h = ((h ^ byte) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def check_harness(E, root, exe=None):
    """Case 14: surtr_harness --scene-clicks ... --init-compounds against the Python calls: totals and hashes of every compound made."""
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    clicks = [([-10.0, 0.3, 0.2], [1.0, 0.0, 0.0]), ([0.3, 0.2, 10.0], [0.0, 0.0, -1.0])]
    arg = ";".join(",".join("%r" % x for x in o + d) for o, d in clicks)
    p = subprocess.run([exe, "--mesh", "cube", "--cells", "8", "--scene-clicks", arg, "--impact-radius", "2.0", "--init-compounds"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [json.loads(x) for x in p.stdout.strip().splitlines() if x.startswith('{"init_compound"')]
    sc = scenes.cube_scene(8)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, 8)
    n = eng.pieces_from_event()
    eng.scene_set_compounds(list(range(0, n, 2)) + [n])
    want = []
    for k, (o, d) in enumerate(clicks):
        made = TS.python_click(eng, o, d, 2.0, 8)["compounds_made"]
        table = eng.scene_compounds()
        eng.scene_fragments(made)
        ev = eng.download()
        f = 0
        for c in made:
            m = int(table[c + 1] - table[c])
            a, b = int(ev["mesh_vert_off"][f]), int(ev["mesh_vert_off"][f + m])
            i0, i1 = int(ev["idx_off"][f]), int(ev["idx_off"][f + m])
            want.append(dict(init_compound=c, click=k, pieces=m, vertices=b - a, indices=i1 - i0, fnv=fnv1a(ev["vnc"][a:b], ev["idx"][i0:i1])))
            f += m
    assert lines == want and len(want) >= 2, (lines, want)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["all_and_list", "render_convex", "after_commit", "poses", "refit_mass", "untouched_and_state", "flagged", "errors", "async"])
def test_gpu_scene_fragments(case):
    run_gpu_child(GPU_CHILD, case, 120)


@pytest.mark.gpu
def test_gpu_harness_init_compounds():
    run_gpu_child(GPU_CHILD, "harness", 150)
