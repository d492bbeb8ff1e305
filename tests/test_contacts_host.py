"""surtr_harness ... --body-clicks ... --contacts MARGIN: FractureEngine::Contacts and surtr::ImpactsFromContacts after every click,
against the same clicks and Engine.scene_contacts through the Python calls -- totals, a hash of the records' bytes and the derived
impacts.  On the emulated program, on the stand-alone sanitized one (an executable of its own: nothing is preloaded) and, marked gpu,
on the real one in a child process under a time limit."""
import json
import os
import subprocess
import textwrap

import numpy as np
import pytest

import test_scene_fragments as SF
import test_scene_poses as TSP
from helpers import run_gpu_child
from surtr_amd import engine, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
MARGIN = 0.25
RADIUS = 4.0


def impacts_from_contacts(rec, radius):
    """surtr::ImpactsFromContacts: one impact per body pair in order of first appearance, at the midpoint of the witness points of the
    pair's closest record (ties: the first), in float as the host layer computes it."""
    order, best = [], {}
    for r in rec:
        key = (int(r["body_a"]), int(r["body_b"]))
        if key not in best:
            order.append(key)
            best[key] = r
        elif r["distance"] < best[key]["distance"]:
            best[key] = r
    out = []
    for key in order:
        r = best[key]
        mid = (r["point_a"] + r["point_b"]) * np.float32(0.5)
        out.append([float(x) for x in mid] + [float(np.float32(radius)), key[0], key[1]])
    return out


def check_harness(E, root, exe=None, clean_stderr=False):
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    clicks = [([-10.0, 6.3, 0.2], [1.0, 0.0, 0.0]), ([0.3, 0.2, 10.0], [0.0, 0.0, -1.0])]
    arg = ";".join(",".join("%r" % x for x in o + d) for o, d in clicks)
    pose_arg = ";".join("%d:" % c + ",".join("%r" % float(x) for x in W.reshape(-1)) for c, W in ((1, TSP.HARNESS_POSE), (3, TSP.HARNESS_FAR)))
    cmd = [exe, "--mesh", "cube", "--cells", "8", "--scene-poses", pose_arg, "--body-clicks", arg, "--impact-radius", "%r" % RADIUS, "--contacts", "%r" % MARGIN]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    assert not clean_stderr or p.stderr == "", p.stderr[-2000:]
    lines = [json.loads(x) for x in p.stdout.strip().splitlines() if x.startswith('{"contacts"')]
    assert len(lines) == len(clicks)
    sc = scenes.cube_scene(8)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, 8)
    n = eng.pieces_from_event()
    eng.scene_set_compounds(list(range(0, n, 2)) + [n])
    poses = np.tile(np.eye(4, dtype=np.float32), ((n + 1) // 2, 1, 1))
    poses[1], poses[3] = TSP.HARNESS_POSE, TSP.HARNESS_FAR
    eng.scene_set_poses(poses)
    total = 0
    for k, (o, d) in enumerate(clicks):
        TSP.python_body_click(eng, o, d, RADIUS, 8, False)
        h = eng.scene_contacts_totals(MARGIN)
        rec = eng.scene_contacts(MARGIN)
        want = dict(contacts=k, records=int(rec.shape[0]), body_pairs=int(h["n_body_pairs"]), piece_pairs=int(h["n_piece_pairs"]),
                    fnv=SF.fnv1a(rec), impacts=impacts_from_contacts(rec, RADIUS))
        got = dict(lines[k])
        got_imp, want_imp = got.pop("impacts"), want.pop("impacts")
        assert got == want, (got, want)
        assert len(got_imp) == len(want_imp)
        for g, w in zip(got_imp, want_imp):
            assert [np.float32(x) for x in g[:4]] == [np.float32(x) for x in w[:4]] and g[4:] == w[4:], (g, w)
        assert len({(a, b) for *_, a, b in want_imp}) == len(want_imp) and all(a < b for *_, a, b in want_imp)
        total += rec.shape[0]
    eng.close()
    return total


@pytest.fixture(scope="module")
def harness_emul(emul_lib_path):
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, "surtr_harness_emul"])
    return os.path.join(EMUL_DIR, "surtr_harness_emul")


@pytest.fixture(scope="module")
def harness_san():
    subprocess.check_call(["make", "-s", "-j%d" % min(16, os.cpu_count() or 1), "-C", EMUL_DIR, "surtr_harness_san"])
    return os.path.join(EMUL_DIR, "surtr_harness_san")


def test_emulated_harness_contacts(emul_engine, harness_emul):
    assert check_harness(emul_engine, ROOT, harness_emul) > 0


def test_sanitized_harness_contacts(emul_engine, harness_san):
    assert check_harness(emul_engine, ROOT, harness_san, clean_stderr=True) > 0


GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_contacts_host as T
    assert T.check_harness(engine, %(root)r) > 0
    print("ok", sys.argv[1])
""")


@pytest.mark.gpu
def test_gpu_harness_contacts():
    run_gpu_child(GPU_CHILD, "harness", 150)
