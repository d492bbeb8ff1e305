"""The C++ host layer over the cooked hulls: surtr_harness ... --init-compounds --hulls --cook (FractureEngine::InitCompounds with
cookUnusable, surtr::CookedUsable) against the Python calls -- counts, statuses, totals and the FNV-1a of points + polygons + indices of
every compound the clicks made; without --cook the lines are the ones --hulls printed before the flag existed, and with it everything
but the cook fields is unchanged (InitCompounds fills Cooked and leaves the rest of its result alone).

CPU tier: surtr_harness_emul (the host layer over the emulation library) and surtr_harness_san (product sources, host layer and harness
in one executable under AddressSanitizer / UndefinedBehaviorSanitizer, run directly: nothing is preloaded).  GPU tier: surtr_harness."""
import json
import os
import subprocess
import textwrap

import numpy as np
import pytest

import cook_ref as CR
import test_scene as TS
import test_scene_fragments as SF
from helpers import run_gpu_child
from surtr_amd import engine, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
TOL = 7e-6
COOK_KEYS = ("cooked", "cooked_usable", "cook_status", "cook_points", "cook_polygons", "cook_indices", "cook_fnv")


def check_harness(E, root, exe=None, clean_stderr=False):
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    clicks = [([-10.0, 0.3, 0.2], [1.0, 0.0, 0.0]), ([0.3, 0.2, 10.0], [0.0, 0.0, -1.0])]
    arg = ";".join(",".join("%r" % x for x in o + d) for o, d in clicks)
    base = [exe, "--mesh", "cube", "--cells", "8", "--scene-clicks", arg, "--impact-radius", "2.0", "--init-compounds", "--hulls"]
    out = {}
    for flag in ((), ("--cook",)):
        p = subprocess.run(base + list(flag), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        assert not clean_stderr or p.stderr == "", p.stderr[-2000:]
        out[flag] = [json.loads(x) for x in p.stdout.strip().splitlines() if x.startswith('{"init_compound"')]
    # everything but the cook fields is what the call without the flag gives
    assert len(out[()]) >= 2 and [{k: v for k, v in line.items() if k not in COOK_KEYS} for line in out[("--cook",)]] == out[()]
    assert all(set(COOK_KEYS) <= set(line) for line in out[("--cook",)]) and not any(set(COOK_KEYS) & set(line) for line in out[()])
    sc = scenes.cube_scene(8)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, 8)
    n = eng.pieces_from_event()
    eng.scene_set_compounds(list(range(0, n, 2)) + [n])
    want, n_cooked = [], 0
    for k, (o, d) in enumerate(clicks):
        made = TS.python_click(eng, o, d, 2.0, 8)["compounds_made"]
        table = eng.scene_compounds()
        eng.scene_fragments(made)
        hl = eng.event_hulls()
        ck = eng.event_cook(hl["records"], 1e-5, 0.0, TOL)
        refused = [not engine.hull_usable(r, 1e-5) for r in hl["records"]]
        assert [not int(r["status"]) & CR.SKIPPED for r in ck["records"]] == refused      # Cooked exactly for the pieces HullUsable refuses
        f = 0
        for c in made:
            m = int(table[c + 1] - table[c])
            r = ck["records"][f:f + m]
            pa, pb = int(r[0]["pt_off"]), int(r[-1]["pt_off"]) + int(r[-1]["nv"])
            fa, fb = int(r[0]["face_off"]), int(r[-1]["face_off"]) + int(r[-1]["n_faces"])
            ia, ib = int(r[0]["idx_off"]), int(r[-1]["idx_off"]) + int(r[-1]["n_idx"])
            took = [x for x in r if not int(x["status"]) & CR.SKIPPED]
            want.append(dict(cooked=len(took), cooked_usable=sum(engine.cooked_usable(x, TOL) for x in took),
                             cook_status=int(np.bitwise_or.reduce([int(x["status"]) for x in took] or [0])), cook_points=pb - pa, cook_polygons=fb - fa,
                             cook_indices=ib - ia, cook_fnv=SF.fnv1a(ck["points"][pa:pb], ck["polygons"][fa:fb], ck["idx"][ia:ib])))
            n_cooked += len(took)
            f += m
    got = [{k: line[k] for k in COOK_KEYS} for line in out[("--cook",)]]
    assert got == want, (got, want)
    eng.close()
    return n_cooked


@pytest.fixture(scope="module")
def harness_emul(emul_lib_path):
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, "surtr_harness_emul"])
    return os.path.join(EMUL_DIR, "surtr_harness_emul")


@pytest.fixture(scope="module")
def harness_san():
    subprocess.check_call(["make", "-s", "-j%d" % min(16, os.cpu_count() or 1), "-C", EMUL_DIR, "surtr_harness_san"])
    return os.path.join(EMUL_DIR, "surtr_harness_san")


def test_emulated_harness_cook(emul_engine, harness_emul):
    assert check_harness(emul_engine, ROOT, harness_emul) > 0      # (the two clicks make pieces HullUsable refuses: something is cooked)


def test_sanitized_harness_cook(emul_engine, harness_san):
    assert check_harness(emul_engine, ROOT, harness_san, clean_stderr=True) > 0


GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_cook_host as T
    assert T.check_harness(engine, %(root)r) > 0
    print("ok", sys.argv[1])
""")


@pytest.mark.gpu
def test_gpu_harness_cook():
    run_gpu_child(GPU_CHILD, "harness", 150)
