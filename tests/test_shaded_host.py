"""The C++ host layer over the lit render buffers: surtr_harness ... --init-compounds --lit (FractureEngine::SetRenderNormals +
InitCompounds' MeshLit, FractureEngine::ShadedRender, Poly::RenderPolyhedronNormal in both overloads) against the Python calls -- the
lit vertices, faces, fallback pieces and the FNV-1a of the lit vertices of every compound the clicks made, and the lit unit box; without
--lit the lines are the ones the harness printed before the flag existed, and with it everything but the lit fields is unchanged.
The harness itself ends with status 3 when ShadedRender differs from MeshLit or the overloads differ from each other.

CPU tier: surtr_harness_emul (the host layer over the emulation library) and surtr_harness_san (product sources, host layer and harness
in one executable under AddressSanitizer / UndefinedBehaviorSanitizer, run directly: nothing is preloaded).  GPU tier: surtr_harness."""
import json
import os
import subprocess
import textwrap

import pytest

import test_scene as TS
import test_scene_fragments as SF
from helpers import run_gpu_child
from surtr_amd import engine, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMUL_DIR = os.path.join(ROOT, "tests", "emul")
LIT_KEYS = ("lit_vertices", "lit_faces", "lit_fallback", "lit_fnv")
BOX_COLOUR = (0.5, 0.25, 0.125)


def check_harness(E, oracle, root, exe=None, clean_stderr=False):
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    clicks = [([-10.0, 0.3, 0.2], [1.0, 0.0, 0.0]), ([0.3, 0.2, 10.0], [0.0, 0.0, -1.0])]
    arg = ";".join(",".join("%r" % x for x in o + d) for o, d in clicks)
    base = [exe, "--mesh", "cube", "--cells", "8", "--scene-clicks", arg, "--impact-radius", "2.0", "--init-compounds"]
    out, box = {}, None
    for flag in ((), ("--lit",)):
        p = subprocess.run(base + list(flag), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        assert not clean_stderr or p.stderr == "", p.stderr[-2000:]
        lines = p.stdout.strip().splitlines()
        out[flag] = [json.loads(x) for x in lines if x.startswith('{"init_compound"')]
        boxes = [json.loads(x) for x in lines if x.startswith('{"lit_box"')]
        assert len(boxes) == (1 if flag else 0)
        box = boxes[0] if boxes else box
    # everything but the lit fields is what the call without the flag gives
    assert len(out[()]) >= 2 and [{k: v for k, v in line.items() if k not in LIT_KEYS} for line in out[("--lit",)]] == out[()], (out[()], out[("--lit",)])
    assert all(set(LIT_KEYS) <= set(line) for line in out[("--lit",)]) and not any(set(LIT_KEYS) & set(line) for line in out[()])
    sc = scenes.cube_scene(8)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, 8)
    n = eng.pieces_from_event()
    eng.scene_set_compounds(list(range(0, n, 2)) + [n])
    want, n_vertices = [], 0
    for k, (o, d) in enumerate(clicks):
        made = TS.python_click(eng, o, d, 2.0, 8)["compounds_made"]
        table = eng.scene_compounds()
        eng.scene_fragments(made)
        rec, vnc, _ = eng.event_shaded()
        f = 0
        for c in made:
            m = int(table[c + 1] - table[c])
            r = rec[f:f + m]
            a, b = int(r[0]["first_vertex"]), int(r[-1]["first_vertex"]) + int(r[-1]["n_vertices"])
            want.append(dict(lit_vertices=b - a, lit_faces=int(r["n_faces"].sum()), lit_fallback=int((r["status"] & engine.SHADE_PER_TRIANGLE != 0).sum()),
                             lit_fnv=SF.fnv1a(vnc[a:b])))
            n_vertices += b - a
            f += m
    got = [{k: line[k] for k in LIT_KEYS} for line in out[("--lit",)]]
    assert got == want, (got, want)
    assert [line["lit_vertices"] for line in out[("--lit",)]] == [line["indices"] for line in out[()]]      # one lit vertex per index
    # Poly::RenderPolyhedronNormal on the unit box: the Python call on Poly::GetBB
    b = oracle.unit_box()
    eng.load_fragments([b], [b])
    eng.event_triangulate(False)
    rec, vnc, _ = eng.event_shaded(BOX_COLOUR)
    assert box == {"lit_box": 36, "fnv": SF.fnv1a(vnc)} and rec[0]["n_faces"] == 6 and rec[0]["status"] == 0
    eng.close()
    return n_vertices


@pytest.fixture(scope="module")
def harness_emul(emul_lib_path):
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, "surtr_harness_emul"])
    return os.path.join(EMUL_DIR, "surtr_harness_emul")


@pytest.fixture(scope="module")
def harness_san():
    subprocess.check_call(["make", "-s", "-j%d" % min(16, os.cpu_count() or 1), "-C", EMUL_DIR, "surtr_harness_san"])
    return os.path.join(EMUL_DIR, "surtr_harness_san")


def test_emulated_harness_lit(emul_engine, oracle, harness_emul):
    assert check_harness(emul_engine, oracle, ROOT, harness_emul) > 0


def test_sanitized_harness_lit(emul_engine, oracle, harness_san):
    assert check_harness(emul_engine, oracle, ROOT, harness_san, clean_stderr=True) > 0


GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    from oracle import oracle
    import test_shaded_host as T
    oracle.lib()
    assert T.check_harness(engine, oracle, %(root)r) > 0
    print("ok", sys.argv[1])
""")


@pytest.mark.gpu
def test_gpu_harness_lit():
    run_gpu_child(GPU_CHILD, "harness", 150)
