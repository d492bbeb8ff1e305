"""The C++ host layer (surtr_amd/host/surtr_host.cpp + harness.cpp) on the CPU tier, plain and under sanitizers.

The layer makes no HIP call: it is a client of the C ABI, and tests/emul/libsurtr_emul.so exports all of that.  tests/emul/Makefile
builds two programs from the two files, unchanged (neither is part of `make all`; the fixtures below build them):
 * surtr_harness_emul -- linked against libsurtr_emul.so;
 * surtr_harness_san  -- the product sources, the host layer and the harness in ONE executable under AddressSanitizer and
   UndefinedBehaviorSanitizer (-fno-sanitize-recover=undefined: the first report ends the run).  It is a program with its own main,
   run directly: no library is preloaded and nothing sanitized is loaded into Python.

(a) test_emulated_harness: every harness check of the GPU tier -- the eight check_harness / run_harness functions of test_scene*.py,
    test_hulls.py and test_pick_queries.py and the two check_cpp_* of test_gpu_parity.py -- with surtr_harness_emul as the program and
    the emulated engine beside it, asserting what they assert on the GPU.  Sizes: the scene checks as they are (the cube x 8 cells);
    --api-dump on the 60 x 36 torus x 64 cells, as on the GPU; the plain event on the same torus (256 cells of the 100 x 60 torus on
    the GPU: the layer takes no other branch for it); the --obj-in ... --ach --obj round trip on blob(2) x 16 cells.
(b) test_sanitized_harness: every command line that (a) ran (recorded while it ran; a mesh file it read is kept and written again)
    goes through surtr_harness_san and surtr_harness_emul side by side: exit status 0, no report on stderr, and stdout and every
    file written byte for byte the emulated program's -- both are g++ -O1 with contraction off.
(c) --edit-bodies (harness.cpp): FractureEngine::RemoveBodies, AddBodies, TransformCompound and PieceHulls, which no other option
    calls, and the refusals they document, against Engine.scene_remove, scene_append, scene_transform_compound and pieces_hulls on
    a second engine, text for text: on the emulated program, on the sanitized one, and (marked gpu, in a child under a time limit)
    on the real one.
(d) test_sanitized_only: two command lines no check states, through the sanitized program against the emulated one as in (b):
    --impacts on two disjoint bodies with --one-event, and two radial --body-clicks with --one-event, each with --init-compounds
    --hulls behind it.

Leak detection is on (LeakSanitizer's default); no sanitizer option is set and there is no suppression file.

That the tiers can fail was tried by hand, each edit made, run and taken back; TRIED below says what each gave.

Not covered: FractureEngine::AllowFlagged / LastFlagged.  A flagged unit needs one of the golden .npz solids, which the harness cannot
read; surtr_rccl.cpp and harness_mgpu.cpp need RCCL and stay on the GPU tier.

Build and run times: see BUILD_TIME and RUNTIME below (measured once)."""
import json
import os
import subprocess
import tempfile
import textwrap

import numpy as np
import pytest

from helpers import ROOT, run_gpu_child
from surtr_amd import engine, scenes

import test_gpu_parity as GP
import test_hulls as TH
import test_pick_queries as PQ
import test_scene as TS
import test_scene_bodies as TSB
import test_scene_fragments as SF
import test_scene_impacts as TSI
import test_scene_poses as TSP
import test_scene_upkeep as TSU

BUILD_TIME = ("make -j16 surtr_harness_san from nothing: 83 s and 105 s in two builds on eight cores (173 s of CPU time; surtr_hip.hip alone is most of the wall time); "
              "surtr_harness_emul behind a built libsurtr_emul.so: 8 s")
RUNTIME = "7.4 s for the 24 tests not marked gpu, both programs built (no test above 0.6 s)"
TRIED = """
 * abort() at the head of FractureEngine::RemoveBodies, AddBodies, TransformCompound and PieceHulls, one at a time:
   test_emulated_harness[edit_bodies] fails each time (and with it the sanitized and the gpu form of the same check).
 * `__shared__ float part[SURTR_NWAVE][6]` of k_bounds_pieces (upkeep_dev.hip) declared [5]: test_sanitized_harness[upkeep],
   [edit_bodies] and test_edit_bodies_sanitized fail with "upkeep_dev.hip:73: runtime error: index 5 out of bounds for type 'float [5]'".
 * `__shared__ float4 plane[RG_MAXH]` of k_scene_outside and k_scene_outside_impacts (regroup_dev.hip) declared one shorter: every test
   PASSES.  The scenes here are fragments of a cube and of a small torus, a few dozen faces each; none comes near 4096 planes, so no
   run indexes the last element.  An extent that only a solid at its limit reaches is not checked by this tier: that takes a harness
   option that reads such a solid.
 * a read of `table.data()[table.size()]` in the one-compound FractureEngine::ExecuteFractureRoutine (surtr_host.cpp): eight
   sanitized tests fail with AddressSanitizer's heap-buffer-overflow report, that function its first frame (every scenario that clicks
   without --one-event).
 * an `int[10]` allocated in the harness' main and dropped: LeakSanitizer reports the 40 bytes and the run ends with a status that is
   not 0 -- leak detection works where this was measured, and stays on."""

EMUL_DIR = os.path.join(ROOT, "tests", "emul")
REPORTS = ("runtime error:", "AddressSanitizer", "LeakSanitizer")
CPU_SIZES = {"host_layer": {"torus": (64, 60, 36), "blob": (2, 16)}, "api_surface": GP.API_SURFACE_SIZES}


# ------------------------------------------------------------------ the two programs
@pytest.fixture(scope="module")
def harness_emul(emul_lib_path):
    subprocess.check_call(["make", "-s", "-C", EMUL_DIR, "surtr_harness_emul"])
    return os.path.join(EMUL_DIR, "surtr_harness_emul")


@pytest.fixture(scope="module")
def harness_san():
    subprocess.check_call(["make", "-s", "-j%d" % min(16, os.cpu_count() or 1), "-C", EMUL_DIR, "surtr_harness_san"])
    return os.path.join(EMUL_DIR, "surtr_harness_san")


# ------------------------------------------------------------------ (a) the GPU tier's harness checks
CHECKS = {
    "scene_clicks": lambda E, oracle, exe: TS.check_harness(E, ROOT, exe),
    "body_clicks_one_event": lambda E, oracle, exe: TSB.check_harness(E, ROOT, exe),
    "body_clicks_poses": lambda E, oracle, exe: TSP.check_harness(E, ROOT, exe),
    "impacts_one_event": lambda E, oracle, exe: TSI.run_harness(E, exe),
    "init_compounds": lambda E, oracle, exe: SF.check_harness(E, ROOT, exe),
    "hulls": lambda E, oracle, exe: TH.check_harness(E, ROOT, exe),
    "pick": lambda E, oracle, exe: PQ.check_harness(E, ROOT, exe),
    "upkeep": lambda E, oracle, exe: TSU.check_harness(E, ROOT, exe),
    "host_layer": lambda E, oracle, exe: GP.check_cpp_host_layer_and_harness(E, oracle, exe, CPU_SIZES["host_layer"]),
    "api_surface": lambda E, oracle, exe: GP.check_cpp_api_surface(E, oracle, exe, CPU_SIZES["api_surface"]),
    "edit_bodies": lambda E, oracle, exe: check_edit_bodies(E, ROOT, exe),
}
FILE_IN, FILE_OUT = ("--obj-in",), ("--api-dump", "--obj")
_RECORDS = {}


def recorded(name, E, oracle, exe, monkeypatch):
    """Runs CHECKS[name] once per session with `exe`, keeping every command line it gave to `exe` (and the bytes of a file named
    behind --obj-in).  -> (the command lines, the exception the check ended with or None)."""
    if name not in _RECORDS:
        lines = []

        def keep(cmd):
            if isinstance(cmd, (list, tuple)) and cmd and cmd[0] == exe:
                files = {cmd[i + 1]: open(cmd[i + 1], "rb").read() for i, a in enumerate(cmd[:-1]) if a in FILE_IN}
                lines.append((list(cmd[1:]), files))

        run = subprocess.run
        with monkeypatch.context() as m:
            m.setattr(subprocess, "run", lambda cmd, *a, **k: (keep(cmd), run(cmd, *a, **k))[1])      # (check_output goes through run)
            try:
                CHECKS[name](E, oracle, exe)
                _RECORDS[name] = (lines, None)
            except Exception as e:      # (b) still runs what was recorded; (a) raises it again
                _RECORDS[name] = (lines, e)
    return _RECORDS[name]


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_emulated_harness(emul_engine, oracle, harness_emul, monkeypatch, name):
    lines, error = recorded(name, emul_engine, oracle, harness_emul, monkeypatch)
    if error is not None:
        raise error
    assert lines, "the check never started the program"


# ------------------------------------------------------------------ (b) the same command lines under the sanitizers
def run_both(args, files, emul, san):
    """One command line through both programs in a fresh directory: files named behind FILE_IN are written there first, files named
    behind FILE_OUT are read after each run.  The sanitized run must end with status 0 and an empty report, and print and write what
    the emulated one did, byte for byte."""
    with tempfile.TemporaryDirectory() as d:
        args, outs = list(args), []
        for i, a in enumerate(args[:-1]):
            if a in FILE_IN:
                p = os.path.join(d, os.path.basename(args[i + 1]))
                with open(p, "wb") as f:
                    f.write(files[args[i + 1]])
                args[i + 1] = p
            elif a in FILE_OUT:
                args[i + 1] = os.path.join(d, os.path.basename(args[i + 1]))
                outs.append(args[i + 1])
        got = []
        for exe in (emul, san):
            p = subprocess.run([exe] + args, capture_output=True, timeout=300)
            err = p.stderr.decode(errors="replace")
            written = []
            for o in outs:
                written.append(open(o, "rb").read() if os.path.exists(o) else None)
                if os.path.exists(o):
                    os.remove(o)
            got.append((p.returncode, p.stdout, written))
            if exe == san:
                assert not any(r in err for r in REPORTS), (args, err[:6000])
                assert p.returncode == 0, (args, p.returncode, err[-3000:])
        assert got[0][0] == 0, (args, got[0])
        assert got[1][1] == got[0][1], (args, got[0][1][-2000:], got[1][1][-2000:])
        assert got[1][2] == got[0][2] and all(w is not None for w in got[0][2]), args
        return got[0][1].decode()


@pytest.mark.parametrize("name", sorted(CHECKS))
def test_sanitized_harness(emul_engine, oracle, harness_emul, harness_san, monkeypatch, name):
    lines, _ = recorded(name, emul_engine, oracle, harness_emul, monkeypatch)
    assert lines, "the check never started the program"
    for args, files in lines:
        run_both(args, files, harness_emul, harness_san)


# ------------------------------------------------------------------ (d) two more scenarios, sanitized against emulated
def pose_arg():
    return ";".join("%d:" % c + ",".join("%r" % float(x) for x in W.reshape(-1)) for c, W in ((1, TSP.HARNESS_POSE), (3, TSP.HARNESS_FAR)))


def test_sanitized_only(harness_emul, harness_san):
    cube = ["--mesh", "cube", "--cells", "8", "--scene-poses", pose_arg()]
    # test_scene_impacts.run_harness' frame: the first sphere reaches body 1 alone, the second bodies 0 and 2, the third is dropped
    out = run_both(cube + ["--impacts", "-1.0,6.3,0.2,5.0;0.3,0.2,3.2,4.0;-2.5,2.5,0.0,3.0", "--one-event", "--init-compounds", "--hulls"], {},
                   harness_emul, harness_san)
    frame = [json.loads(x) for x in out.splitlines() if x.startswith('{"impacts"')]
    assert len(frame) == 1 and frame[0]["compounds_hit"] == [[1], [0, 2]]
    made = [json.loads(x) for x in out.splitlines() if x.startswith('{"init_compound"')]
    assert [m["init_compound"] for m in made] == frame[0]["compounds_made"] and all(m["hull_polygons"] >= 4 * m["pieces"] for m in made)
    # test_scene_bodies.check_harness' two radial clicks
    out = run_both(cube + ["--body-clicks", "-10.0,6.3,0.2,1.0,0.0,0.0;0.3,0.2,10.0,0.0,0.0,-1.0", "--impact-radius", "4.0", "--radial", "--one-event",
                           "--init-compounds", "--hulls"], {}, harness_emul, harness_san)
    clicks = [json.loads(x) for x in out.splitlines() if x.startswith('{"body_click"')]
    made = [json.loads(x) for x in out.splitlines() if x.startswith('{"init_compound"')]
    assert len(clicks) == 2 and all(c["compounds_made"] for c in clicks)
    assert [m["init_compound"] for m in made] == clicks[0]["compounds_made"] + clicks[1]["compounds_made"]


# ------------------------------------------------------------------ (c) RemoveBodies, AddBodies, TransformCompound, PieceHulls
EDIT_CLICKS = [([-10.0, 6.3, 0.2], [1.0, 0.0, 0.0]), ([0.3, 0.2, 10.0], [0.0, 0.0, -1.0])]
# the poses of the two new bodies, and the matrix TransformCompound applies to the pieces of the second
EDIT_MATRICES = [TSP.pose_about(TSP.rotation((1, 2, 3), 0.9), (0, 0, 0), (0, -30, 0)), PQ.world(np.eye(3), (0, 30, 0)),
                 TSP.pose_about(TSP.rotation((0, 1, 0), 0.7), (8, 0, 0), (1, 2, 3))]


def scene_text(eng, edit):
    """The line print_scene_state (harness.cpp) prints: table, poses, body masses, bounds -- %u, %.9g of a float, %.17g of a double."""
    b = eng.scene_bounds(set=1)
    return '{"edit": "%s", "table": [%s], "poses": [%s], "mass": [%s], "bounds": [%s]}' % (
        edit, ", ".join("%d" % x for x in eng.scene_compounds()),
        ", ".join("[" + ", ".join("%.9g" % float(x) for x in W.reshape(-1)) + "]" for W in eng.scene_poses()),
        ", ".join("%.17g" % float(x) for x in eng.scene_mass(set=1)["mass"]),
        ", ".join("[" + ", ".join(["%.9g" % float(x) for x in r["lo"]] + ["%.9g" % float(x) for x in r["hi"]] + ["%d" % r["n_vertices"], "%d" % r["status"]]) + "]"
                  for r in b))


def refused(call):
    with pytest.raises(engine.SurtrError) as e:
        call()
    return e.value.code


def check_edit_bodies(E, root, exe=None):
    """surtr_harness --body-clicks ... --edit-bodies against the same clicks and edits through the Python calls, line for line as
    text.  Conditions, asserted on the reference: the clicks leave at least four bodies, one of them posed; the removal takes the
    first and the last; the second new body has two pieces; the transform changes that body's bounds and no other's."""
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
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
    for o, d in EDIT_CLICKS:
        TSP.python_body_click(eng, o, d, 4.0, 8, False)
    bodies = [[{"mesh": sc["mesh"], "conv": sc["convex"]}],
              [{"mesh": TS.shifted(sc["mesh"], (dx, 0, 0)), "conv": TS.shifted(sc["convex"], (dx, 0, 0))} for dx in (8, 16)]]
    table = eng.scene_compounds()
    nc = len(table) - 1
    assert nc >= 4 and any(W.tobytes() == TSP.HARNESS_FAR.tobytes() for W in eng.scene_poses()[1:nc - 1])
    want = []
    # the refusals: E_INVALID from each, and the scene as it was
    codes = (refused(lambda: eng.scene_remove([nc])), refused(lambda: eng.scene_append(bodies, world=EDIT_MATRICES[:1])),
             refused(lambda: eng.transform_pieces(np.tile(np.eye(4, dtype=np.float32), (int(table[-1]) - 1, 1, 1)))))
    assert codes == (E.E_INVALID,) * 3
    want.append('{"refused": {"remove_out_of_range": %d, "add_pose_count": %d, "transform_matrix_count": %d}}' % codes)
    want.append(scene_text(eng, "refused"))
    assert [int(x) for x in eng.scene_compounds()] == [int(x) for x in table]
    eng.scene_remove([nc - 1, 0])
    want.append(scene_text(eng, "remove"))
    first = eng.scene_append(bodies, world=np.asarray(EDIT_MATRICES[:2]))
    assert first == nc - 2
    want.append('{"first_new": %d}' % first)
    want.append(scene_text(eng, "add"))
    table = eng.scene_compounds()
    assert int(table[first + 2] - table[first + 1]) == 2
    before = eng.scene_bounds(set=1)
    eng.scene_transform_compound(first + 1, [EDIT_MATRICES[2]] * 2)
    after = eng.scene_bounds(set=1)
    assert before[:first + 1].tobytes() == after[:first + 1].tobytes() and before[first + 1].tobytes() != after[first + 1].tobytes()
    want.append(scene_text(eng, "transform"))
    hl = eng.pieces_hulls()
    assert hl["records"].shape[0] == int(table[-1])
    want.append('{"edit": "piece_hulls", "hulls": %d, "hull_polygons": %d, "hull_indices": %d, "hulls_usable": %d, "hull_fnv": "%s"}' % (
        hl["records"].shape[0], hl["polygons"].shape[0], hl["idx"].shape[0], sum(engine.hull_usable(r) for r in hl["records"]),
        SF.fnv1a(hl["polygons"], hl["idx"])))
    eng.close()
    cmd = [exe, "--mesh", "cube", "--cells", "8", "--scene-poses", pose_arg(), "--body-clicks", ";".join(",".join("%r" % x for x in o + d) for o, d in EDIT_CLICKS),
           "--impact-radius", "4.0", "--edit-bodies", ";".join(",".join("%r" % float(x) for x in W.reshape(-1)) for W in EDIT_MATRICES)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    got = [x for x in p.stdout.splitlines() if x.startswith(('{"refused"', '{"edit"', '{"first_new"'))]
    assert len(got) == len(want) == 7
    for g, w in zip(got, want):
        assert g == w, (g, w)


def test_edit_bodies_sanitized(emul_engine, harness_san):
    """(c) on the sanitized program itself: the Python calls run on the emulation library, as for the emulated program."""
    check_edit_bodies(emul_engine, ROOT, harness_san)


GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    from surtr_amd import engine
    import test_host_cpu as T
    case = sys.argv[1]
    getattr(T, "check_" + case)(engine, %(root)r)
    print("ok", case)
""")


@pytest.mark.gpu
def test_gpu_harness_edit_bodies():
    run_gpu_child(GPU_CHILD, "edit_bodies", 60)
