"""The pattern library in the C++ host layer (FractureEngine::StorePattern / SelectPattern / PatternCount / ClearPatterns, Impact::pattern
and Impact::partial in ExecuteFractureRoutine(impacts) and OnImpacts) through the harness: --patterns "cells:mean[:seed];..." and
--impacts "x,y,z,r[,pattern[,partial]];...".

The frame is test_scene_impacts.run_harness' (the scene of --body-clicks, body 1 posed, body 3 far away; the first sphere reaches body 1
alone, the second bodies 0 and 2, the third is dropped), with a stored pattern and a flag per sphere.  The same line with --one-event
(place_cells_patterns, one event over CELLS_ALL, event_regroup_impacts_partial, one commit) and without it (SelectPattern before each
sequential cycle of the calls that were there before) must print the same text: table, poses, the bodies' masses to 17 digits, and
with --init-compounds --hulls the hashes of every compound made.  cell_base is the prefix sum of the patterns' cells.

--pattern-pair (check_pair): FractureEngine::PrepareFracturePatterns and UsePatternPair, after which DoFracture picks the partial or the
general pattern by FractureArgs::PartialFracture (Src/Surtr.cpp:1806-1807, 1887), against DoFracture after GenerateFracturePattern of
that pattern.

Conditions, on the sequential form alone: the line differs from the one without the optional fields (the patterns and flags matter),
and from the one with patterns and flags exchanged.

CPU tier: surtr_harness_emul, and once surtr_harness_san (a program of its own) against it, byte for byte, as tests/test_host_cpu.py
does.  GPU tier: the same command lines on surtr_harness in a child process under a time limit."""
import json
import os
import subprocess
import textwrap

import pytest

from helpers import ROOT, run_gpu_child
from test_host_cpu import harness_emul, harness_san, pose_arg, run_both      # noqa: F401 (the two fixtures build the programs)

SPHERES = ["-1.0,6.3,0.2,5.0", "0.3,0.2,3.2,4.0", "-2.5,2.5,0.0,3.0"]
PATTERNS = "6:0.2;12:1.0:7"
TAIL = ["--init-compounds", "--hulls"]


def frame_args(fields, patterns=PATTERNS):
    """fields: what follows x,y,z,r of every sphere ('' for none)."""
    args = ["--mesh", "cube", "--cells", "8", "--scene-poses", pose_arg()]
    if patterns:
        args += ["--patterns", patterns]
    return args + ["--impacts", ";".join(s + f for s, f in zip(SPHERES, fields))] + TAIL


CHOSEN, SWAPPED, PLAIN, INSTALLED = (",0,1", ",1,0", ""), (",1,0", ",0,1", ""), ("", "", ""), (",-1,0", ",1", ",0,1")


def scene_lines(out):
    return [x for x in out.splitlines() if x.startswith(('{"impacts"', '{"init_compound"'))]


def run(exe, args):
    p = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (args, p.stdout[-2000:], p.stderr[-2000:])
    return scene_lines(p.stdout)


def check_frames(E, root, exe=None):
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    seq = {}
    for name, fields, base in (("chosen", CHOSEN, [0, 6, 18]), ("swapped", SWAPPED, [0, 12, 18]), ("installed", INSTALLED, [0, 8, 20])):
        seq[name] = run(exe, frame_args(fields))
        one = run(exe, frame_args(fields) + ["--one-event"])
        assert len(seq[name]) >= 4 and one == seq[name], (name, seq[name], one)          # the frame's line and a line per compound made
        line = json.loads(one[0])
        assert line["impacts"] == 2 and line["compounds_hit"] == [[1], [0, 2]] and line["cell_base"] == base, (name, line)
    # without the two fields the harness prints what it printed before them, with or without --patterns
    plain = run(exe, frame_args(PLAIN, patterns=None))
    assert plain == run(exe, frame_args(PLAIN) + ["--one-event"])
    assert "cell_base" not in json.loads(plain[0])
    tables = {k: json.dumps([json.loads(v[0])[f] for f in ("table", "mass")]) for k, v in dict(seq, plain=plain).items()}
    assert len(set(tables.values())) == 4, tables      # every choice of patterns and flags leaves another scene
    # a pattern that is not stored
    # (the sequential form stores the installed pattern for the impacts that name none: that must not make id 2 a stored one)
    p = subprocess.run([exe] + frame_args((",2,1", "", "")), capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "code 1" in p.stderr and not scene_lines(p.stdout), (p.returncode, p.stderr[-500:])


def check_pair(E, root, exe=None):
    """--pattern-pair: PrepareFracturePatterns + UsePatternPair make DoFracture select by PartialFracture; every line equals the one after
    GenerateFracturePattern of the pattern that flag picks."""
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    p = subprocess.run([exe, "--mesh", "cube", "--cells", "8", "--patterns", "6:0.05;14:1.0", "--pattern-pair"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    lines = [json.loads(x) for x in p.stdout.splitlines() if x.startswith('{"pattern_pair"')]
    assert [(x["pattern_pair"], x["partial"]) for x in lines] == [("pair", 1), ("pair", 0), ("pair", 1), ("built", 1), ("built", 0)]
    assert all(x["patterns"] == 2 for x in lines)
    same = lambda a, b: {k: v for k, v in a.items() if k != "pattern_pair"} == {k: v for k, v in b.items() if k != "pattern_pair"}
    assert same(lines[0], lines[3]) and same(lines[1], lines[4]) and same(lines[0], lines[2])
    assert lines[0]["fragments"] > 0 and lines[1]["fragments"] > 0 and lines[0]["fragments"] != lines[1]["fragments"], lines      # the flag picks another pattern


def test_harness_pattern_pair(emul_engine, harness_emul):
    check_pair(emul_engine, ROOT, harness_emul)


def test_harness_frames_one_event_equals_sequential(emul_engine, harness_emul):
    check_frames(emul_engine, ROOT, harness_emul)


def test_harness_frames_sanitized(harness_emul, harness_san):
    for extra in ([], ["--one-event"]):
        out = run_both(frame_args(CHOSEN) + extra, {}, harness_emul, harness_san)
        assert json.loads(scene_lines(out)[0])["cell_base"] == [0, 6, 18]
    assert '"pattern_pair"' in run_both(["--mesh", "cube", "--cells", "8", "--patterns", "6:0.05;14:1.0", "--pattern-pair"], {}, harness_emul, harness_san)


GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    from surtr_amd import engine
    import test_pattern_library_host as T
    case = sys.argv[1]
    getattr(T, "check_" + case)(engine, %(root)r)
    print("ok", case)
""")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["frames", "pair"])
def test_gpu_harness_pattern_library(case):
    run_gpu_child(GPU_CHILD, case, 150)
