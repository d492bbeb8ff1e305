import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOPOLOGY_KEYS = ("frag_ids", "mesh_vert_off", "mesh_nbr_off", "mesh_nbr", "conv_vert_off", "conv_nbr_off", "conv_nbr",
                 "idx_off", "idx")
COORD_KEYS = ("mesh_pos", "conv_pos", "vnc")
RTOL = 1e-5   # north_star: "float intersection coordinates within 1e-5 relative"


def assert_event_equal(got, ref, render=True):
    for k in TOPOLOGY_KEYS:
        if k in ("idx_off", "idx") and not render:
            continue
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        assert np.array_equal(got[k], ref[k]), k
    for k in COORD_KEYS:
        if k == "vnc" and not render:
            continue
        assert got[k].shape == ref[k].shape, (k, got[k].shape, ref[k].shape)
        scale = max(1.0, float(np.abs(ref[k]).max())) if ref[k].size else 1.0
        assert np.allclose(got[k], ref[k], rtol=RTOL, atol=RTOL * scale * 1e-2), k


def run_event(engine_mod, oracle, sc, flags=3, cells=None, threads=4):
    eng = engine_mod.Engine(0)
    try:
        eng.upload_pieces([sc["mesh"]], [sc["convex"]])
        eng.upload_pattern(sc["face_off"], sc["v012"])
        eng.place_cells(sc["scale"], sc["translate"])
        n = sc["n_cells"] if cells is None else cells
        c = eng.fracture_event(0, n, flags=flags)
        got = eng.download()
    finally:
        eng.close()
    planes = oracle.place_cells(sc["v012"], sc["scale"], sc["translate"])
    ref = oracle.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=bool(flags & 1), render=bool(flags & 2),
                       threads=threads, cell_end=n)
    return c, got, ref


def run_gpu_child(template, case, seconds):
    """One case of a module's GPU tier in a child process of its own, under a time limit: template is the child's program with
    %(root)r and %(tests)r for the two import paths, and it prints "ok <case>" when the case has passed."""
    code = template % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}
    try:
        p = subprocess.run(["timeout", "-k", "10", str(seconds), sys.executable, "-c", code, case], cwd=ROOT, capture_output=True, text=True,
                           timeout=seconds + 30)
    except subprocess.TimeoutExpired:
        pytest.fail("%s: no result within %d s" % (case, seconds))
    print(p.stdout[-3000:])
    assert p.returncode == 0, (p.returncode, p.stdout[-3000:], p.stderr[-3000:])
    assert ("ok " + case) in p.stdout


def fragment(ev, k, which="mesh"):
    vo, no = ev[which[:4] + "_vert_off"], ev[which[:4] + "_nbr_off"]
    a, b = int(vo[k]), int(vo[k + 1])
    return {"pos": ev[which[:4] + "_pos"][a:b], "off": (no[a:b + 1] - no[a]).astype(np.uint32),
            "nbr": ev[which[:4] + "_nbr"][int(no[a]):int(no[b])]}


def solid_is_polyhedron(s):
    """Indices in range, no vertex linked to itself, every link has its way back: what Poly::ExtractNeighborFromMesh checks
    (Src/Poly.cpp:253-260) and what every walk of the path relies on."""
    n = s["pos"].shape[0]
    off, nbr = s["off"].astype(np.int64), s["nbr"].astype(np.int64)
    if nbr.size and (nbr.min() < 0 or nbr.max() >= n):
        return False
    rings = [nbr[off[v]:off[v + 1]] for v in range(n)]
    for v in range(n):
        for u in rings[v]:
            if u == v or v not in rings[u]:
                return False
    return True


def solid_has_doubled_neighbour(s):
    """Some ring lists a vertex twice: the shape every solid has that the reference produced by renumbering a link through a
    stale ID (two links collapse onto one vertex)."""
    off, nbr = s["off"].astype(np.int64), s["nbr"].astype(np.int64)
    return any(len(set(nbr[off[v]:off[v + 1]].tolist())) < off[v + 1] - off[v] for v in range(s["pos"].shape[0]))


def assert_event_equal_flagged(got, ref, render=True):
    """assert_event_equal for events with flags.  THE DEGENERATE POLICY: where the restated reference
    leaves its own arrays (an index that is no vertex, a link renumbered through a stale or never-set ID), or a walk of
    ExtractFaces never ends, the engine does not emulate what the reference's memory happens to hold: it FLAGS --
      * a pair whose Mesh clip has no valid answer yields no fragment (got["flagged_pairs"]: its (cell, piece); counted in
        n_failed): the reference's fragments of that pair are left out of the comparison, after checking that one of them
        really is no polyhedron;
      * a fragment whose refit has no valid answer keeps its un-refitted Convex (frag_status != 0): what is checked is that
        the reference's (restated) result really is invalid;
      * a fragment whose ExtractFaces does not end has no triangles on either side (plain comparison).
    Everything else is compared fragment by fragment, bit for bit."""
    st = got.get("frag_status")
    flagged = set(map(tuple, got.get("flagged_pairs", [])))
    if (st is None or not np.any(st)) and not flagged:
        return assert_event_equal(got, ref, render)
    rid = {tuple(r): i for i, r in enumerate(ref["frag_ids"].tolist())}
    dropped = [i for i, r in enumerate(ref["frag_ids"].tolist()) if (r[0], r[1]) in flagged]
    for pair in flagged:
        mine = [i for i in dropped if tuple(ref["frag_ids"][i][:2]) == pair]
        assert not mine or any(not solid_is_polyhedron(fragment(ref, i, w)) or solid_has_doubled_neighbour(fragment(ref, i, w))
                               for i in mine for w in ("mesh", "conv")), ("pair flagged although the reference's result for it is a regular polyhedron", pair)
    assert got["frag_ids"].shape[0] == ref["frag_ids"].shape[0] - len(dropped), (got["frag_ids"].shape, ref["frag_ids"].shape, len(dropped))
    for k in range(got["frag_ids"].shape[0]):
        key = tuple(got["frag_ids"][k].tolist())
        assert key in rid and (key[0], key[1]) not in flagged, ("fragment not in the reference's event", key)
        kr = rid[key]
        gm, rm = fragment(got, k, "mesh"), fragment(ref, kr, "mesh")
        assert np.array_equal(gm["off"], rm["off"]) and np.array_equal(gm["nbr"], rm["nbr"]), ("mesh", k)
        assert np.allclose(gm["pos"], rm["pos"], rtol=RTOL, atol=1e-6), ("mesh_pos", k)
        gc, rc = fragment(got, k, "conv"), fragment(ref, kr, "conv")
        same = gc["pos"].shape == rc["pos"].shape and np.array_equal(gc["off"], rc["off"]) and np.array_equal(gc["nbr"], rc["nbr"]) \
            and np.allclose(gc["pos"], rc["pos"], rtol=RTOL, atol=1e-6)
        if st is None or st[k] == 0:
            assert same, ("conv", k)
        elif not same:
            # the engine kept the un-refitted Convex: either the reference's result is no polyhedron, or on its way there it
            # stored a link that names no vertex (whatever it returns after that is an accident of its heap)
            from oracle import oracle as _O
            _O.links_off_the_array(reset=True)
            _O.refit(gc, gm, 4)
            undefined = _O.links_off_the_array(reset=True) > 0
            assert undefined or not solid_is_polyhedron(rc), ("fragment flagged although the reference's refit is well defined", k)
            assert solid_is_polyhedron(gc), ("conv kept", k)
        if render:
            a, b = int(got["idx_off"][k]), int(got["idx_off"][k + 1]); c, d = int(ref["idx_off"][kr]), int(ref["idx_off"][kr + 1])
            assert np.array_equal(got["idx"][a:b], ref["idx"][c:d]), ("idx", k)
