"""The chunked plane loops (clip_core.h: planes_first_cut, planes_first_cut_ball) on designed cells.

A lane tests a point against the cell's planes in order up to the first plane that cuts it: P1 of the sorted pre-pass
(prep_sorted.h) for every vertex of the undecided groups, and the record clipper (wave_clip.h) and the general clipper
(clip_core.h) for the first clipping plane of every new vertex.  The loops take the planes in chunks (C = 2 in P1 and in the
general clipper, C = 4 in the record clipper) and read plane F - 1 again where the last chunk has spare places, so what can go
wrong sits at the chunk edges: a plane count that is no multiple of C, cutting planes that are the last of their chunk or the
first of the next, planes that cut nothing in between, a point that lies in a plane before the one that cuts it.

The piece is bumpy_torus(64, 40): 2 560 vertices, enough for k_prep_pairs_sorted.  Every case is ONE cell (one pair) whose plane
list is edited by hand: planes of a Voronoi cell of the piece, or up to three planes that leave the outer tip of the torus (so that
what is left fits the record clipper of the small-capacity emulation build too), plus redundant planes x = 100 + j that cut
nothing, are far from every ball and hold no vertex.  The event must equal the oracle's bit for bit with the record clipper on and off, and the
pair must take the route the case is about: a case without an in-plane vertex and with at most 64 planes is taken by the record
clipper and not handed on; a case with an in-plane vertex, or with 65 planes, goes to the general clipper.  One case has no route
through a clipper at all: where plane 0 removes every vertex, every vertex has the same first clipping plane, the pre-pass finds
no band and ends the pair (P1 still runs on the vertices next to the plane, and leaves at its first chunk).

Not designed here: a NEW vertex that lies in a later plane (the zero mask of the first-cut form).  Its position is computed, so no
plane list puts one there on purpose; the torus scenes of test_record_clipper.py and test_emul_parity.py meet such vertices."""
import os

import numpy as np
import pytest

from helpers import TOPOLOGY_KEYS, assert_event_equal
from surtr_amd import meshgen, scenes

CELLS = (16, 48, 56)      # cells of the 64-cell pattern whose every plane cuts the piece and holds none of its vertices
# the outer tip of the torus (x > 1.25 or so), then a slab of it in y, then its upper part: slightly skew, so that no vertex of the
# regular grid lies in one of them
TIP = (np.float32([-1, 0.03, 0.02, 1.25]), np.float32([0.05, 1, 0.02, -0.2]), np.float32([0.03, -1, 0.02, -0.25]))
C_REC, C_P1 = 4, 2        # SURTR_PLANE_CHUNK, SURTR_PLANE_CHUNK_P1 (= SURTR_PLANE_CHUNK_GEN)
# plane counts: 1, C - 1, C, C + 1, 2C, 2C + 1 for both chunk sizes, WC_MAXF and WC_MAXF + 1
COUNTS = sorted({1, C_P1 - 1, C_P1, C_P1 + 1, 2 * C_P1, 2 * C_P1 + 1, C_REC - 1, C_REC, C_REC + 1, 2 * C_REC, 2 * C_REC + 1, 64, 65})

_STATE = {}


def _dist(pl, p):
    """plane_dist in float32, in its order of operations"""
    t = pl[0] * p[:, 0] + pl[1] * p[:, 1]
    t = t + pl[2] * p[:, 2]
    return pl[3] + t


def _scene(oracle):
    if "sc" not in _STATE:
        v, t = meshgen.bumpy_torus(64, 40)
        sc = scenes.make_scene(v, t, 64)
        _STATE["sc"] = sc
        _STATE["planes"] = oracle.place_cells(sc["v012"], sc["scale"], sc["translate"])
        _STATE["pos"] = np.ascontiguousarray(sc["mesh"]["pos"], np.float32).reshape(-1, 3)
    return _STATE["sc"], _STATE["planes"], _STATE["pos"]


def _redundant(n, first=0):
    return [np.float32([1, 0, 0, -(100 + first + j)]) for j in range(n)]


def _cases(oracle):
    """name -> (plane list, route): route 'rec' = taken by the record clipper, 'general' = goes to the general clipper,
    'prepass' = the pre-pass leaves no band, so neither clipper is asked"""
    if "cases" in _STATE:
        return _STATE["cases"]
    sc, planes, pos = _scene(oracle)
    fo = sc["face_off"]
    real = {c: [planes[i] for i in range(int(fo[c]), int(fo[c + 1]))] for c in CELLS}
    tiny = np.float32(1e-10)
    for c, r in list(real.items()) + [("tip", TIP)]:      # what the cases below rely on
        for pl in r:
            s = _dist(pl, pos)
            assert (s >= tiny).any() and (s < 0).any() and not (np.abs(s) < tiny).any(), c
    cases = {}
    for F in COUNTS:
        r = list(TIP)
        R = 1 if F == 1 else min(F - 1, 3)
        red = _redundant(F - R)
        route = "rec" if F <= 64 else "general"
        cases["F%d-front" % F] = (red + r[:R], route)                       # (the only cutting planes are the last ones)
        if red:
            cases["F%d-end" % F] = (r[:R] + red, route)
        if red and R > 1:
            cases["F%d-middle" % F] = (r[:1] + red + r[1:R], route)
    # a whole cell with redundant planes after every one of its own, up to WC_MAXF planes; and behind 2C + 1 of them
    r = real[48]
    k, mix = 0, []
    for i, pl in enumerate(r):
        extra = (64 - len(r)) // len(r) + (1 if i < (64 - len(r)) % len(r) else 0)
        mix += [pl] + _redundant(extra, k); k += extra
    assert len(mix) == 64
    cases["cell-interleaved-64"] = (mix, "rec")
    cases["cell-last-planes-cut"] = (_redundant(2 * C_REC + 1) + r, "rec")
    # plane 0 removes every vertex of the Mesh (none survives it, none lies in it) but not all of the Convex, whose pair would be
    # skipped otherwise: a direction that is none of the Convex's face normals, just beyond the Mesh's last vertex
    d = np.float32([1, 0.37, 0.23]) / np.float32(np.sqrt(1 + 0.37 ** 2 + 0.23 ** 2))
    top = _dist(np.float32([d[0], d[1], d[2], 0]), pos).max()
    p0 = np.float32([-d[0], -d[1], -d[2], top + np.float32(1e-5)])
    cpos = np.ascontiguousarray(sc["convex"]["pos"], np.float32).reshape(-1, 3)
    assert (_dist(p0, pos) >= tiny).all() and (_dist(p0, cpos) < -np.float32(1e-4)).any()
    # (every vertex has first clipping plane 0, so the pre-pass finds no band and ends the pair itself: no clipper sees it)
    cases["plane0-removes-all"] = ([p0] + real[16], "prepass")
    # a plane through a mesh vertex: plane_dist is exactly 0 there
    r = real[16]
    cutby = np.full(pos.shape[0], len(r), np.int64)
    for i in reversed(range(len(r))):
        cutby[_dist(r[i], pos) >= tiny] = i
    v = int(np.nonzero(cutby == 2)[0][0])                    # first clipped by the cell's plane 2
    u = int(np.nonzero(cutby == len(r))[0][0])               # clipped by none
    for name, w in (("v", v), ("u", u)):
        z = np.float32([1, 0, 0, -pos[w, 0]])
        assert _dist(z, pos[w:w + 1])[0] == 0.0
        _STATE["z" + name] = z
    cases["inplane-before-first-cut"] = ([_STATE["zv"]] + r, "general")       # v lies in plane 0, the list's plane 3 clips it: the 0x80 bit
    cases["inplane-middle-before-first-cut"] = (r[:2] + [_STATE["zv"]] + r[2:], "general")
    cases["inplane-only-candidate"] = (r + [_STATE["zu"]], "general")        # u: no plane clips it, it lies in the last one
    cases["inplane-only-candidate-first"] = ([_STATE["zu"]] + r, "general")
    _STATE["cases"] = cases
    return cases


CASE_NAMES = (["F%d-%s" % (F, p) for F in COUNTS for p in ("front", "end", "middle")
               if not (F == 1 and p != "front") and not (F == 2 and p == "middle")]
              + ["cell-interleaved-64", "cell-last-planes-cut", "plane0-removes-all", "inplane-before-first-cut",
                 "inplane-middle-before-first-cut", "inplane-only-candidate", "inplane-only-candidate-first"])


def _reference(oracle, name):
    key = ("ref", name)
    if key not in _STATE:
        sc, _, _ = _scene(oracle)
        pl = np.asarray(_cases(oracle)[name][0], np.float32)
        _STATE[key] = oracle.event([sc["mesh"]], [sc["convex"]], np.uint32([0, pl.shape[0]]), pl, refit=True, render=True, threads=1, cell_end=1)
    return _STATE[key]


def _run(eng, oracle, name, wave, monkeypatch):
    sc, _, _ = _scene(oracle)
    pl = np.asarray(_cases(oracle)[name][0], np.float32)
    monkeypatch.setenv("SURTR_WAVE", wave)
    eng.upload_planes(np.uint32([0, pl.shape[0]]), pl)
    c = eng.fracture_event(0, 1, flags=3)
    qs = eng.queue_stats()
    ho = eng.handover_stats()
    return c, eng.download(), qs, ho


def _check(eng, oracle, name, monkeypatch):
    pl, route = _cases(oracle)[name]
    ref = _reference(oracle, name)
    out = {}
    for wave in ("1", "0"):
        c, got, qs, ho = _run(eng, oracle, name, wave, monkeypatch)
        took, handed = int(qs[88]), int(qs[89]) + int(qs[94])
        print(name, "F", len(pl), "wave", wave, "fragments", c.n_frag, "took", took, "handed on", int(qs[89]), "to the catcher", int(qs[94]), "pushed", ho["pushed"])
        assert c.status == 0 and c.n_failed == 0 and c.n_frag == ref["frag_ids"].shape[0], (name, wave, c.status, c.n_frag)
        assert_event_equal(got, ref)
        assert np.array_equal(got["mesh_pos"], ref["mesh_pos"]), (name, wave)       # same float program: bit for bit
        if wave == "0":
            assert took == 0 and handed == 0, (name, took, handed)
        elif route == "rec":
            assert took > 0 and handed == 0 and ho["pushed"] == 0, (name, "not taken by the record clipper", took, handed, ho)
        elif route == "general":
            assert took == 0 and handed > 0, (name, "not handed to the general clipper", took, handed, ho)
        else:
            assert took == 0 and handed == 0 and c.n_frag == 0, (name, "the pre-pass did not end the pair", took, handed, ho)
        out[wave] = got
    for k in TOPOLOGY_KEYS + ("mesh_pos", "conv_pos", "vnc"):
        assert np.array_equal(out["1"][k], out["0"][k]), (name, k)


def test_case_list_is_complete(oracle):
    assert sorted(CASE_NAMES) == sorted(_cases(oracle))
    for name, (pl, route) in _cases(oracle).items():
        assert 1 <= len(pl) <= 127


@pytest.fixture(scope="module")
def emul_piece(emul_lib_path, oracle):
    """One engine on the record-clipper emulation build with the piece resident, for every case of the emulation tier."""
    from surtr_amd import engine
    engine._use_library_for_tests(os.path.join(os.path.dirname(emul_lib_path), "libsurtr_emul_rec.so"))
    sc, _, _ = _scene(oracle)
    eng = engine.Engine(0)
    try:
        eng.upload_pieces([sc["mesh"]], [sc["convex"]])
        yield eng
    finally:
        eng.close()
        engine._use_library_for_tests(None)


@pytest.mark.parametrize("name", CASE_NAMES)
def test_plane_loops_emulation(emul_piece, oracle, monkeypatch, name):
    _check(emul_piece, oracle, name, monkeypatch)


@pytest.fixture(scope="module")
def gpu_piece(oracle):
    from surtr_amd import engine
    engine._use_library_for_tests(None)
    assert os.path.exists(engine.lib_path()), "libsurtr_hip.so missing: run __graft_entry__.build()"
    sc, _, _ = _scene(oracle)
    eng = engine.Engine(0)
    try:
        eng.upload_pieces([sc["mesh"]], [sc["convex"]])
        yield eng
    finally:
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
def test_plane_loops_gpu(gpu_piece, oracle, monkeypatch, name):
    _check(gpu_piece, oracle, name, monkeypatch)
