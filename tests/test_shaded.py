"""Lit render buffers (shade_dev.hip): event_shaded / event_shaded_dev against tests/shade_ref.py, the definition of include/surtr_hip.h
restated in Python (a sequential walk of the rings, math.fsum in float64, the common-face rule and the fallback written out).

What compare() demands of an answer, per fragment of the download it belongs to:
  exact    n_faces, first_vertex, n_vertices, status, tri_face; positions (the bytes of Mesh vertex idx[j]) and colours;
  normals  |got - ref64| <= 2^-25 + 2^-30 per component: half a float32 ulp below 1 for the rounding of n to float, and 2^-30 for the
           order of the float64 sum -- shade_ref gives e = k * max_c(sum |T_i|_c) / max_c |N_c| * 2^-52 per face, and compare() REQUIRES
           e <= 2^-30 of every face.  The quotient is 0 / 0 where every term T_i is exactly zero: such a sum is exactly zero in any
           order and shade_ref gives e = 0 (N zero by cancellation of non-zero terms gives e = inf and is refused).  compare() returns
           these faces: among the designed solids they are the two caps of the prism over collinear(12), named, and the test asserts
           that no other designed face is one; the resident scene has one more, a triangle with two corners in one place;
  bits     every vertex of one face carries the same normal bits; a non-zero normal has |n.n - 1| <= 2^-22.
compare() returns what it found wrong, so that the same comparison can be shown to refuse five mutations of a good answer.

Shapes: the smallest at which each route can go wrong (the issue's list), built by tests/faces_ref.py through test_faces_shapes.build,
presented with load_fragments + event_triangulate, each alone and 24 as one batch; on the emulation the batch once more with the global
tier forced (set_shade_tier), which must give the same bytes.  The LDS tier takes fragments of up to LDS_LIMIT = 2048 half-edges: the
pyramid over a 512-gon (H = 2048) is the largest it takes, the roof over it (H = 2050) the smallest it does not; the pyramid and the
roof over a 256-gon (H = 1024, 1026) sit on the limit of the variant the tier was measured against.

The CPU tier runs on the emulation library (conftest's emul_engine); the GPU tier runs the same functions on the MI355X in child
processes under a time limit (helpers.run_gpu_child)."""
import ctypes
import os
import textwrap

import numpy as np
import pytest

import faces_ref as FR
import shade_ref as SR
import test_faces_shapes as FS
import test_scene_fragments as SF
from helpers import fragment, run_gpu_child
from surtr_amd import engine, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
S = engine.SHADED_DTYPE
TOL = 2.0 ** -25 + 2.0 ** -30
SUM_BOUND = 2.0 ** -30
UNIT_TOL = 2.0 ** -22
COLOUR = (0.5, 0.25, 0.125)
LDS_LIMIT = 2048
SIZES = (4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257, 600)
EXTRA = {"pyramid-256": lambda: FR.pyramid_over(FR.regular(256)), "roof-256": lambda: FR.roof_over(FR.regular(256), 128)}
ROUTES = ("pyramid-512", "roof-512", "pyramid-1023-cut", "bipyramid-683", "pyramid-1024", "pyramid-256", "roof-256", "polytope-130",
          "polytope-700", "union")


def names():
    out = []
    for n in SIZES:
        out.append("regular-%d-r0" % n)
        if n % 2 == 0 and n >= 8:
            out += ["star-%d-r0" % n, "pinched-%d-r0" % n]
        if n >= 8:
            out.append("spiral-%d-r0" % n)
    return out + ["collinear-12-r0"] + list(ROUTES)


def build(name):
    return EXTRA[name]() if name in EXTRA else FS.build(name)


BATCH = [n for n in names() if n.endswith("-r0") and 5 <= int(n.split("-")[1]) <= 129 and not n.startswith("collinear")][:17] + \
        ["collinear-12-r0", "pyramid-256", "roof-256", "bipyramid-683", "pyramid-1024", "polytope-700", "union"]


# ------------------------------------------------------------------ the comparison
def compare(ev, rec, vnc, tri, colour):
    """-> (list of what is wrong, [(fragment, face), ...] whose terms are all exactly zero: the faces the quotient e does not exist for)."""
    wrong, loose = [], []
    nf = ev["frag_ids"].shape[0]
    if rec.shape[0] != nf or vnc.shape != (ev["idx"].shape[0], 9) or tri.shape[0] * 3 != ev["idx"].shape[0]:
        return ["shapes %r %r %r" % (rec.shape, vnc.shape, tri.shape)], loose
    for k in range(nf):
        s = fragment(ev, k, "mesh")
        a, b = int(ev["idx_off"][k]), int(ev["idx_off"][k + 1])
        idx = ev["idx"][a:b]
        ref = SR.shade_solid(s["pos"], s["off"], s["nbr"], idx)
        want = (a, b - a, ref["n_faces"], SR.PER_TRIANGLE if ref["per_triangle"] else 0)
        if tuple(int(x) for x in rec[k].tolist()) != want:
            wrong.append("fragment %d: record %r, reference %r" % (k, rec[k].tolist(), want))
        for f, e in enumerate(ref["bound"]):
            if not e <= SUM_BOUND:
                wrong.append("fragment %d face %d: summation bound %g above 2^-30" % (k, f, e))
            elif f in ref["flat"] and len(ref["loops"][f]) >= 3:
                loose.append((k, f))
        if a == b:
            continue
        tf = tri[a // 3:b // 3]
        if not np.array_equal(tf, ref["tri_face"]):
            wrong.append("fragment %d: tri_face differs at %r" % (k, np.nonzero(tf != ref["tri_face"])[0][:4].tolist()))
        v = vnc[a:b]
        if v[:, :3].tobytes() != np.ascontiguousarray(s["pos"][idx], np.float32).tobytes():
            wrong.append("fragment %d: positions" % k)
        if v[:, 6:].tobytes() != np.tile(np.float32(colour), (b - a, 1)).tobytes():
            wrong.append("fragment %d: colours" % k)
        n = v[:, 3:6].astype(np.float64)
        err = np.abs(n - np.repeat(ref["tri_normal"], 3, axis=0))
        if not (err <= TOL).all():
            wrong.append("fragment %d: normal off by %.3g (allowed %.3g) at vertex %d" % (k, err.max(), TOL, int(err.max(1).argmax())))
        nn = (n * n).sum(1)
        if not ((nn == 0) | (np.abs(nn - 1.0) <= UNIT_TOL)).all():
            wrong.append("fragment %d: a normal that is neither zero nor of length one" % k)
        face_of_vertex = np.repeat(tf, 3)
        bits = np.ascontiguousarray(v[:, 3:6]).view(np.uint32)
        for f in np.unique(tf[tf != SR.NO_FACE]):
            rows = bits[face_of_vertex == f]
            if (rows != rows[0]).any():
                wrong.append("fragment %d face %d: its vertices carry different bits" % (k, int(f)))
        for t in np.nonzero(tf == SR.NO_FACE)[0]:
            rows = bits[3 * t:3 * t + 3]
            if (rows != rows[0]).any():
                wrong.append("fragment %d triangle %d: its vertices carry different bits" % (k, int(t)))
    return wrong, loose


def check(eng, colour=COLOUR, flat=None):
    """event_shaded of the current fragments against the reference; the event's own download is the same before and after the call.
    flat: the faces whose terms are all exactly zero, when the case knows them."""
    before = eng.download()
    rec, vnc, tri = eng.event_shaded(colour, tri_face=True)
    after = eng.download()
    for k in before:
        assert np.asarray(before[k]).tobytes() == np.asarray(after[k]).tobytes(), k
    wrong, loose = compare(before, rec, vnc, tri, colour)
    assert not wrong, wrong[:5]
    if flat is not None:
        assert sorted(loose) == sorted(flat), (loose, flat)
    rec2, vnc2, none = eng.event_shaded(colour)                              # twice: the same bits; without tri_face: the same vertices
    assert none is None and rec2.tobytes() == rec.tobytes() and vnc2.tobytes() == vnc.tobytes()
    return before, rec, vnc, tri


def present(eng, solids):
    eng.load_fragments(solids, solids)
    eng.event_triangulate(False)


def collinear_caps(solids, first=0):
    """The faces of a prism over collinear(n) that have n corners: the only faces whose N is exactly zero."""
    out = []
    for k, (name, s) in enumerate(solids):
        if name.startswith("collinear"):
            n = int(name.split("-")[1])
            ref = SR.shade_solid(s["pos"], s["off"], s["nbr"], np.zeros(0, np.uint32))
            caps = [(first + k, f) for f, lp in enumerate(ref["loops"]) if len(lp) == n]
            assert len(caps) == 2
            out += caps
    return out


# ------------------------------------------------------------------ cases
def run_designed(E, emulation):
    eng = E.Engine(0)
    sizes = {}
    for name in names():
        s = build(name)
        sizes[name] = int(s["nbr"].shape[0])
        present(eng, [s])
        ev, rec, vnc, tri = check(eng, flat=collinear_caps([(name, s)]))
        assert ev["mesh_pos"].tobytes() == np.ascontiguousarray(s["pos"], np.float32).tobytes()
        assert rec[0]["status"] == 0 and rec[0]["n_faces"] == len(s["faces"]), name
        if not name.startswith("collinear"):
            assert (tri != SR.NO_FACE).all() and rec[0]["n_vertices"] > 0, name
    # both sides of every limit were there
    assert sizes["pyramid-512"] == LDS_LIMIT and sizes["roof-512"] == LDS_LIMIT + 2 and sizes["pyramid-256"] == 1024 and sizes["roof-256"] == 1026
    assert sizes["pyramid-1023-cut"] == 4096 and sizes["bipyramid-683"] == 4098 and sizes["union"] == 7320
    batch = [(n, build(n)) for n in BATCH]
    assert len(batch) == 24
    present(eng, [s for _, s in batch])
    _, rec, vnc, tri = check(eng, flat=collinear_caps(batch))
    assert (rec["n_vertices"][[n.startswith("collinear") for n, _ in batch]] > 0).all()      # (its walls have triangles, its caps none)
    if emulation:
        for limit in (64, 1):                                                # the global tier forced: the same bytes
            eng.set_shade_tier(limit)
            rec2, vnc2, tri2 = eng.event_shaded(COLOUR, tri_face=True)
            assert rec2.tobytes() == rec.tobytes() and vnc2.tobytes() == vnc.tobytes() and tri2.tobytes() == tri.tobytes()
        eng.set_shade_tier(0)
    eng.close()


def run_events(E):
    g = np.load(os.path.join(GOLDEN, "cube8.npz"))
    sc = scenes.cube_scene(8)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_planes(g["face_off"], g["planes"])
    eng.fracture_event(0, 8, flags=3)
    ev, rec, _, tri = check(eng)
    assert rec.shape[0] == 8 and (rec["n_faces"] >= 4).all() and (tri != SR.NO_FACE).all()
    eng.close()
    sc = scenes.blob_scene(64)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, 64, flags=3)
    ev, rec, _, _ = check(eng)
    assert rec.shape[0] == ev["frag_ids"].shape[0] >= 32
    rec2, vnc2, _ = eng.event_shaded(None)                                    # no colour: the 0.25 grey of surtr_triangulate
    assert (vnc2[:, 6:] == np.float32(0.25)).all()
    eng.close()


def run_scene(E):
    eng, _ = SF.scene_after_click_one(E)
    table = eng.scene_compounds()
    for render_convex in (False, True):
        eng.scene_fragments([5, 2], render_convex=render_convex)
        ev, rec, _, _ = check(eng, flat=[(1, 13)] if render_convex else [])   # (a triangle of that Convex has two corners in one place)
        assert rec.shape[0] == len(SF.pieces_of(table, [5, 2])) >= 2 and (rec["n_vertices"] > 0).all()
    eng.close()


def doubled_ring_solid():
    """A tetrahedron with a fifth vertex wired in by hand so that ring(0) lists vertex 4 twice (and ring(4) lists 0 twice): every link has
    its way back, every ring has three entries or more, and the successor is no permutation."""
    pos = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.25, 0.25, 0.25]])
    rings = [[1, 4, 2, 4, 3], [0, 2, 3], [0, 3, 1], [0, 1, 2], [0, 0, 0]]
    off = np.cumsum([0] + [len(r) for r in rings]).astype(np.uint32)
    return {"pos": pos, "off": off, "nbr": np.int32([x for r in rings for x in r])}


def run_fallback(E):
    """The whole-fragment fallback, between two regular solids of one batch: flagged, no faces, per-triangle normals."""
    eng = E.Engine(0)
    cube = FR.prism_over(FR.regular(4))
    d = np.load(os.path.join(GOLDEN, "degenerate_sliver_convex.npz"))
    cands = [doubled_ring_solid()] + [{"pos": d[p + "_pos"], "off": d[p + "_off"], "nbr": d[p + "_nbr"]} for p in ("mesh", "conv") if p + "_pos" in d.files]
    done = 0
    for bad in cands:
        if SR.successor(bad["off"], bad["nbr"], np.asarray(bad["pos"]).reshape(-1, 3).shape[0]) is not None:
            continue
        try:
            eng.load_fragments([cube, bad, cube], [cube, cube, cube])
        except engine.SurtrError:
            continue                                                         # (surtr_load_fragments vets what it is given)
        eng.event_triangulate(False)
        ev, rec, vnc, tri = check(eng)
        assert rec[1]["status"] == engine.SHADE_PER_TRIANGLE and rec[1]["n_faces"] == 0 and rec[0]["status"] == 0 == rec[2]["status"]
        a, b = int(rec[1]["first_vertex"]), int(rec[1]["first_vertex"] + rec[1]["n_vertices"])
        assert (tri[a // 3:b // 3] == SR.NO_FACE).all()
        done += 1
    eng.close()
    return done


def dev_buffers(torch, sizes):
    """-> 'device' byte buffers filled with 0xAB, their addresses, and a function that reads them back (the emulation's device memory is
    host memory)."""
    if torch is None:
        bufs = [np.full(max(b, 1), 0xAB, np.uint8) for b in sizes]
        return bufs, [b.ctypes.data for b in bufs], lambda: [b.copy() for b in bufs]
    bufs = [torch.full((max(b, 1),), 0xAB, dtype=torch.uint8, device="cuda") for b in sizes]
    torch.cuda.synchronize()
    return bufs, [b.data_ptr() for b in bufs], lambda: [b.cpu().numpy() for b in bufs]


GUARD = 256


def unpack(raw, n, nv):
    return raw[0][:16].view(S)[0], raw[0][16:16 * (n + 1)].view(S), raw[1][:36 * nv].view(np.float32).reshape(-1, 9), raw[2][:4 * (nv // 3)].view(np.uint32)


def run_errors(E, torch=None):
    L = E.lib()
    bare = E.Engine(0)
    _, ptrs, read = dev_buffers(torch, (16 * 8, 36 * 64, 4 * 64))
    with pytest.raises(engine.SurtrError) as e:
        bare.event_shaded()
    assert e.value.code == engine.E_STATE                                    # no current fragments
    with pytest.raises(engine.SurtrError) as e:
        bare.event_shaded_dev(ptrs[0], 16 * 8, ptrs[1], 64, ptrs[2], 64)
    assert e.value.code == engine.E_STATE
    cube = FR.prism_over(FR.regular(5))
    bare.load_fragments([cube], [cube])
    for call in (bare.event_shaded, lambda: bare.event_shaded_dev(ptrs[0], 16 * 8, ptrs[1], 64, ptrs[2], 64)):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == engine.E_STATE                                # never triangulated
    assert all((b == 0xAB).all() for b in read())
    bare.event_triangulate(False)
    check(bare)                                                              # the context is still usable
    # after a failed event (an arena too small for its fragments)
    sc = scenes.blob_scene(64)
    bare.set_arena(64, 256, 256)
    bare.upload_pieces([sc["mesh"]], [sc["convex"]])
    bare.upload_pattern(sc["face_off"], sc["v012"])
    bare.place_cells(sc["scale"], sc["translate"])
    with pytest.raises(engine.SurtrError) as e:
        bare.fracture_event(0, 64)
    assert e.value.code == engine.E_CAPACITY
    for call in (bare.event_shaded, lambda: bare.event_shaded_dev(ptrs[0], 16 * 8, ptrs[1], 64, ptrs[2], 64)):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == engine.E_STATE
    assert all((b == 0xAB).all() for b in read())
    bare.close()

    eng = E.Engine(0)
    solids = [build(n) for n in ("regular-5-r0", "star-64-r0", "pyramid-256", "roof-256")]
    present(eng, solids)
    ev, want_rec, want_vnc, want_tri = check(eng)                            # (the download leaves the counts with the host)
    n, nv = want_rec.shape[0], want_vnc.shape[0]
    fn = L.surtr_event_shaded
    rec, vnc, tri = np.zeros(n, S), np.zeros((nv, 9), np.float32), np.zeros(nv // 3, np.uint32)
    c = [ctypes.c_uint32(n), ctypes.c_uint32(nv), ctypes.c_uint32(0)]
    P = engine._p
    assert fn(None, None, ctypes.byref(c[0]), None, ctypes.byref(c[1]), None, None, None) == engine.E_INVALID
    assert fn(eng._h, None, None, None, ctypes.byref(c[1]), None, None, None) == engine.E_INVALID
    assert fn(eng._h, None, ctypes.byref(c[0]), P(rec), ctypes.byref(c[1]), None, None, None) == engine.E_INVALID
    assert fn(eng._h, None, ctypes.byref(c[0]), None, ctypes.byref(c[1]), P(vnc), None, None) == engine.E_INVALID
    assert fn(eng._h, None, ctypes.byref(c[0]), None, ctypes.byref(c[1]), None, P(tri), None) == engine.E_INVALID
    for short in range(2):                                                   # each count one too small: the counts come back, nothing is written
        c = [ctypes.c_uint32(n), ctypes.c_uint32(nv), ctypes.c_uint32(0)]
        c[short].value -= 1
        assert fn(eng._h, None, ctypes.byref(c[0]), P(rec), ctypes.byref(c[1]), P(vnc), P(tri), ctypes.byref(c[2])) == engine.E_CAPACITY
        assert [c[0].value, c[1].value] == [n, nv] and not rec["n_vertices"].any() and not vnc.any() and not tri.any()
    sizes = (16 * (n + 1) + GUARD, 36 * nv + GUARD, 4 * (nv // 3) + GUARD)
    _, ptrs, read = dev_buffers(torch, sizes)
    for args in ((0, 16 * (n + 1), ptrs[1], nv, ptrs[2], nv // 3), (ptrs[0], 16 * (n + 1), 0, nv, ptrs[2], nv // 3), (ptrs[0], 16 * (n + 1), ptrs[1], 0, ptrs[2], nv // 3),
                 (ptrs[0], 16 * (n + 1), ptrs[1], nv, 0, nv // 3), (ptrs[0], 16 * (n + 1), ptrs[1], nv, ptrs[2], 0)):
        with pytest.raises(engine.SurtrError) as e:
            eng.event_shaded_dev(*args, color=COLOUR)
        assert e.value.code == engine.E_INVALID
    # the host holds the counts: anything one short is refused before anything is enqueued
    for args in ((ptrs[0], 15, ptrs[1], nv, ptrs[2], nv // 3), (ptrs[0], 16 * n + 15, ptrs[1], nv, ptrs[2], nv // 3), (ptrs[0], 16 * (n + 1), ptrs[1], nv - 1, ptrs[2], nv // 3),
                 (ptrs[0], 16 * (n + 1), ptrs[1], nv, ptrs[2], nv // 3 - 1)):
        with pytest.raises(engine.SurtrError) as e:
            eng.event_shaded_dev(*args, color=COLOUR)
        assert e.value.code == engine.E_CAPACITY
    assert all((b == 0xAB).all() for b in read())

    def exact_fit(with_tri):
        _, ptrs, read = dev_buffers(torch, sizes)
        eng.event_shaded_dev(ptrs[0], 16 * (n + 1), ptrs[1], nv, ptrs[2] if with_tri else 0, nv // 3 if with_tri else 0, color=COLOUR)
        raw = read()
        hdr, rec, vnc, tri = unpack(raw, n, nv)
        assert tuple(hdr.tolist()) == (n, nv, int(want_rec["n_faces"].sum()), 0)
        assert rec.tobytes() == want_rec.tobytes() and vnc.tobytes() == want_vnc.tobytes()
        assert tri.tobytes() == want_tri.tobytes() if with_tri else (raw[2] == 0xAB).all()
        assert (raw[0][16 * (n + 1):] == 0xAB).all() and (raw[1][36 * nv:] == 0xAB).all() and (raw[2][4 * (nv // 3):] == 0xAB).all()      # the guard words
    exact_fit(True)
    exact_fit(False)
    # only the device knows the counts (nothing has read them since the triangulation): the header says what is needed, nothing else is written
    present(eng, solids)
    for args in ((16 * (n + 1), nv - 1, nv // 3), (16 * (n + 1), nv, nv // 3 - 1), (16 * n, nv, nv // 3)):
        _, ptrs, read = dev_buffers(torch, sizes)
        eng.event_shaded_dev(ptrs[0], args[0], ptrs[1], args[1], ptrs[2], args[2], color=COLOUR)
        raw = read()
        assert tuple(raw[0][:16].view(S)[0].tolist()) == (n, nv, int(want_rec["n_faces"].sum()), engine.E_CAPACITY)
        assert (raw[0][16:] == 0xAB).all() and (raw[1] == 0xAB).all() and (raw[2] == 0xAB).all()
    exact_fit(True)                                                          # (still without the counts on the host)
    check(eng)
    eng.close()


def run_mutations(E):
    """The comparison has teeth: it accepts the engine's answer and refuses each of five mutations of it."""
    eng = E.Engine(0)
    present(eng, [build("regular-5-r0"), build("star-64-r0")])
    ev, rec, vnc, tri = check(eng)
    eng.close()
    assert compare(ev, rec, vnc, tri, COLOUR) == ([], [])
    face = np.repeat(tri, 3)
    first = int(rec[1]["first_vertex"])
    f0, f1 = int(tri[first // 3]), int(tri[first // 3 + 1] if tri[first // 3 + 1] != tri[first // 3] else tri[-1])
    in1 = np.arange(vnc.shape[0]) >= first
    assert f0 != f1

    def mutated(fn):
        r, v, t = rec.copy(), vnc.copy(), tri.copy()
        fn(r, v, t)
        return compare(ev, r, v, t, COLOUR)[0]

    def negate(r, v, t):
        v[in1 & (face == f0), 3:6] *= -1

    def neighbour(r, v, t):
        v[in1 & (face == f0), 3:6] = v[in1 & (face == f1)][0, 3:6]

    def off_by_one(r, v, t):
        t[first // 3] += 1

    def unnormalised(r, v, t):
        v[in1 & (face == f0), 3:6] *= np.float32(1.0009765625)

    def swapped(r, v, t):
        v[[first, first + 1], :3] = v[[first + 1, first], :3]

    assert (vnc[in1 & (face == f0)][0, 3:6] != vnc[in1 & (face == f1)][0, 3:6]).any()
    for fn in (negate, neighbour, off_by_one, unnormalised, swapped):
        assert mutated(fn), fn.__name__


# ------------------------------------------------------------------ CPU tier (emulation)
def test_designed_solids_alone_and_as_a_batch(emul_engine):
    run_designed(emul_engine, True)


def test_events_cube8_and_blob64(emul_engine):
    run_events(emul_engine)


def test_scene_fragments_both_render_routes(emul_engine):
    run_scene(emul_engine)


def test_whole_fragment_fallback(emul_engine):
    assert run_fallback(emul_engine) >= 1


def test_errors_capacities_and_guard_words(emul_engine):
    run_errors(emul_engine)


def test_the_comparison_refuses_five_mutations(emul_engine):
    run_mutations(emul_engine)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_shaded as T
    case = sys.argv[1]
    if case == "errors":
        T.run_errors(engine, torch)
    elif case == "streams":
        T.run_streams(engine, torch)
    elif case == "designed":
        T.run_designed(engine, False)
    elif case == "fallback":
        assert T.run_fallback(engine) >= 1
    else:
        getattr(T, "run_" + case)(engine)
    print("ok", case)
""")


def run_streams(E, torch):
    """The _dev form on a second stream, queued twice beside a running event of another context, with the in-flight hint at 6: the same
    bytes as the host form."""
    eng = E.Engine(0)
    solids = [build(n) for n in ("spiral-129-r0", "pyramid-256", "roof-256", "polytope-130", "union")]
    present(eng, solids)
    _, want_rec, want_vnc, want_tri = check(eng)
    n, nv = want_rec.shape[0], want_vnc.shape[0]
    sc = scenes.blob_scene(64)
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    other = E.Engine(0, stream=s1.cuda_stream)
    other.set_events_in_flight(6)
    other.upload_pieces([sc["mesh"]], [sc["convex"]])
    other.upload_pattern(sc["face_off"], sc["v012"])
    other.place_cells(sc["scale"], sc["translate"])
    eng.set_stream(s2.cuda_stream)
    eng.set_events_in_flight(6)
    present(eng, solids)                                                     # (on the new stream; the host does not hold the counts)
    sizes = (16 * (n + 1), 36 * nv, 4 * (nv // 3))
    sets = [dev_buffers(torch, sizes) for _ in range(2)]
    other.fracture_event_async(0, 64)
    for _, ptrs, _ in sets:
        eng.event_shaded_dev(ptrs[0], sizes[0], ptrs[1], nv, ptrs[2], nv // 3, color=COLOUR)
    s2.synchronize()
    assert other.event_counts().n_frag >= 32
    for _, _, read in sets:
        hdr, rec, vnc, tri = unpack(read(), n, nv)
        assert hdr["status"] == 0
        assert rec.tobytes() == want_rec.tobytes() and vnc.tobytes() == want_vnc.tobytes() and tri.tobytes() == want_tri.tobytes()
    other.close()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["designed", "events", "scene", "fallback", "errors", "mutations", "streams"])
def test_gpu_shaded(case):
    run_gpu_child(GPU_CHILD, case, 120)
