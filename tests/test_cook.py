"""Cooked hulls (cook_dev.hip): event_cook / pieces_cook / cook_points and the _dev forms.

NO REFERENCE RUNS THE NEW CODE.  Every answer goes through cook_ref.check_solid -- float64 numpy written from the definition of
include/surtr_hip.h, which builds no hull of its own -- and, for point sets in general position, the hull's vertex set is compared with
Qhull's (scipy on the CPU tier, where the general-position gap of the sets is asserted on Qhull's answer first; the GPU tier reads the
committed tests/golden/cook_random_vertices.npz, which the CPU tier compares with scipy's answer).  On the emulation planes and errors
are byte for byte the float64 restatement; on the MI355X a plane component may differ by one float32 ulp (tests/test_hulls.py says why).

Bounds (cook_ref has them in full): planarity <= plane_tol + s_f per face, every INPUT point at most 2 plane_tol + weld_dist + s_f in front
of every plane, s_f the rounding of the written plane.  weld_dist is 0 in every case but one, where the welded points lie 1e-4 away from
the kept ones by design.

The CPU tier runs on the emulation library; the GPU tier runs the same functions on the MI355X, one child process per case."""
import ctypes
import os
import textwrap

import numpy as np
import pytest

import cook_ref as CR
import faces_ref as FR
import regroup_ref as RR
import test_hulls as TH
import test_scene as TS
import test_scene_fragments as SF
from helpers import run_gpu_child
from surtr_amd import engine, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
C, P = engine.COOK_DTYPE, engine.POLY_DTYPE
F32 = np.float32
TOL = 7e-6


def check_all(got, inputs, weld, tol, exact, cooked=None):
    """Every solid of one answer: the cooked ones through the checker, the others hand nothing out; the offsets are the exclusive sums."""
    rec = got["records"]
    assert rec.dtype == C and got["polygons"].dtype == P and got["idx"].dtype == np.uint16 and got["points"].dtype == F32 and got["src"].dtype == np.uint32
    assert rec.shape[0] == len(inputs)
    for name, cnt in (("pt_off", "nv"), ("face_off", "n_faces"), ("idx_off", "n_idx")):
        assert np.array_equal(rec[name], np.concatenate([[0], np.cumsum(rec[cnt])[:-1]]).astype(np.uint32)), name
    assert got["points"].shape[0] == int(rec["nv"].sum()) == got["src"].shape[0]
    assert got["polygons"].shape[0] == int(rec["n_faces"].sum()) and got["idx"].shape[0] == int(rec["n_idx"].sum())
    for k, pts in enumerate(inputs):
        if cooked is not None and k not in cooked:
            assert rec[k]["status"] == CR.SKIPPED, (k, rec[k])
        if int(rec[k]["status"]) & CR.WITHHELD:
            CR.check_withheld(rec[k], np.asarray(pts).reshape(-1, 3).shape[0])
        else:
            CR.check_solid(pts, CR.solid_of(got, k), weld, tol, exact)


# ------------------------------------------------------------------ designed solids
def golden_convex(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {"pos": d["conv_pos"], "off": d["conv_off"], "nbr": d["conv_nbr"]}


def cube_points():
    return F32([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)])


def cube_with_extras():
    """The corners, the origin (second, so that a hull vertex follows it), the 6 face centres, the 12 edge midpoints, a corner again."""
    c = cube_points()
    grid = F32([[x, y, z] for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)])
    zeros = (grid == 0).sum(1)
    return np.concatenate([c[:1], F32([[0, 0, 0]]), c[1:], grid[zeros == 2], grid[zeros == 1], c[5:6]]).astype(F32)


def convex_solids():
    """[(name, solid with rings)]: what load_fragments / upload_pieces take."""
    return ([("tetrahedron", FR.pyramid_over(FR.regular(3))), ("cube", RR.box((-1, -1, -1), (1, 1, 1)))] +
            [("prism %d" % n, FR.prism_over(FR.regular(n))) for n in (63, 64, 65)] + [("prism 300", FR.prism_over(FR.regular(300)))] +
            [("polytope %d" % n, FR.tangent_polytope(n)) for n in (34, 35)] +
            [(n, golden_convex(n)) for n in ("degenerate_sliver_convex", "sliver_convex_walk_bound", "pinched_face_fragment")])


def degenerate_sets():
    r = np.random.default_rng(7)
    flat = np.concatenate([r.random((10, 2)), np.full((10, 1), 0.25)], 1)
    line = np.outer(np.linspace(-1.0, 1.0, 10), [0.5, 0.25, 1.0])
    same = np.tile(F32([[0.3, -0.2, 0.9]]), (10, 1))
    nan = np.concatenate([cube_points(), F32([[0.0, np.nan, 0.0]])])
    return [("ten coplanar", F32(flat), CR.DEGENERATE), ("ten collinear", F32(line), CR.DEGENERATE), ("ten equal", same, CR.FEW), ("a NaN", nan, CR.NONFINITE)]


def expect(rec, **kw):
    for k, v in kw.items():
        assert int(rec[k]) == v, (k, int(rec[k]), v, rec)


def run_designed(E, exact):
    eng = E.Engine(0)
    maxv = engine.cook_max_vertices()
    assert maxv >= 256
    solids = convex_solids()
    pts = {n: np.ascontiguousarray(s["pos"], F32).reshape(-1, 3) for n, s in solids}
    assert [pts["prism %d" % n].shape[0] for n in (63, 64, 65, 300)] == [126, 128, 130, 600]
    alone = {}
    for name, p in pts.items():
        g = eng.cook_points([p], 0.0, TOL)
        check_all(g, [p], 0.0, TOL, exact)
        alone[name] = CR.solid_bytes(g, 0)
        r = g["records"][0]
        if name == "tetrahedron":
            expect(r, status=0, nv=4, n_faces=4, n_idx=12, max_loop=3, n_welded=0)
        elif name == "cube":
            expect(r, status=0, nv=8, n_faces=6, n_idx=24, max_loop=4, n_welded=0)
        elif name in ("prism 63", "prism 64", "prism 65"):
            n = int(name.split()[1])
            expect(r, status=0, nv=2 * n, n_faces=n + 2, n_idx=6 * n, max_loop=n, n_welded=0)
        elif name == "prism 300":
            if maxv >= 600:
                expect(r, status=CR.OVER_255, nv=600, n_faces=302, max_loop=300)
            else:
                expect(r, status=CR.LARGE)
        elif name in ("degenerate_sliver_convex", "sliver_convex_walk_bound"):
            # flat solids: every point within 4e-8 of one plane (the smallest singular value of the centred points bounds it), far
            # under plane_tol, so no start simplex exists; asserted on the points first
            assert np.linalg.svd(p.astype(np.float64) - p.astype(np.float64).mean(0), compute_uv=False)[2] < 4e-8 < TOL
            expect(r, status=CR.DEGENERATE)
        else:
            assert not int(r["status"]) & CR.WITHHELD, (name, r)         # solids with a volume: Qhull builds a hull of every one
    # the cube where coplanarity is exact: plane_tol 0
    g = eng.cook_points([cube_points()], 0.0, 0.0)
    check_all(g, [cube_points()], 0.0, 0.0, exact)
    expect(g["records"][0], status=0, nv=8, n_faces=6, max_loop=4)
    assert g["records"][0]["convexity"] == 0 and g["records"][0]["planarity"] == 0
    # ... with its face centres, edge midpoints, the origin and a corner twice
    extra = cube_with_extras()
    assert extra.shape[0] == 28
    g = eng.cook_points([extra], 0.0, TOL)
    check_all(g, [extra], 0.0, TOL, exact)
    expect(g["records"][0], status=0, nv_in=28, nv=8, n_faces=6, max_loop=4, n_welded=1)
    assert sorted(g["src"].tolist()) == [0, 2, 3, 4, 5, 6, 7, 8]
    # two clusters 1e-4 apart at weld_dist 1e-3: the second copy of every corner goes
    twice = np.concatenate([cube_points(), cube_points() + F32([1e-4, 0, 0])]).astype(F32)
    g = eng.cook_points([twice], 1e-3, TOL)
    check_all(g, [twice], 1e-3, TOL, exact)
    expect(g["records"][0], status=0, nv=8, n_faces=6, n_welded=8)
    assert g["src"].tolist() == list(range(8))
    g = eng.cook_points([twice], 0.0, TOL)                              # without the weld all sixteen are hull vertices or lie in a face
    check_all(g, [twice], 0.0, TOL, exact)
    expect(g["records"][0], n_welded=0)
    # degenerate input
    for name, p, status in degenerate_sets():
        g = eng.cook_points([p], 0.0, TOL)
        check_all(g, [p], 0.0, TOL, exact)
        expect(g["records"][0], status=status)
        alone[name] = CR.solid_bytes(g, 0)
        pts[name] = p
    # one batch with the withheld ones in the middle, then reversed: the same bytes per solid
    names = [n for n, _ in solids]
    order = names[:4] + [n for n, _, _ in degenerate_sets()] + names[4:]
    for batch in (order, order[::-1]):
        g = eng.cook_points([pts[n] for n in batch], 0.0, TOL)
        check_all(g, [pts[n] for n in batch], 0.0, TOL, exact)
        for k, n in enumerate(batch):
            assert CR.solid_bytes(g, k) == alone[n], n
    # the same solids as the Convex of fragments and as resident pieces
    for batch in (names, names[::-1]):
        ss = [dict(solids)[n] for n in batch]
        eng.load_fragments(ss, ss)
        g = eng.event_cook(None, 1e-5, 0.0, TOL)
        eng2 = E.Engine(0)
        eng2.upload_pieces(ss, ss)
        res = eng2.pieces_cook(None, 1e-5, 0.0, TOL)
        eng2.close()
        for k, n in enumerate(batch):
            assert CR.solid_bytes(g, k) == alone[n], n
        for key in ("records", "points", "src", "polygons", "idx"):
            assert res[key].tobytes() == g[key].tobytes(), key
    eng.close()


# ------------------------------------------------------------------ thin solids: what the ring hulls fail on
def thin_sets():
    """Solids 3 to 40 plane_tol thick, where the merge has the most to get wrong: unit-sphere points and box clouds squeezed to a
    thickness t in [2e-5, 3e-4], two parallel planes 1e-3 apart with 5e-6 noise, spheres of extent 1e-4.  None is degenerate: the
    thinnest is about three plane_tol thick, so every one must be cooked, with status 0, and pass the checker."""
    out = []
    for seed in range(8):
        r = np.random.default_rng(seed)
        t = 10 ** r.uniform(np.log10(2e-5), np.log10(3e-4))
        n = int(r.integers(12, 120))
        p = r.standard_normal((n, 3))
        p /= np.linalg.norm(p, axis=1)[:, None]
        q = r.random((n, 3))
        q[:, 2] = r.integers(0, 2, n) * 1e-3 + r.normal(0, 5e-6, n)
        out += [("sphere x %.3g" % t, F32(p * [1, 1, t])), ("box x %.3g" % t, F32(r.random((n, 3)) * [1, 1, t])), ("two planes", F32(q)),
                ("sphere of 1e-4", F32(p * 5e-5))]
    return out


def run_thin(E, exact):
    eng = E.Engine(0)
    sets = thin_sets()
    g = eng.cook_points([p for _, p in sets], 0.0, TOL)
    assert not g["records"]["status"].any(), [(n, int(s)) for (n, _), s in zip(sets, g["records"]["status"]) if s]
    check_all(g, [p for _, p in sets], 0.0, TOL, exact)
    assert all(engine.cooked_usable(r, TOL) for r in g["records"])
    assert int((g["records"]["n_faces"] < 2 * g["records"]["nv"] - 4).sum()) >= 16      # (the merge is at work on them)
    eng.close()


# ------------------------------------------------------------------ the checker refuses wrong answers
def run_mutations(E):
    eng = E.Engine(0)
    extra = np.concatenate([cube_with_extras(), F32([[1.5, 0.25, 0.125]])])      # (a vertex on four triangles besides the cube's)
    ans = CR.solid_of(eng.cook_points([extra], 0.0, TOL), 0)
    eng.close()
    CR.check_solid(extra, ans, 0.0, TOL, True)
    assert max(map(len, ans["loops"])) >= 4
    muts = CR.mutations(extra, ans, TOL)
    assert len(muts) == 7
    for name, wrong, reason in muts:
        with pytest.raises(CR.Refused) as e:
            CR.check_solid(extra, wrong, 0.0, TOL, True)
        print(name, "->", e.value)
        assert e.value.reason == reason, (name, e.value.reason, reason)


# ------------------------------------------------------------------ general position against Qhull
RANDOM = [(kind, n) for kind in ("sphere", "ball") for n in (4, 5, 8, 33, 64, 65, 130, 300)]


def random_set(kind, n):
    r = np.random.default_rng(1000 + n)
    p = r.standard_normal((n, 3))
    p /= np.linalg.norm(p, axis=1)[:, None]
    if kind == "ball":
        p *= r.random((n, 1)) ** (1 / 3)
    return (p * [1.0, 0.6, 0.35]).astype(np.float32)


def golden_vertices():
    d = np.load(os.path.join(GOLDEN, "cook_random_vertices.npz"))
    return {(kind, n): d["%s_%d" % (kind, n)] for kind, n in RANDOM}


def qhull_vertices():
    """Qhull's answer for the sixteen sets, after the general-position gap is asserted on it: 2 V - 4 triangles, and no point that is
    not a triangle's own vertex within 1e-9 * extent of its plane."""
    from scipy.spatial import ConvexHull
    out = {}
    for kind, n in RANDOM:
        p = random_set(kind, n).astype(np.float64)
        h = ConvexHull(p)
        assert h.simplices.shape[0] == 2 * h.vertices.shape[0] - 4
        d = np.abs(h.equations[:, :3] @ p.T + h.equations[:, 3:4])
        for f, tri in enumerate(h.simplices):
            d[f, tri] = np.inf
        ext = (p.max(0) - p.min(0)).max()
        assert d.min() > 1e-9 * ext, (kind, n, d.min() / ext)
        out[(kind, n)] = np.sort(h.vertices).astype(np.uint32)
    return out


def run_random(E, exact):
    want = golden_vertices()
    assert max(len(want[("sphere", n)]) for _, n in RANDOM) == 300 <= engine.cook_max_vertices()
    eng = E.Engine(0)
    sets = [random_set(kind, n) for kind, n in RANDOM]
    g = eng.cook_points(sets, 0.0, 0.0)
    check_all(g, sets, 0.0, 0.0, exact)
    for k, key in enumerate(RANDOM):
        s = CR.solid_of(g, k)
        assert np.array_equal(s["src"], want[key]), key
        assert len(s["loops"]) == 2 * len(want[key]) - 4 and all(len(lp) == 3 for lp in s["loops"]), key
    g = eng.cook_points(sets, 0.0, TOL)                                 # at 7e-6 only the checker applies
    check_all(g, sets, 0.0, TOL, exact)
    assert not (g["records"]["status"] & CR.WITHHELD).any()
    eng.close()


# ------------------------------------------------------------------ the scene
def convexes_of(eng, pieces):
    return [eng.download_piece(p, 1) for p in pieces]


def positions(solids):
    return [np.ascontiguousarray(s["pos"], F32).reshape(-1, 3) for s in solids]


def same_bytes(a, b):
    for k in ("records", "points", "src", "polygons", "idx"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def cook_everything(eng, solids, exact, flat_allowed=False):
    """Every solid cooked (no hull records).  No solid may come back FAILED or LARGE (or FEW, NONFINITE, SKIPPED); DEGENERATE only where
    flat_allowed and the checker itself finds the points flat: within 2 plane_tol of one plane (cook_ref.check_flat says why 2)."""
    g = eng.event_cook(None, 1e-5, 0.0, TOL)
    pts = positions(solids)
    check_all(g, pts, 0.0, TOL, exact)
    st = g["records"]["status"]
    assert not (st & (CR.WITHHELD & ~CR.DEGENERATE)).any(), st
    flat = np.nonzero(st & CR.DEGENERATE)[0]
    assert flat_allowed or flat.shape[0] == 0, st
    for k in flat:
        print("solid %d of %d points is flat: width %.3g" % (k, pts[k].shape[0], CR.check_flat(pts[k], TOL)))
    assert all(engine.cooked_usable(r, TOL) for r in g["records"] if not r["status"] & CR.WITHHELD)
    return g


def cook_selected(eng, solids, exact, expect=None):
    """The selection on the device from the records event_hulls gives for the fragments the context holds now: exactly the solids
    hull_usable refuses are cooked, each with the bytes it has when every solid is cooked."""
    hl = eng.event_hulls()
    refused = [k for k, r in enumerate(hl["records"]) if not engine.hull_usable(r, 1e-5)]
    assert expect is None or refused == expect, (refused, expect)
    sel, everything = eng.event_cook(hl["records"], 1e-5, 0.0, TOL), eng.event_cook(None, 1e-5, 0.0, TOL)
    check_all(sel, positions(solids), 0.0, TOL, exact, cooked=refused)
    for k in range(len(solids)):
        assert bool(int(sel["records"][k]["status"]) & CR.SKIPPED) == (k not in refused)
        if k in refused:
            assert CR.solid_bytes(sel, k) == CR.solid_bytes(everything, k)
    return refused


def run_scene(E, exact):
    eng, world = SF.scene_after_click_one(E)
    solids = convexes_of(eng, range(10))
    eng.scene_fragments(None)
    # the selection, on the reference's records first: exactly pieces 2 and 9 are refused
    refs = [TH.ref_hull(s) for s in solids]
    refused = [k for k, r in enumerate(refs) if not engine.hull_usable(dict(status=r["status"], extent=r["extent"], convexity=r["convexity"], planarity=r["planarity"]), 1e-5)]
    assert refused == [2, 9]
    hl = eng.event_hulls()
    assert [k for k, r in enumerate(hl["records"]) if not engine.hull_usable(r, 1e-5)] == [2, 9]
    got = eng.event_cook(hl["records"], 1e-5, 0.0, TOL)
    check_all(got, positions(solids), 0.0, TOL, exact, cooked=(2, 9))
    rec = got["records"]
    assert [int(s) & CR.WITHHELD for s in rec["status"]] == [CR.SKIPPED if k not in (2, 9) else 0 for k in range(10)]
    assert engine.cooked_usable(rec[2], TOL) and engine.cooked_usable(rec[9], TOL) and not engine.cooked_usable(rec[0], TOL)
    assert solids[2]["pos"].shape[0] == 24 and rec[2]["n_welded"] == 1
    same_bytes(eng.pieces_cook(eng.pieces_hulls()["records"], 1e-5, 0.0, TOL), got)
    # every solid
    everything = cook_everything(eng, solids, exact)
    same_bytes(eng.pieces_cook(None, 1e-5, 0.0, TOL), everything)
    for k in (2, 9):
        assert CR.solid_bytes(everything, k) == CR.solid_bytes(got, k)
    # a list of compounds, in the order given
    eng.scene_fragments([5, 2, 0])
    ids = SF.pieces_of(SF.TABLE, [5, 2, 0])
    cook_everything(eng, [solids[p] for _, p in ids], exact)
    cook_selected(eng, [solids[p] for _, p in ids], exact, expect=[k for k, (_, p) in enumerate(ids) if p in (2, 9)])
    # after a refit: the Convex the context holds now
    eng.event_refit()
    _, refitted = scenes.fragments_as_pieces(eng.download())
    cook_everything(eng, refitted, exact)
    cook_selected(eng, refitted, exact)
    # after a second commit, on the compounds it made
    n, first, n_new, src, _ = TS.click_two(E, eng, world, 2)
    table = eng.scene_compounds()
    made = list(range(first, first + n_new))
    ids = SF.pieces_of(table, made)
    eng.scene_fragments(made)
    made_solids = convexes_of(eng, [p for _, p in ids])
    # (three of these pieces are slivers thinner than 2e-6, under plane_tol: DEGENERATE by the definition, and the checker agrees)
    cook_everything(eng, made_solids, exact, flat_allowed=True)
    hl = eng.event_hulls()
    sel = eng.event_cook(hl["records"], 1e-5, 0.0, TOL)
    cooked = [k for k, r in enumerate(hl["records"]) if not engine.hull_usable(r, 1e-5)]
    check_all(sel, positions(made_solids), 0.0, TOL, exact, cooked=cooked)
    assert not (sel["records"]["status"] & (CR.FAILED | CR.LARGE)).any()
    eng.close()


# ------------------------------------------------------------------ errors, capacity and state
SIZES = (64, 12, 4, 20, 2)      # bytes per record, point, src entry, polygon, index


def dev_buffers(torch, counts):
    """-> five 'device' byte buffers (records with the header, points, src, polygons, indices) filled with 0xAB, their addresses and a
    function that reads them back (the emulation's device memory is host memory)."""
    sizes = [max(c * b, 1) for c, b in zip(counts, SIZES)]
    if torch is None:
        bufs = [np.full(b, 0xAB, np.uint8) for b in sizes]
        return bufs, [b.ctypes.data for b in bufs], lambda: [b.copy() for b in bufs]
    bufs = [torch.full((b,), 0xAB, dtype=torch.uint8, device="cuda") for b in sizes]
    torch.cuda.synchronize()
    return bufs, [b.data_ptr() for b in bufs], lambda: [b.cpu().numpy() for b in bufs]


def unpack_dev(raw, n):
    hdr = raw[0][:64].view(C)[0]
    nv, nf, ni = int(hdr["nv"]), int(hdr["n_faces"]), int(hdr["n_idx"])
    return hdr, {"records": raw[0][64:64 * (n + 1)].view(C), "points": raw[1][:12 * nv].view(F32).reshape(-1, 3), "src": raw[2][:4 * nv].view(np.uint32),
                 "polygons": raw[3][:20 * nf].view(P), "idx": raw[4][:2 * ni].view(np.uint16)}


def hull_buffer(torch, eng, dev_call, n, npoly, nidx):
    """The buffer a _hulls_dev call writes (header + records), left on the 'device'."""
    (rec, poly, idx), ptrs, _ = TH.dev_buffers(engine, torch, 48 * (n + 1), npoly, nidx)
    dev_call(ptrs[0], 48 * (n + 1), ptrs[1], npoly, ptrs[2], nidx)
    return (rec, poly, idx), ptrs[0]


def cube8_event(E):
    """The arena is left sound: the fixture's event right after."""
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
    eng.close()


def dev_args(ptrs, counts, hulls=0, rel_tol=1e-5, weld=0.0, tol=TOL):
    return (hulls, rel_tol, weld, tol, ptrs[0], 64 * counts[0], ptrs[1], counts[1], ptrs[2], ptrs[3], counts[2], ptrs[4], counts[3])


def run_errors(E, exact, torch=None):
    L = E.lib()
    bare = E.Engine(0)
    _, ptrs, read = dev_buffers(torch, (4, 64, 64, 64, 256))
    for host, dev in ((bare.event_cook, bare.event_cook_dev), (bare.pieces_cook, bare.pieces_cook_dev)):
        with pytest.raises(engine.SurtrError) as e:
            host()
        assert e.value.code == engine.E_STATE                               # no event / before any upload
        with pytest.raises(engine.SurtrError) as e:
            dev(*dev_args(ptrs, (4, 64, 64, 256)))
        assert e.value.code == engine.E_STATE
    for weld, tol in ((-1.0, TOL), (0.0, -1e-9), (float("nan"), TOL), (0.0, float("inf"))):
        with pytest.raises(engine.SurtrError) as e:
            bare.cook_points([cube_points()], weld, tol)
        assert e.value.code == engine.E_INVALID
    assert all((b == 0xAB).all() for b in read())
    bare.close()

    eng, _ = SF.scene_after_click_one(E)
    eng.scene_fragments(None)
    before, event, counts = TS.snapshot(eng), eng.download(), bytes(eng.event_counts())
    hl = eng.event_hulls()
    want_all, want_sel = eng.event_cook(None, 1e-5, 0.0, TOL), eng.event_cook(hl["records"], 1e-5, 0.0, TOL)
    same_bytes(eng.event_cook(None, 1e-5, 0.0, TOL), want_all)              # two calls: the same bits

    def unchanged():
        TS.assert_unchanged(eng, before)
        assert bytes(eng.event_counts()) == counts
        now = eng.download()
        for k in SF.ARRAYS + ("frag_ids",):
            assert np.asarray(now[k]).tobytes() == np.asarray(event[k]).tobytes(), k
    # the host forms: invalid tolerances, hull records of another count, counts one too small
    for host in (eng.event_cook, eng.pieces_cook):
        for weld, tol, rel in ((-1.0, TOL, 1e-5), (0.0, -1.0, 1e-5), (0.0, float("nan"), 1e-5), (0.0, TOL, -1.0)):
            with pytest.raises(engine.SurtrError) as e:
                host(None, rel, weld, tol)
            assert e.value.code == engine.E_INVALID
        with pytest.raises(engine.SurtrError) as e:
            host(hl["records"][:9], 1e-5, 0.0, TOL)
        assert e.value.code == engine.E_INVALID
    full = [want_all[k].shape[0] for k in ("records", "points", "polygons", "idx")]
    for fn in (L.surtr_event_cook, L.surtr_pieces_cook):
        for short in range(4):
            c = [ctypes.c_uint32(x) for x in full]
            c[short].value -= 1
            out = [np.zeros(full[0], C), np.zeros((full[1], 3), F32), np.zeros(full[1], np.uint32), np.zeros(full[2], P), np.zeros(full[3], np.uint16)]
            rc = fn(eng._h, None, ctypes.c_uint32(0), ctypes.c_float(1e-5), ctypes.c_float(0.0), ctypes.c_float(TOL), ctypes.byref(c[0]), engine._p(out[0]),
                    ctypes.byref(c[1]), engine._p(out[1]), engine._p(out[2]), ctypes.byref(c[2]), engine._p(out[3]), ctypes.byref(c[3]), engine._p(out[4]))
            assert rc == engine.E_CAPACITY and [x.value for x in c] == full
            assert all(not np.frombuffer(o.tobytes(), np.uint8).any() for o in out)
        c = [ctypes.c_uint32(x) for x in full]
        assert fn(eng._h, None, ctypes.c_uint32(0), ctypes.c_float(1e-5), ctypes.c_float(0.0), ctypes.c_float(TOL), ctypes.byref(c[0]), engine._p(np.zeros(full[0], C)),
                  ctypes.byref(c[1]), None, None, ctypes.byref(c[2]), None, ctypes.byref(c[3]), None) == engine.E_INVALID      # some but not all arrays
    unchanged()
    # the _dev forms
    for dev, hulls_dev in ((eng.event_cook_dev, eng.event_hulls_dev), (eng.pieces_cook_dev, eng.pieces_hulls_dev)):
        keep, hptr = hull_buffer(torch, eng, hulls_dev, 10, hl["polygons"].shape[0], hl["idx"].shape[0])
        for want, hp in ((want_all, 0), (want_sel, hptr)):
            n = [want[k].shape[0] for k in ("records", "points", "polygons", "idx")]
            cap = (n[0] + 1, n[1], n[2], n[3])
            _, ptrs, read = dev_buffers(torch, (cap[0], cap[1], cap[1], cap[2], cap[3]))
            for bad in ((hp, 1e-5, -1.0, TOL), (hp, 1e-5, 0.0, float("nan")), (hp, -1e-5, 0.0, TOL)):
                with pytest.raises(engine.SurtrError) as e:
                    dev(*(bad + dev_args(ptrs, cap)[4:]))
                assert e.value.code == engine.E_INVALID
            for k in (4, 6, 8, 9, 11):                                      # a NULL array with room asked for
                a = list(dev_args(ptrs, cap, hp))
                a[k] = 0
                with pytest.raises(engine.SurtrError) as e:
                    dev(*a)
                assert e.value.code == engine.E_INVALID
            for short in (63, 64 * n[0]):                                   # records: refused on the host, which knows the count
                a = list(dev_args(ptrs, cap, hp))
                a[5] = short
                with pytest.raises(engine.SurtrError) as e:
                    dev(*a)
                assert e.value.code == engine.E_CAPACITY
            assert all((b == 0xAB).all() for b in read())
            for short in (1, 2, 3):                                         # points, polygons, indices one short: the header and nothing else
                c2 = list(cap)
                c2[short] -= 1
                dev(*dev_args(ptrs, c2, hp))
                raw = read()
                hdr = raw[0][:64].view(C)[0]
                assert (hdr["nv_in"], hdr["nv"], hdr["n_faces"], hdr["n_idx"], hdr["status"]) == (n[0], n[1], n[2], n[3], engine.E_CAPACITY)
                assert (raw[0][64:] == 0xAB).all() and all((r == 0xAB).all() for r in raw[1:])
            dev(*dev_args(ptrs, cap, hp))                                   # exactly enough: the _dev form against the host form
            hdr, got = unpack_dev(read(), n[0])
            assert (hdr["nv_in"], hdr["nv"], hdr["n_faces"], hdr["n_idx"], hdr["status"]) == (n[0], n[1], n[2], n[3], 0)
            same_bytes(got, want)
        # hull records of another call: a header that names another number of solids
        stale = np.zeros(11, TH.H)
        stale[0]["nv"] = 9
        if torch is None:
            sbuf = stale.view(np.uint8).copy(); sptr = sbuf.ctypes.data
        else:
            sbuf = torch.from_numpy(stale.view(np.uint8).copy()).cuda(); sptr = sbuf.data_ptr()
        dev(*dev_args(ptrs, cap, sptr))
        raw = read()
        assert raw[0][:64].view(C)[0]["status"] == engine.E_STATE and raw[0][:64].view(C)[0]["nv"] == 0
        unchanged()
    eng.close()
    cube8_event(E)


def run_streams(E, torch):
    """The _dev forms on a stream of their own, queued twice, with the in-flight hint at 6; then cook_dev directly behind
    event_hulls_dev directly behind fracture_event_async, with no count on the host."""
    eng, _ = SF.scene_after_click_one(E)
    eng.scene_fragments(None)
    hl = eng.event_hulls()
    want = eng.event_cook(hl["records"], 1e-5, 0.0, TOL)
    n = [want[k].shape[0] for k in ("records", "points", "polygons", "idx")]
    cap = (n[0] + 1, n[1], n[2], n[3])
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    eng.set_events_in_flight(6)
    with torch.cuda.stream(st):
        for dev, hulls_dev in ((eng.event_cook_dev, eng.event_hulls_dev), (eng.pieces_cook_dev, eng.pieces_hulls_dev)):
            keep, hptr = hull_buffer(torch, eng, hulls_dev, 10, hl["polygons"].shape[0], hl["idx"].shape[0])
            sets = [dev_buffers(torch, (cap[0], cap[1], cap[1], cap[2], cap[3])) for _ in range(2)]
            for _, ptrs, _ in sets:
                dev(*dev_args(ptrs, cap, hptr))
            st.synchronize()
            for _, _, read in sets:
                hdr, got = unpack_dev(read(), n[0])
                assert hdr["status"] == 0
                same_bytes(got, want)
    eng.close()
    sc = scenes.cube_scene(8)
    eng = E.Engine(0, stream=st.cuda_stream)
    eng.set_events_in_flight(6)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    with torch.cuda.stream(st):
        eng.fracture_event_async(0, 8)
        hkeep, hptrs, _ = TH.dev_buffers(engine, torch, 48 * 64, 4096, 4096)
        hp = hptrs[0]
        eng.event_hulls_dev(hp, 48 * 64, hptrs[1], 4096, hptrs[2], 4096)
        _, tight, read_tight = dev_buffers(torch, (64, 4096, 4096, 4, 4096))      # records fit, polygons do not
        _, ample, read_ample = dev_buffers(torch, (64, 4096, 4096, 4096, 4096))
        eng.event_cook_dev(*dev_args(tight, (64, 4096, 4, 4096), 0))
        eng.event_cook_dev(*dev_args(ample, (64, 4096, 4096, 4096), 0))
        _, sel, read_sel = dev_buffers(torch, (64, 4096, 4096, 4096, 4096))
        eng.event_cook_dev(*dev_args(sel, (64, 4096, 4096, 4096), hp))
    st.synchronize()
    nfrag = eng.event_counts().n_frag
    assert nfrag == 8
    want = eng.event_cook(None, 1e-5, 0.0, TOL)
    hdr = read_tight()[0][:64].view(C)[0]
    assert (hdr["nv_in"], hdr["nv"], hdr["n_faces"], hdr["n_idx"], hdr["status"]) == (8, want["points"].shape[0], want["polygons"].shape[0], want["idx"].shape[0], engine.E_CAPACITY)
    raw = read_tight()
    assert (raw[0][64:] == 0xAB).all() and all((r == 0xAB).all() for r in raw[1:])
    hdr, got = unpack_dev(read_ample(), 8)
    assert hdr["status"] == 0
    same_bytes(got, want)
    _, convexes = scenes.fragments_as_pieces(eng.download())
    check_all(got, positions(convexes), 0.0, TOL, False)
    hdr, got = unpack_dev(read_sel(), 8)
    assert hdr["status"] == 0
    same_bytes(got, eng.event_cook(eng.event_hulls()["records"], 1e-5, 0.0, TOL))
    eng.close()


# ------------------------------------------------------------------ CPU tier (emulation)
def test_designed_solids_alone_in_batches_and_resident(emul_engine):
    run_designed(emul_engine, True)


def test_thin_solids_are_cooked_within_the_bounds(emul_engine):
    run_thin(emul_engine, True)


def test_checker_refuses_seven_wrong_answers(emul_engine):
    run_mutations(emul_engine)


def test_random_sets_have_qhulls_vertices(emul_engine):
    from scipy.spatial import ConvexHull  # noqa: F401  (the CPU tier has scipy; the GPU tier reads the committed file only)
    mine, want = qhull_vertices(), golden_vertices()
    for key in RANDOM:
        assert np.array_equal(mine[key], want[key]), key
    assert [len(want[("sphere", n)]) for _, n in RANDOM[:8]] == [4, 5, 8, 33, 64, 65, 130, 300]
    assert [len(want[("ball", n)]) for _, n in RANDOM[:8]][0] == 4 and len(want[("ball", 300)]) == 75
    run_random(emul_engine, True)


def test_scene_pieces_selected_and_all(emul_engine):
    run_scene(emul_engine, True)


def test_errors_capacity_state_and_dev_forms(emul_engine):
    run_errors(emul_engine, True)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    from oracle import oracle
    import test_cook as T
    case = sys.argv[1]
    if case == "errors":
        T.run_errors(engine, False, torch)
    elif case == "streams":
        T.run_streams(engine, torch)
    else:
        getattr(T, "run_" + case)(engine, False)
    print("ok", case)
""")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["designed", "thin", "random", "scene", "errors", "streams"])
def test_gpu_cook(case):
    run_gpu_child(GPU_CHILD, case, 120)
