"""Collision hulls: face loops and planes of every Convex on the device (hull_dev.hip): event_hulls / pieces_hulls and their _dev forms.

NO REFERENCE RUNS THE NEW CODE.  Two references, both on the host:
  loops    oracle.extract_faces of each Convex (the restated Poly::ExtractFaces);
  numbers  ref_hull below: the definition of include/surtr_hip.h restated with Python floats (IEEE double), one operation at a time in the
           stated order, rounded to float32 where the definition says so -- status bits, planes, the two errors, the extent.
On the emulation tier every byte of the engine's answer equals the reference's.  On the MI355X a plane component may differ by one float32
ulp (double sqrt and division may differ from the host's by one double ulp, which moves a float rounding by at most one step), and the two
errors are recomputed from the planes THE GPU RETURNED and must agree within one float32 ulp of the value plus 2^-40 * extent (four double
operations on terms of size <= extent).

Designed solids.  A solid of three vertices cannot be presented to the engine at all (surtr_load_fragments and surtr_upload_pieces refuse
it, SURTR_E_INVALID, as tests/test_pick_queries.py records): the reference says FEW for it and the test asserts the refusal.  The Convex
of tests/golden/degenerate_sliver_convex.npz is an un-clipped box whose rings repeat nothing (status 0 by the reference); the Convex that
does list a neighbour twice is the one of tests/golden/sliver_convex_walk_bound.npz: both are checked, the second is the IRREGULAR one.

The convex designed solids' planarity and convexity are at most CONVEX_ULPS = 2 float32 ulps of the extent (the issue's slack bound of
8, lowered).  Reasoning: the vertices of such a face lie in its plane up to their own float rounding, so what is left is the rounding
of (n, d) to float: with every component within ONE float32 ulp of the double value (half an ulp on the host; the GPU tier allows the
plane one ulp), coordinates |x| <= 1.1, |n| <= 1, |d| <= 1.1 and an extent in [1, 4), the error is at most 3 * 1.1 * 2^-24 + 2^-23 =
1.83 ulps of an extent in [1, 2) and less of a larger one.  The float64 reference shows 0.40; the bound is asserted on it first, then on
the engine.

The CPU tier runs on the emulation library (conftest's emul_engine); the GPU tier runs the same functions on the MI355X in child
processes under a time limit (helpers.run_gpu_child)."""
import ctypes
import json
import math
import os
import subprocess
import textwrap

import numpy as np
import pytest

import faces_ref as FR
import regroup_ref as RR
import test_scene as TS
import test_scene_fragments as SF
from helpers import run_gpu_child
from surtr_amd import engine, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
H, P = engine.HULL_DTYPE, engine.POLY_DTYPE
FEW, OPEN, FLAT, IRREGULAR, LARGE, OVER_255 = 1, 2, 4, 8, 16, 32
WITHHELD = FEW | OPEN | IRREGULAR | LARGE
F32 = np.float32
CONVEX_ULPS = 2


# ------------------------------------------------------------------ the reference (Python floats are IEEE doubles)
def _rings(s):
    off, nbr = np.asarray(s["off"], np.int64), np.asarray(s["nbr"], np.int64)
    return [[int(x) for x in nbr[off[v]:off[v + 1]]] for v in range(len(off) - 1)]


def _next(rings, u, w):
    """-> (the ring entry of w listed just before u, u was listed)."""
    r = rings[w]
    if not r:
        return -1, False
    k = r.index(u) if u in r else len(r)
    return r[len(r) - 1 if k in (0, len(r)) else k - 1], k < len(r)


def _lead(rings, nv, v, w, nh):
    """One walk from half-edge (v -> w): -> (length of the loop when it leads it, else 0; status bits)."""
    prev, cur = v, w
    for k in range(1, nh + 1):
        x, listed = _next(rings, prev, cur)
        if not listed or not 0 <= x < nv:
            return 0, OPEN
        prev, cur = cur, x
        if prev == v:
            return (k, 0) if cur == w else (0, IRREGULAR)
        if prev < v:
            return 0, 0
    return 0, OPEN


def _plane64(q):
    """Newell normal and mid-range offset of a loop of float64 positions -> four Python floats, or None when N is exactly zero."""
    nx = ny = nz = 0.0
    for i in range(1, len(q) - 1):
        ax, ay, az = q[i][0] - q[0][0], q[i][1] - q[0][1], q[i][2] - q[0][2]
        bx, by, bz = q[i + 1][0] - q[0][0], q[i + 1][1] - q[0][1], q[i + 1][2] - q[0][2]
        cx, cy, cz = ay * bz - az * by, az * bx - ax * bz, ax * by - ay * bx
        nx, ny, nz = nx + cx, ny + cy, nz + cz
    if nx == 0.0 and ny == 0.0 and nz == 0.0:
        return None
    ln = math.sqrt((nx * nx + ny * ny) + nz * nz)
    nx, ny, nz = nx / ln, ny / ln, nz / ln
    t = [(nx * p[0] + ny * p[1]) + nz * p[2] for p in q]
    return nx, ny, nz, -(max(t) + min(t)) / 2.0


def _dist(pl, p):
    return ((float(pl[0]) * p[0] + float(pl[1]) * p[1]) + float(pl[2]) * p[2]) + float(pl[3])


def errors_from_planes(pos, loops, planes):
    """(convexity, planarity, any flat face) in double from float32 planes, as the definition reads them."""
    pts = [[float(c) for c in p] for p in np.asarray(pos, np.float32)]
    conv, plan, flat, solid_face = -math.inf, 0.0, False, False
    for loop, pl in zip(loops, planes):
        if pl[0] == 0 and pl[1] == 0 and pl[2] == 0:
            flat = True
            continue
        solid_face = True
        conv = max(conv, max(_dist(pl, p) for p in pts))
        plan = max(plan, max(abs(_dist(pl, pts[v])) for v in loop))
    return (conv if solid_face else 0.0), plan, flat


_REFS = {}


def ref_hull(s):
    """The definition on one solid, computed once per solid and left unchanged."""
    key = (np.asarray(s["pos"], np.float32).tobytes(), np.asarray(s["off"], np.uint32).tobytes(), np.asarray(s["nbr"], np.int32).tobytes())
    if key not in _REFS:
        _REFS[key] = _ref_hull(s)
    return _REFS[key]


def _ref_hull(s):
    """The definition on one solid -> dict(record fields without the offsets, loops, planes float32[F, 4])."""
    pos = np.asarray(s["pos"], np.float32).reshape(-1, 3)
    rings, nv = _rings(s), pos.shape[0]
    out = dict(nv=nv, n_faces=0, n_idx=0, status=0, max_loop=0, convexity=F32(0), planarity=F32(0), extent=F32(0), loops=[], planes=np.zeros((0, 4), F32))
    nh = sum(len(r) for r in rings)
    st = (FEW if nv < 4 else 0) | (LARGE if nv > 65535 or nh > 65535 else 0)
    if st:
        out["status"] = st | (OVER_255 if nv > 255 else 0)
        return out
    if not np.isfinite(pos).all():
        st |= OPEN
    loops = []
    for v in range(nv):
        for s_, w in enumerate(rings[v]):
            if not 0 <= w < nv:
                st |= OPEN
                continue
            if w in rings[v][:s_]:
                st |= IRREGULAR
                continue
            k, bits = _lead(rings, nv, v, w, nh)
            st |= bits
            if k:
                loop, prev, cur = [v], v, w
                while len(loop) < k:
                    loop.append(cur)
                    prev, cur = cur, _next(rings, prev, cur)[0]
                loops.append(loop)
    if nh % 2 or nv - nh // 2 + len(loops) != 2:
        st |= IRREGULAR
    if st & WITHHELD:
        out["status"] = st | (OVER_255 if nv > 255 else 0)
        return out
    pts = [[float(c) for c in p] for p in pos]
    planes = np.zeros((len(loops), 4), F32)
    for f, loop in enumerate(loops):
        pl = _plane64([pts[v] for v in loop])
        if pl is not None:
            planes[f] = [F32(c) for c in pl]
    conv, plan, flat = errors_from_planes(pos, loops, planes)
    ext = (pos.max(0) - pos.min(0)).astype(F32).max()
    out.update(n_faces=len(loops), n_idx=sum(map(len, loops)), max_loop=max(map(len, loops)), loops=loops, planes=planes,
               status=st | (FLAT if flat else 0) | (OVER_255 if nv > 255 or len(loops) > 255 else 0),
               convexity=F32(conv), planarity=F32(plan), extent=F32(ext))
    return out


def ref_batch(solids):
    """-> (records, polygons, idx, the per-solid references) as the engine lays them out."""
    refs = [ref_hull(s) for s in solids]
    rec = np.zeros(len(refs), H)
    polys, idx = [], []
    fo = io = 0
    for k, r in enumerate(refs):
        for name in ("nv", "n_faces", "n_idx", "status", "max_loop", "convexity", "planarity", "extent"):
            rec[k][name] = r[name]
        rec[k]["face_off"], rec[k]["idx_off"] = fo, io
        base = 0
        for loop, pl in zip(r["loops"], r["planes"]):
            p = np.zeros((), P)
            p["plane"], p["n_verts"], p["index_base"] = pl, len(loop), base
            polys.append(p)
            idx += loop
            base += len(loop)
        fo += r["n_faces"]; io += r["n_idx"]
    return rec, (np.asarray(polys, P) if polys else np.zeros(0, P)), np.asarray(idx, np.uint16), refs


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, F32)).astype(F32)).astype(np.float64)


def check(got, solids, oracle, exact, refs_out=None):
    """One answer of the engine against both references.  exact: every byte equal (emulation); else the GPU tolerances."""
    rec, polys, idx, refs = ref_batch(solids)
    if refs_out is not None:
        refs_out.extend(refs)
    g = got["records"]
    assert g.dtype == H and got["polygons"].dtype == P and got["idx"].dtype == np.uint16
    for name in ("nv", "n_faces", "n_idx", "status", "face_off", "idx_off", "max_loop", "reserved0", "reserved1", "extent"):
        assert np.array_equal(g[name], rec[name]), (name, g[name], rec[name])
    # offsets are the exclusive sums, index_base the sum inside the solid
    assert np.array_equal(g["face_off"], np.concatenate([[0], np.cumsum(g["n_faces"])[:-1]]).astype(np.uint32))
    assert np.array_equal(g["idx_off"], np.concatenate([[0], np.cumsum(g["n_idx"])[:-1]]).astype(np.uint32))
    assert got["polygons"].shape[0] == int(g["n_faces"].sum()) and got["idx"].shape[0] == int(g["n_idx"].sum())
    assert np.array_equal(got["idx"], idx)
    assert np.array_equal(got["polygons"]["n_verts"], polys["n_verts"]) and np.array_equal(got["polygons"]["index_base"], polys["index_base"])
    for k, (s, r) in enumerate(zip(solids, refs)):
        a, b = int(g[k]["face_off"]), int(g[k]["face_off"]) + int(g[k]["n_faces"])
        if r["status"] & WITHHELD:
            assert a == b and g[k]["n_idx"] == 0 and g[k]["convexity"] == 0 and g[k]["planarity"] == 0
            continue
        # the loops are ExtractFaces', offsets and indices equal exactly
        fo, fi = oracle.extract_faces(s)
        i0 = int(g[k]["idx_off"])
        assert np.array_equal(fo, np.concatenate([[0], np.cumsum(got["polygons"]["n_verts"][a:b].astype(np.int64))]))
        assert np.array_equal(fo[:-1], got["polygons"]["index_base"][a:b])
        assert np.array_equal(fi.astype(np.int64), got["idx"][i0:i0 + int(g[k]["n_idx"])].astype(np.int64))
        gp = got["polygons"]["plane"][a:b]
        if exact:
            assert gp.tobytes() == r["planes"].tobytes(), k
            assert g[k]["convexity"].tobytes() == r["convexity"].tobytes() and g[k]["planarity"].tobytes() == r["planarity"].tobytes(), (k, g[k], r)
        else:
            d = np.abs(gp.astype(np.float64) - r["planes"].astype(np.float64))
            tol = np.maximum(ulp32(gp), ulp32(r["planes"]))
            print("solid %d: planes off by at most %.3g ulp" % (k, float((d / tol).max())))
            assert (d <= tol).all(), k
            assert np.array_equal((gp[:, :3] == 0).all(1), (r["planes"][:, :3] == 0).all(1))
            conv, plan, _ = errors_from_planes(s["pos"], r["loops"], gp)
            for name, want in (("convexity", conv), ("planarity", plan)):
                err, room = abs(float(g[k][name]) - want), float(ulp32(want)) + 2.0 ** -40 * float(g[k]["extent"])
                print("solid %d: %s %.9g against %.17g from its planes: off by %.3g of %.3g" % (k, name, g[k][name], want, err, room))
                assert err <= room, (k, name)
    return refs


# ------------------------------------------------------------------ designed solids
def golden_convex(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"))
    return {"pos": d["conv_pos"], "off": d["conv_off"], "nbr": d["conv_nbr"]}


_DESIGNED = []


def designed():
    """[(name, solid, listed status or None: whatever the reference says), ...]; the convex ones first."""
    if not _DESIGNED:
        three = {"pos": np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0]]), "off": np.uint32([0, 2, 4, 6]), "nbr": np.int32([1, 2, 2, 0, 0, 1])}
        _DESIGNED.extend([("tetrahedron", FR.pyramid_over(FR.regular(3)), 0), ("cube", RR.box((-1, -1, -1), (1, 1, 1)), 0)] +
                         [("prism %d" % n, FR.prism_over(FR.regular(n)), 0) for n in (63, 64, 65)] +
                         [("prism 300", FR.prism_over(FR.regular(300)), OVER_255)] +
                         [("polytope %d" % n, FR.tangent_polytope(n), 0) for n in (34, 35)] +
                         [("three vertices", three, FEW),
                          ("degenerate_sliver_convex", golden_convex("degenerate_sliver_convex"), 0),
                          ("sliver_convex_walk_bound", golden_convex("sliver_convex_walk_bound"), None),
                          ("pinched_face_fragment", golden_convex("pinched_face_fragment"), None)])
    return _DESIGNED


N_CONVEX = 8


def run_designed(E, oracle, exact):
    cases = designed()
    refs = {name: ref_hull(s) for name, s, _ in cases}
    # the reference first: listed statuses, sizes at the wave boundary, the bound on the convex ones
    for name, s, listed in cases:
        if listed is not None:
            assert refs[name]["status"] == listed, (name, refs[name]["status"])
    assert [cases[k][1]["pos"].shape[0] for k in (2, 3, 4, 5, 6, 7)] == [126, 128, 130, 600, 64, 66]
    assert refs["prism 64"]["max_loop"] == 64 and refs["prism 65"]["max_loop"] == 65 and refs["prism 300"]["max_loop"] == 300
    assert refs["sliver_convex_walk_bound"]["status"] & IRREGULAR and refs["sliver_convex_walk_bound"]["n_faces"] == 0
    pinched = refs["pinched_face_fragment"]
    fo, fi = oracle.extract_faces(cases[-1][1])
    if not pinched["status"] & WITHHELD:      # whichever the reference says: equal loops, or IRREGULAR
        assert [v for loop in pinched["loops"] for v in loop] == fi.tolist() and pinched["n_faces"] == len(fo) - 1
    else:
        assert pinched["status"] & IRREGULAR
    for name, s, _ in cases[:N_CONVEX]:
        r = refs[name]
        bound = CONVEX_ULPS * float(ulp32(r["extent"]))
        print("%s: extent %.6g planarity %.3g convexity %.3g (%.2f / %.2f ulps of the extent)"
              % (name, r["extent"], r["planarity"], r["convexity"], r["planarity"] / ulp32(r["extent"]), r["convexity"] / ulp32(r["extent"])))
        assert 0 <= r["planarity"] <= bound and r["convexity"] <= bound and not r["status"] & FLAT, name
    eng = E.Engine(0)
    # three vertices: no entry point takes such a solid
    for call in (lambda: eng.load_fragments([cases[8][1]], [cases[8][1]]), lambda: eng.upload_pieces([cases[8][1]], [cases[8][1]])):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == engine.E_INVALID
    loadable = [c for c in cases if c[0] != "three vertices"]
    for name, s, _ in loadable:                                      # each alone
        eng.load_fragments([s], [s])
        got = eng.event_hulls()
        check(got, [s], oracle, exact)
        if name in [c[0] for c in cases[:N_CONVEX]]:
            bound = F32(CONVEX_ULPS * float(ulp32(got["records"][0]["extent"])))
            assert got["records"][0]["planarity"] <= bound and got["records"][0]["convexity"] <= bound, name
    # one batch, the withheld solids in the middle; then reversed
    order = [c[1] for c in loadable[:4]] + [loadable[-2][1], loadable[-1][1]] + [c[1] for c in loadable[4:-2]]
    assert any(ref_hull(s)["status"] & WITHHELD for s in order[4:6]) and not ref_hull(order[-1])["status"] & WITHHELD
    for batch in (order, order[::-1]):
        eng.load_fragments(batch, batch)
        got = eng.event_hulls()
        check(got, batch, oracle, exact)
        # the same solids resident: pieces_hulls gives the same bytes
        eng2 = E.Engine(0)
        eng2.upload_pieces(batch, batch)
        res = eng2.pieces_hulls()
        for k in ("records", "polygons", "idx"):
            assert res[k].tobytes() == got[k].tobytes(), k
        eng2.close()
    eng.close()


# ------------------------------------------------------------------ the scene
def convexes_of(eng, pieces):
    return [eng.download_piece(p, 1) for p in pieces]


def same_bytes(a, b):
    for k in ("records", "polygons", "idx"):
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), k


def run_scene(E, oracle, exact):
    eng, world = SF.scene_after_click_one(E)
    solids = convexes_of(eng, range(10))
    assert max(s["pos"].shape[0] for s in solids) == 140                    # the ACH Convex of the blob
    refs = []
    eng.scene_fragments(None)
    via_event = eng.event_hulls()
    check(via_event, solids, oracle, exact, refs)
    same_bytes(eng.pieces_hulls(), via_event)
    # conditions taken from the reference, asserted there first and then on the engine
    rec = via_event["records"]
    for st, nf, conv, plan, ext, planes in [(np.asarray([r["status"] for r in refs]), np.asarray([r["n_faces"] for r in refs]),
                                              np.asarray([r["convexity"] for r in refs]), np.asarray([r["planarity"] for r in refs]),
                                              np.asarray([r["extent"] for r in refs]), [r["planes"] for r in refs]),
                                             (rec["status"], rec["n_faces"], rec["convexity"], rec["planarity"], rec["extent"],
                                              [via_event["polygons"]["plane"][int(r["face_off"]):int(r["face_off"]) + int(r["n_faces"])] for r in rec])]:
        assert (nf > 0).all() and not (st & WITHHELD).any()                 # all ten emit polygons
        flat = np.nonzero(st & FLAT)[0]
        assert flat.shape[0] == 1 and int((planes[int(flat[0])][:, :3] == 0).all(1).sum()) == 1
        print("convexity / extent:", (conv / ext).tolist()); print("planarity / extent:", (plan / ext).tolist())
        assert int((conv > 0.1 * ext).sum()) == 1
        assert (plan <= 1e-6 * ext).all()
    usable = [engine.hull_usable(r) for r in rec]
    assert usable == [engine.hull_usable(dict(status=r["status"], extent=r["extent"], convexity=r["convexity"], planarity=r["planarity"])) for r in refs]
    assert 0 < sum(usable) < 10
    # a list of compounds, in the order given
    eng.scene_fragments([5, 2, 0])
    ids = SF.pieces_of(SF.TABLE, [5, 2, 0])
    check(eng.event_hulls(), [solids[p] for _, p in ids], oracle, exact)
    # after a refit: the Convex the context holds now
    eng.event_refit()
    ev = eng.download()
    _, refitted = scenes.fragments_as_pieces(ev)
    assert any(a["pos"].shape != b["pos"].shape or a["pos"].tobytes() != b["pos"].tobytes() for a, b in zip(refitted, [solids[p] for _, p in ids]))
    check(eng.event_hulls(), refitted, oracle, exact)
    # after a second commit
    n, first, n_new, src, _ = TS.click_two(E, eng, world, 2)
    table = eng.scene_compounds()
    made = list(range(first, first + n_new))
    ids = SF.pieces_of(table, made)
    eng.scene_fragments(made)
    check(eng.event_hulls(), convexes_of(eng, [p for _, p in ids]), oracle, exact)
    everything = eng.pieces_hulls()
    check(everything, convexes_of(eng, range(int(table[-1]))), oracle, exact)
    eng.close()


# ------------------------------------------------------------------ errors and state
def dev_buffers(E, torch, rec_bytes, n_polys, n_idx):
    """-> three 'device' byte buffers filled with 0xAB and a function that reads them back (the emulation's device memory is host memory)."""
    sizes = (rec_bytes, 20 * n_polys, 2 * n_idx)
    if torch is None:
        bufs = [np.full(max(b, 1), 0xAB, np.uint8) for b in sizes]
        return bufs, [b.ctypes.data for b in bufs], lambda: [b.copy() for b in bufs]
    bufs = [torch.full((max(b, 1),), 0xAB, dtype=torch.uint8, device="cuda") for b in sizes]
    torch.cuda.synchronize()
    return bufs, [b.data_ptr() for b in bufs], lambda: [b.cpu().numpy() for b in bufs]


def unpack_dev(raw, n):
    hdr = raw[0][:48].view(H)[0]
    rec = raw[0][48:48 * (n + 1)].view(H)
    return hdr, {"records": rec, "polygons": raw[1][:20 * int(hdr["n_faces"])].view(P), "idx": raw[2][:2 * int(hdr["n_idx"])].view(np.uint16)}


def run_errors(E, oracle, exact, torch=None):
    L = E.lib()
    bare = E.Engine(0)
    n3 = [ctypes.c_uint32(0) for _ in range(3)]
    _, ptrs, read = dev_buffers(E, torch, 48 * 4, 64, 256)
    for host, dev in ((bare.event_hulls, bare.event_hulls_dev), (bare.pieces_hulls, bare.pieces_hulls_dev)):
        with pytest.raises(engine.SurtrError) as e:
            host()
        assert e.value.code == engine.E_STATE                               # no event / before any upload
        with pytest.raises(engine.SurtrError) as e:
            dev(ptrs[0], 48 * 4, ptrs[1], 64, ptrs[2], 256)
        assert e.value.code == engine.E_STATE
    assert all((b == 0xAB).all() for b in read())
    # after a failed event (an arena too small for its fragments)
    sc = scenes.blob_scene(64)
    bare.set_arena(64, 256, 256)
    bare.upload_pieces([sc["mesh"]], [sc["convex"]])
    bare.upload_pattern(sc["face_off"], sc["v012"])
    bare.place_cells(sc["scale"], sc["translate"])
    with pytest.raises(engine.SurtrError) as e:
        bare.fracture_event(0, 64)
    assert e.value.code == engine.E_CAPACITY
    with pytest.raises(engine.SurtrError) as e:
        bare.event_hulls()
    assert e.value.code == engine.E_STATE
    with pytest.raises(engine.SurtrError) as e:
        bare.event_hulls_dev(ptrs[0], 48 * 4, ptrs[1], 64, ptrs[2], 256)
    assert e.value.code == engine.E_STATE
    assert bare.pieces_hulls()["records"].shape[0] == 1                     # the resident piece is still there
    bare.close()

    eng, _ = SF.scene_after_click_one(E)
    eng.scene_fragments(None)
    before, event, counts = TS.snapshot(eng), eng.download(), bytes(eng.event_counts())
    want = eng.event_hulls()
    nrec, npoly, nidx = want["records"].shape[0], want["polygons"].shape[0], want["idx"].shape[0]
    assert nrec == 10

    def unchanged():
        TS.assert_unchanged(eng, before)
        assert bytes(eng.event_counts()) == counts
        now = eng.download()
        for k in SF.ARRAYS + ("frag_ids",):
            assert np.asarray(now[k]).tobytes() == np.asarray(event[k]).tobytes(), k
    for fn in (L.surtr_event_hulls, L.surtr_pieces_hulls):
        # NULL pointers for the counts; some but not all arrays
        rec, poly, idx = np.zeros(nrec, H), np.zeros(npoly, P), np.zeros(nidx, np.uint16)
        c = [ctypes.c_uint32(nrec), ctypes.c_uint32(npoly), ctypes.c_uint32(nidx)]
        assert fn(eng._h, None, None, ctypes.byref(c[1]), None, ctypes.byref(c[2]), None) == engine.E_INVALID
        assert fn(eng._h, ctypes.byref(c[0]), engine._p(rec), ctypes.byref(c[1]), None, ctypes.byref(c[2]), engine._p(idx)) == engine.E_INVALID
        assert fn(None, ctypes.byref(c[0]), None, ctypes.byref(c[1]), None, ctypes.byref(c[2]), None) == engine.E_INVALID
        # each count one too small: SURTR_E_CAPACITY, the counts returned, nothing written
        for short in range(3):
            c = [ctypes.c_uint32(nrec), ctypes.c_uint32(npoly), ctypes.c_uint32(nidx)]
            c[short].value -= 1
            assert fn(eng._h, ctypes.byref(c[0]), engine._p(rec), ctypes.byref(c[1]), engine._p(poly), ctypes.byref(c[2]), engine._p(idx)) == engine.E_CAPACITY
            assert [x.value for x in c] == [nrec, npoly, nidx] and not rec["nv"].any() and not poly["n_verts"].any() and not idx.any()
        unchanged()
    for dev in (eng.event_hulls_dev, eng.pieces_hulls_dev):
        bufs, ptrs, read = dev_buffers(E, torch, 48 * (nrec + 1), npoly, nidx)
        for args in ((0, 48 * (nrec + 1), ptrs[1], npoly, ptrs[2], nidx), (ptrs[0], 48 * (nrec + 1), 0, npoly, ptrs[2], nidx),
                     (ptrs[0], 48 * (nrec + 1), ptrs[1], npoly, 0, nidx)):
            with pytest.raises(engine.SurtrError) as e:
                dev(*args)
            assert e.value.code == engine.E_INVALID
        # records that do not fit are refused on the host (the counts are known there): nothing is written
        for short in (47, 48 * nrec):
            with pytest.raises(engine.SurtrError) as e:
                dev(ptrs[0], short, ptrs[1], npoly, ptrs[2], nidx)
            assert e.value.code == engine.E_CAPACITY
        assert all((b == 0xAB).all() for b in read())
        # polygons or indices that do not fit: found on the device, which writes the header and nothing else
        for pc, ic in ((npoly - 1, nidx), (npoly, nidx - 1)):
            dev(ptrs[0], 48 * (nrec + 1), ptrs[1], pc, ptrs[2], ic)
            raw = read()
            hdr = raw[0][:48].view(H)[0]
            assert (hdr["nv"], hdr["n_faces"], hdr["n_idx"], hdr["status"]) == (nrec, npoly, nidx, engine.E_CAPACITY)
            assert (raw[0][48:] == 0xAB).all() and (raw[1] == 0xAB).all() and (raw[2] == 0xAB).all()
        # everything fits exactly: the _dev form against the host form
        dev(ptrs[0], 48 * (nrec + 1), ptrs[1], npoly, ptrs[2], nidx)
        hdr, got = unpack_dev(read(), nrec)
        assert (hdr["nv"], hdr["n_faces"], hdr["n_idx"], hdr["status"]) == (nrec, npoly, nidx, 0) and not hdr["extent"]
        same_bytes(got, want)
        unchanged()
    same_bytes(eng.event_hulls(), want)                                     # two calls: the same bits
    eng.close()


# ------------------------------------------------------------------ CPU tier (emulation)
def test_designed_solids_alone_and_as_batches(emul_engine, oracle):
    run_designed(emul_engine, oracle, True)


def test_scene_pieces_by_both_routes(emul_engine, oracle):
    run_scene(emul_engine, oracle, True)


def test_errors_state_and_dev_forms(emul_engine, oracle):
    run_errors(emul_engine, oracle, True)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    from oracle import oracle
    import test_hulls as T
    case = sys.argv[1]
    oracle.lib()
    if case == "errors":
        T.run_errors(engine, oracle, False, torch)
    elif case == "streams":
        T.run_streams(engine, oracle, torch)
    elif case == "harness":
        T.check_harness(engine, %(root)r)
    else:
        getattr(T, "run_" + case)(engine, oracle, False)
    print("ok", case)
""")


def run_streams(E, oracle, torch):
    """The _dev forms on a stream of their own, queued twice, with the in-flight hint at 6; then the device-side capacity refusal right
    behind fracture_event_async (no counts on the host)."""
    eng, _ = SF.scene_after_click_one(E)
    eng.scene_fragments(None)
    want = eng.event_hulls()
    nrec, npoly, nidx = want["records"].shape[0], want["polygons"].shape[0], want["idx"].shape[0]
    st = torch.cuda.Stream()
    eng.set_stream(st.cuda_stream)
    eng.set_events_in_flight(6)
    with torch.cuda.stream(st):
        for dev in (eng.event_hulls_dev, eng.pieces_hulls_dev):
            sets = [dev_buffers(E, torch, 48 * (nrec + 1), npoly, nidx) for _ in range(2)]
            for _, ptrs, _ in sets:
                dev(ptrs[0], 48 * (nrec + 1), ptrs[1], npoly, ptrs[2], nidx)
            st.synchronize()
            for _, _, read in sets:
                hdr, got = unpack_dev(read(), nrec)
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
        _, small, read_small = dev_buffers(E, torch, 48 * 4, 4096, 4096)       # room for three records: the event has eight fragments
        _, tight, read_tight = dev_buffers(E, torch, 48 * 64, 4, 4096)         # records fit, polygons do not
        _, ample, read_ample = dev_buffers(E, torch, 48 * 64, 4096, 4096)
        eng.event_hulls_dev(small[0], 48 * 4, small[1], 4096, small[2], 4096)
        eng.event_hulls_dev(tight[0], 48 * 64, tight[1], 4, tight[2], 4096)
        eng.event_hulls_dev(ample[0], 48 * 64, ample[1], 4096, ample[2], 4096)
    st.synchronize()
    n = eng.event_counts().n_frag
    assert n == 8
    want = eng.event_hulls()
    for read in (read_small, read_tight):
        raw = read()
        hdr = raw[0][:48].view(H)[0]
        assert (hdr["nv"], hdr["n_faces"], hdr["n_idx"], hdr["status"]) == (n, want["polygons"].shape[0], want["idx"].shape[0], engine.E_CAPACITY)
        assert (raw[0][48:] == 0xAB).all() and (raw[1] == 0xAB).all() and (raw[2] == 0xAB).all()
    hdr, got = unpack_dev(read_ample(), n)
    assert hdr["status"] == 0
    same_bytes(got, want)
    _, convexes = scenes.fragments_as_pieces(eng.download())
    check(want, convexes, oracle, False)
    eng.close()


def check_harness(E, root, exe=None):
    """surtr_harness --scene-clicks ... --init-compounds --hulls against the Python calls, and without --hulls against the lines the
    harness printed before the flag existed (test_scene_fragments.check_harness states them)."""
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    clicks = [([-10.0, 0.3, 0.2], [1.0, 0.0, 0.0]), ([0.3, 0.2, 10.0], [0.0, 0.0, -1.0])]
    arg = ";".join(",".join("%r" % x for x in o + d) for o, d in clicks)
    base = [exe, "--mesh", "cube", "--cells", "8", "--scene-clicks", arg, "--impact-radius", "2.0", "--init-compounds"]
    out = {}
    for flag in ((), ("--hulls",)):
        p = subprocess.run(base + list(flag), capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        out[flag] = [json.loads(x) for x in p.stdout.strip().splitlines() if x.startswith('{"init_compound"')]
    sc = scenes.cube_scene(8)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, 8)
    n = eng.pieces_from_event()
    eng.scene_set_compounds(list(range(0, n, 2)) + [n])
    plain, hulled = [], []
    for k, (o, d) in enumerate(clicks):
        made = TS.python_click(eng, o, d, 2.0, 8)["compounds_made"]
        table = eng.scene_compounds()
        eng.scene_fragments(made)
        ev, hl = eng.download(), eng.event_hulls()
        f = 0
        for c in made:
            m = int(table[c + 1] - table[c])
            a, b = int(ev["mesh_vert_off"][f]), int(ev["mesh_vert_off"][f + m])
            i0, i1 = int(ev["idx_off"][f]), int(ev["idx_off"][f + m])
            line = dict(init_compound=c, click=k, pieces=m, vertices=b - a, indices=i1 - i0, fnv=SF.fnv1a(ev["vnc"][a:b], ev["idx"][i0:i1]))
            plain.append(line)
            r = hl["records"][f:f + m]
            fa, fb = int(r[0]["face_off"]), int(r[-1]["face_off"]) + int(r[-1]["n_faces"])
            ia, ib = int(r[0]["idx_off"]), int(r[-1]["idx_off"]) + int(r[-1]["n_idx"])
            hulled.append(dict(line, hull_polygons=fb - fa, hull_indices=ib - ia, hulls_usable=sum(engine.hull_usable(x) for x in r),
                               hull_fnv=SF.fnv1a(hl["polygons"][fa:fb], hl["idx"][ia:ib])))
            f += m
    assert out[()] == plain and len(plain) >= 2, (out[()], plain)
    assert out[("--hulls",)] == hulled, (out[("--hulls",)], hulled)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["designed", "scene", "errors", "streams"])
def test_gpu_hulls(case):
    run_gpu_child(GPU_CHILD, case, 120)


@pytest.mark.gpu
def test_gpu_harness_init_compounds_hulls():
    run_gpu_child(GPU_CHILD, "harness", 150)
