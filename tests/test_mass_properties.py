"""Mass, centre of mass and inertia tensor of every fragment and resident piece on the device (mass_dev.hip), and of compounds
(surtr_combine_mass), against a numpy float64 reference built from Engine.extract_faces: every face fanned around its lowest
vertex, every term relative to the solid's vertex 0 (Poly::Moments' origin shift).

The CPU tier runs on the one emulation library of tests/emul (conftest's emul_engine); the GPU tier runs the bench scene on the
MI355X in child processes under a time limit (helpers.run_gpu_child)."""
import ctypes
import textwrap

import numpy as np
import pytest

from helpers import run_gpu_child
from surtr_amd import engine, scenes

RHO = 10.0


# ------------------------------------------------------------------ numpy reference
def ref_integrals(eng, solid):
    """(nv, J) with J = integrals of 1, x, y, z, xx, yy, zz, xy, yz, zx relative to vertex 0 (float64)."""
    pos = np.asarray(solid["pos"], np.float32).reshape(-1, 3).astype(np.float64)
    if pos.shape[0] < 4:
        return pos.shape[0], None
    fo, fi = eng.extract_faces(solid)
    tris = []
    for f in range(fo.shape[0] - 1):
        loop = fi[fo[f]:fo[f + 1]]
        loop = np.roll(loop, -int(np.argmin(loop)))
        for j in range(1, loop.shape[0] - 1):
            tris.append((loop[0], loop[j], loop[j + 1]))
    return pos.shape[0], tet_integrals(pos - pos[0], np.asarray(tris, np.int64).reshape(-1, 3))


def tet_integrals(P, T):
    """The tetrahedra (vertex 0, triangle): the kernel's formula, operation for operation (elementwise float64, no fused
    multiply-add), so that a thin solid -- whose triple products cancel -- rounds alike; only the order of the sums differs."""
    a, b, c = P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]
    ax, ay, az, bx, by, bz, cx, cy, cz = a[:, 0], a[:, 1], a[:, 2], b[:, 0], b[:, 1], b[:, 2], c[:, 0], c[:, 1], c[:, 2]
    v6 = ax * (by * cz - bz * cy) + ay * (bz * cx - bx * cz) + az * (bx * cy - by * cx)
    sx, sy, sz = ax + bx + cx, ay + by + cy, az + bz + cz
    J = np.zeros(10)
    J[0] = v6.sum() / 6.0
    J[1:4] = [(v6 * sx).sum() / 24.0, (v6 * sy).sum() / 24.0, (v6 * sz).sum() / 24.0]
    sq = lambda p, q, r, t: (v6 * (p[0] * p[1] + q[0] * q[1] + r[0] * r[1] + t[0] * t[1])).sum() / 120.0
    J[4:10] = [sq((ax, ax), (bx, bx), (cx, cx), (sx, sx)), sq((ay, ay), (by, by), (cy, cy), (sy, sy)),
               sq((az, az), (bz, bz), (cz, cz), (sz, sz)), sq((ax, ay), (bx, by), (cx, cy), (sx, sy)),
               sq((ay, az), (by, bz), (cy, cz), (sy, sz)), sq((az, ax), (bz, bx), (cz, cx), (sz, sx))]
    tet_integrals.cond = float(np.abs(v6).sum() / max(abs(v6.sum()), 1e-300))      # cancellation in the sums (1 for a box)
    # what float terms (Poly::Moments) can be off by: their rounding inside every triple product
    tet_integrals.fmag = float((np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) * np.linalg.norm(c, axis=1)).sum() / 6.0 * 1e-6)
    return J


def record_from_integrals(J, origin, rho=RHO):
    vol = J[0]
    c = J[1:4] / vol
    xx, yy, zz = J[4] - vol * c[0] ** 2, J[5] - vol * c[1] ** 2, J[6] - vol * c[2] ** 2
    xy, yz, zx = J[7] - vol * c[0] * c[1], J[8] - vol * c[1] * c[2], J[9] - vol * c[2] * c[0]
    inertia = rho * np.array([yy + zz, xx + zz, xx + yy, -xy, -yz, -zx])
    return vol, np.asarray(origin, np.float64) + c, inertia


def tensor(i6):
    return np.array([[i6[0], i6[3], i6[5]], [i6[3], i6[1], i6[4]], [i6[5], i6[4], i6[2]]])


def check_against_reference(ref_eng, solids, rec, rho=RHO, require_ok=True):
    assert rec.shape[0] == len(solids)
    for k, s in enumerate(solids):
        nv, J = ref_integrals(ref_eng, s)
        r = rec[k]
        assert r["nv"] == nv, k
        if J is None:
            assert r["status"] == 1 and r["volume"] == 0 and r["mass"] == 0 and not r["com"].any() and not r["inertia"].any(), k
            continue
        pos = np.asarray(s["pos"], np.float64).reshape(-1, 3)
        L = float(np.abs(pos.max(0) - pos.min(0)).max())
        if J[0] <= 0:
            # a sliver whose faces enclose no volume: flagged, the volume is still the definition's
            assert r["status"] == 2 and abs(r["volume"] - J[0]) <= 1e-12 * L ** 3, (k, r["status"], r["volume"], J[0])
            continue
        # com and inertia are ratios of sums in which the tetrahedra of a thin solid cancel: the tolerance follows that
        cond, fmag = tet_integrals.cond, tet_integrals.fmag
        vol, com, inertia = record_from_integrals(J, pos[0], rho)
        if require_ok:
            assert r["status"] == 0, (k, r["status"])
        assert abs(r["volume"] - vol) <= 1e-12 * L ** 3, (k, r["volume"], vol)
        assert abs(r["mass"] - rho * vol) <= 1e-12 * rho * L ** 3, k
        assert np.abs(r["com"] - com).max() <= 1e-12 * L * cond, (k, np.abs(r["com"] - com).max(), L, cond, r["volume"])
        tr = abs(inertia[:3].sum())
        assert np.abs(r["inertia"] - inertia).max() <= 1e-10 * tr * cond, (k, r["inertia"], inertia, cond)
        # the reference's own routine (float terms) agrees on the volume
        mv, _ = engine.moments(s)
        assert abs(r["volume"] - mv) <= 1e-5 * abs(vol) + fmag, (k, r["volume"], mv)


def solids_of(ev, pre):
    out = []
    vo, no = ev[pre + "_vert_off"], ev[pre + "_nbr_off"]
    for k in range(ev["frag_ids"].shape[0]):
        a, b = int(vo[k]), int(vo[k + 1])
        out.append({"pos": ev[pre + "_pos"][a:b], "off": (no[a:b + 1] - no[a]).astype(np.uint32), "nbr": ev[pre + "_nbr"][int(no[a]):int(no[b])]})
    return out


def run_scene(eng, sc, flags=engine.EVT_REFIT | engine.EVT_RENDER, cells=None):
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, sc["n_cells"] if cells is None else cells, flags=flags)
    return eng.download()


def regular_tetrahedron():
    p = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32)
    tris = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], np.int32)
    for t in (tris, tris[:, ::-1].copy()):
        s = engine.neighbors_from_mesh(p, t)
        if engine.moments(s)[0] > 0:
            return s
    raise AssertionError("no orientation with a positive volume")


ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])       # orthonormal, det 1


# ------------------------------------------------------------------ CPU tier (emulation)
def test_known_answers(emul_engine):
    box = scenes.box_solid((1, 1, 1), (0, 0, 0), factor=1.0)
    rot = dict(box, pos=(box["pos"].astype(np.float64) @ ROT.T).astype(np.float32))
    tet = regular_tetrahedron()
    eng = emul_engine.Engine(0)
    eng.load_fragments([box, rot, tet], [box, rot, tet])
    for s in (0, 1):
        rec = eng.event_mass(set=s, density=RHO)
        assert rec.shape == (3,) and (rec["status"] == 0).all()
        # unit box about its centre: volume 1, inertia rho/6 on the diagonal
        assert abs(rec[0]["volume"] - 1.0) < 1e-15 and np.abs(rec[0]["com"]).max() < 1e-15
        assert np.allclose(rec[0]["inertia"], [RHO / 6] * 3 + [0] * 3, rtol=0, atol=1e-14)
        # rotated: R I R^T (positions rounded to float: 1e-6)
        want = ROT @ tensor(rec[0]["inertia"]) @ ROT.T
        assert abs(rec[1]["volume"] - 1.0) < 1e-6 and np.abs(rec[1]["com"]).max() < 1e-6
        assert np.abs(tensor(rec[1]["inertia"]) - want).max() < 1e-5
        # regular tetrahedron of edge a = 2 sqrt 2: V = a^3 / (6 sqrt 2) = 8/3, I = m a^2 / 20 on the diagonal
        m = RHO * 8.0 / 3.0
        assert abs(rec[2]["volume"] - 8.0 / 3.0) < 1e-14 and np.abs(rec[2]["com"]).max() < 1e-15
        assert np.allclose(rec[2]["inertia"], [m * 8.0 / 20.0] * 3 + [0] * 3, rtol=1e-14, atol=1e-13)
    eng.close()


@pytest.mark.parametrize("scene", ["cube", "torus"])
def test_event_against_reference(emul_engine, scene):
    sc = scenes.cube_scene(8) if scene == "cube" else scenes.torus_scene(24)
    eng, ref = emul_engine.Engine(0), emul_engine.Engine(0)
    ev = run_scene(eng, sc)
    recs = {s: eng.event_mass(set=s) for s in (0, 1)}
    for s, pre in ((0, "mesh"), (1, "conv")):
        check_against_reference(ref, solids_of(ev, pre), recs[s])
    # the Mesh fragments partition the Mesh
    nv, J = ref_integrals(ref, sc["mesh"])
    whole = J[0]
    assert abs(recs[0]["volume"].sum() - whole) <= 1e-6 * abs(whole), (recs[0]["volume"].sum(), whole)
    eng.close(); ref.close()


@pytest.mark.parametrize("partial", [False, True])
def test_compounds(emul_engine, partial):
    sc = scenes.cube_scene(8)
    eng, ref = emul_engine.Engine(0), emul_engine.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, sc["n_cells"], flags=0)       # regroup runs on the un-refitted Convex solids
    ev = eng.download()
    kw = dict(partial=True, sphere_points=sc["mesh"]["pos"][::7], origin=sc["translate"], radius=0.4) if partial else {}
    co, cp = eng.event_regroup(**kw)
    for s, pre in ((0, "mesh"), (1, "conv")):
        rec = eng.event_mass(set=s)
        comp = engine.combine_mass(co, cp, rec)         # no piece was skipped: pieces = fragments
        assert comp.shape[0] == co.shape[0] - 1
        solids = solids_of(ev, pre)
        for c in range(comp.shape[0]):
            members = cp[co[c]:co[c + 1]]
            if members.size == 0:
                assert comp[c]["volume"] == 0 and comp[c]["mass"] == 0
                continue
            # all triangles of the compound at once, about one common origin
            origin = np.asarray(solids[members[0]]["pos"][0], np.float64)
            P, T, base = [], [], 0
            for p in members:
                sp = np.asarray(solids[p]["pos"], np.float64)
                fo, fi = ref.extract_faces(solids[p])
                for f in range(fo.shape[0] - 1):
                    loop = fi[fo[f]:fo[f + 1]]
                    loop = np.roll(loop, -int(np.argmin(loop)))
                    T += [(base + loop[0], base + loop[j], base + loop[j + 1]) for j in range(1, loop.shape[0] - 1)]
                P.append(sp - origin); base += sp.shape[0]
            J = tet_integrals(np.concatenate(P), np.asarray(T, np.int64))
            vol, com, inertia = record_from_integrals(J, origin)
            L = float(np.ptp(np.concatenate(P), axis=0).max())
            assert abs(comp[c]["volume"] - vol) <= 1e-12 * L ** 3
            assert np.abs(comp[c]["com"] - com).max() <= 1e-11 * L
            assert np.abs(comp[c]["inertia"] - inertia).max() <= 1e-10 * abs(inertia[:3].sum())
            assert comp[c]["nv"] == sum(solids[p]["pos"].shape[0] for p in members)
    eng.close(); ref.close()


def test_resident_pieces(emul_engine):
    sc = scenes.cube_scene(8)
    eng, ref = emul_engine.Engine(0), emul_engine.Engine(0)
    with pytest.raises(engine.SurtrError) as e:
        eng.pieces_mass()
    assert e.value.code == engine.E_STATE
    ev = run_scene(eng, sc)
    n = eng.pieces_from_event()
    meshes, convexes = scenes.fragments_as_pieces(ev)
    keep = [k for k in range(len(meshes)) if meshes[k]["pos"].shape[0] >= 4 and convexes[k]["pos"].shape[0] >= 4]
    assert n == len(keep)
    for s, solids in ((0, meshes), (1, convexes)):
        check_against_reference(ref, [solids[k] for k in keep], eng.pieces_mass(set=s))
    eng.close(); ref.close()


def test_edge_cases(emul_engine):
    eng = emul_engine.Engine(0)
    L = emul_engine.lib()
    # before any event
    with pytest.raises(engine.SurtrError) as e:
        eng.event_mass()
    assert e.value.code == engine.E_STATE
    buf = np.full(8 * 96, 0xAB, np.uint8)
    rc = L.surtr_event_mass_dev(eng._h, ctypes.c_int(1), ctypes.c_float(RHO), buf.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(buf.size))
    assert rc == engine.E_STATE and (buf == 0xAB).all()
    # a flat solid: zero volume, status 2
    box = scenes.box_solid((1, 1, 1), (0, 0, 0), factor=1.0)
    flat = scenes.box_solid((1, 1, 0), (0, 0, 0), factor=1.0)
    eng.load_fragments([box, flat, box], [box, flat, box])
    rec = eng.event_mass(set=1)
    assert list(rec["status"]) == [0, 2, 0] and rec[1]["volume"] == 0.0
    # a buffer one record too small: SURTR_E_CAPACITY, nothing written (the emulation's device memory is host memory)
    small = np.full(2 * 96, 0xAB, np.uint8)
    rc = L.surtr_event_mass_dev(eng._h, ctypes.c_int(1), ctypes.c_float(RHO), small.ctypes.data_as(ctypes.c_void_p), ctypes.c_size_t(small.size))
    assert rc == engine.E_CAPACITY and (small == 0xAB).all()
    n = ctypes.c_uint32(2)
    out = np.zeros(2, engine.MASS_DTYPE)
    assert L.surtr_event_mass(eng._h, ctypes.c_int(1), ctypes.c_float(RHO), ctypes.byref(n), out.ctypes.data_as(ctypes.c_void_p)) == engine.E_CAPACITY
    assert n.value == 3 and not out["nv"].any()
    # two calls: the same bits
    a, b = eng.event_mass(set=0), eng.event_mass(set=0)
    assert a.tobytes() == b.tobytes()
    eng.close()


def test_long_faces(emul_engine):
    """A prism over a 300-gon: its two caps are far longer than the walk bound and go through pointer jumping."""
    n = 300
    t = np.arange(n) * (2 * np.pi / n)
    ring = np.stack([np.cos(t), np.sin(t)], 1)
    pos = np.concatenate([np.c_[ring, np.zeros(n)], np.c_[ring, np.ones(n)]]).astype(np.float32)
    tris = []
    for i in range(n):
        j = (i + 1) % n
        tris += [(i, j, n + j), (i, n + j, n + i)]
    tris += [(0, j + 1, j) for j in range(1, n - 1)] + [(n, n + j, n + j + 1) for j in range(1, n - 1)]
    tris = np.asarray(tris, np.int32)
    # merge the cap triangles into one face each: rings of the caps' fans hold only the polygon's two neighbours + the wall
    s = engine.neighbors_from_mesh(pos, tris)
    if engine.moments(s)[0] < 0:
        s = engine.neighbors_from_mesh(pos, tris[:, ::-1].copy())
    capped = _drop_cap_diagonals(s, n)
    eng, ref = emul_engine.Engine(0), emul_engine.Engine(0)
    eng.load_fragments([capped], [capped])
    fo, _ = ref.extract_faces(capped)
    assert np.diff(fo).max() == n           # the caps are single faces
    for st in (0, 1):
        check_against_reference(ref, [capped], eng.event_mass(set=st))
    eng.close(); ref.close()


def _drop_cap_diagonals(s, n):
    """Keeps only the links of the prism's edges (polygon sides and walls): the caps become n-gons."""
    off, nbr = s["off"].astype(np.int64), s["nbr"]
    new_off, new_nbr = [0], []
    for v in range(2 * n):
        i = v % n
        keep = {(i + 1) % n + (v // n) * n, (i - 1) % n + (v // n) * n, (v + n) % (2 * n), ((i + 1) % n) + ((v // n) ^ 1) * n,
                ((i - 1) % n) + ((v // n) ^ 1) * n}
        r = [u for u in nbr[off[v]:off[v + 1]] if u in keep]
        new_nbr += r; new_off.append(len(new_nbr))
    return {"pos": s["pos"], "off": np.asarray(new_off, np.uint32), "nbr": np.asarray(new_nbr, np.int32)}


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys, numpy as np
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine, scenes
    import test_mass_properties as T
    case = sys.argv[1]
    sc = scenes.torus_scene(4096)
    if case == "torus":
        eng, ref = engine.Engine(0), engine.Engine(0)
        ev = T.run_scene(eng, sc)
        meshes, convexes = scenes.fragments_as_pieces(ev)
        kept = [k for k in range(len(meshes)) if meshes[k]["pos"].shape[0] >= 4 and convexes[k]["pos"].shape[0] >= 4]
        for s, solids in ((0, meshes), (1, convexes)):
            rec = eng.event_mass(set=s)
            T.check_against_reference(ref, solids, rec, require_ok=False)
            # every kept solid is ok, or a sliver of no volume (checked against the reference just above)
            bad = [k for k in kept if rec[k]["status"] != 0]
            print("set", s, "fragments", len(solids), "kept", len(kept), "flagged", [(k, int(rec[k]["status"]), rec[k]["volume"], int(rec[k]["nv"])) for k in bad])
            assert all(rec[k]["status"] == 2 and rec[k]["volume"] <= 0 for k in bad)
        n = eng.pieces_from_event()
        assert n == len(kept)
        for s, solids in ((0, meshes), (1, convexes)):
            T.check_against_reference(ref, [solids[k] for k in kept], eng.pieces_mass(set=s))
    elif case == "contexts":
        # two contexts on two streams with the in-flight hint at 6; the device call goes in right behind the asynchronous
        # event (no counts on the host yet), the host convenience comes after: every copy must carry the same bits
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        engs = [engine.Engine(0, stream=st.cuda_stream) for st in streams]
        cap = 1 << 16
        bufs = [[torch.full((cap * 96,), 0xAB, dtype=torch.uint8, device="cuda") for s in (0, 1)] for e in engs]
        torch.cuda.synchronize()
        for e, bb in zip(engs, bufs):
            e.set_events_in_flight(6)
            e.upload_pieces([sc["mesh"]], [sc["convex"]])
            e.upload_pattern(sc["face_off"], sc["v012"])
            e.place_cells(sc["scale"], sc["translate"])
            e.fracture_event_async(0, sc["n_cells"])
            for s in (0, 1):
                e.event_mass_dev(bb[s].data_ptr(), bb[s].numel(), set=s)
        torch.cuda.synchronize()
        for s in (0, 1):
            got = []
            for e, bb in zip(engs, bufs):
                n = e.event_counts().n_frag
                assert 0 < n < cap
                raw = bb[s].cpu().numpy()
                assert (raw[n * 96:] == 0xAB).all()
                got += [raw[:n * 96].tobytes(), e.event_mass(set=s).tobytes(), e.event_mass(set=s).tobytes()]
            assert all(g == got[0] for g in got), s
    print("ok", case)
""")


@pytest.mark.gpu
def test_gpu_torus_event_and_pieces():
    run_gpu_child(GPU_CHILD, "torus", 900)


@pytest.mark.gpu
def test_gpu_determinism_across_contexts():
    run_gpu_child(GPU_CHILD, "contexts", 300)
