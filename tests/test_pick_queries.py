"""Ray cast and sphere overlap on the Convex solids of the resident pieces (query_dev.hip) against a numpy float64 reference
written from the definition: faces from Engine.extract_faces rotated to their smallest vertex, the face plane through that vertex
and the two that follow it, Cyrus-Beck for rays, point-to-convex-polyhedron distance for spheres.

The reference reads the resident solids back with Engine.download_piece: the queries run on the pieces as they stand in HBM,
whatever put them there.  With L the scene's bounding-box diagonal, eps = 1e-5 L decides what float planes can tell apart and
1e-4 L is the tolerance of hit distances; at most 5 % of random rays (pairs) may be undecided, and that cap is checked on the
reference alone before the engine is looked at.

Scene (b): surtr_transform_pieces forgets the event, so the issue's order (transform, then pieces_from_event) is an error by the
C ABI; the piece is transformed before the event and every resident fragment once more after pieces_from_event, so a bound
kept from before either step would be stale.  The 64-cell scenes leave 46-51 resident pieces, fewer than a wave: scene (d), a
lattice of 306 turned boxes, covers several waves and several workgroups.
Scene (c): a solid of three vertices cannot become a resident piece -- surtr_upload_pieces and surtr_load_fragments both refuse
it (SURTR_E_INVALID), and a solid whose rings do not close is refused as well (SURTR_E_TOPOLOGY), which the test asserts; the
flagged solid that can be resident is a flat one (faces of zero normal).  The Convex of tests/golden/degenerate_sliver_convex.npz is the un-clipped box (no ring of it repeats an
entry, and its clip has no valid answer: SURTR_E_TOPOLOGY); the sliver Convex whose rings do list a neighbour twice is the one of
tests/golden/sliver_convex_walk_bound.npz, which is used.

The CPU tier runs on the one emulation library of tests/emul (conftest's emul_engine); the GPU tier runs the same scenes on the
MI355X in child processes under a time limit (helpers.run_gpu_child)."""
import ctypes
import json
import os
import subprocess
import textwrap

import numpy as np
import pytest

from helpers import run_gpu_child
from surtr_amd import engine, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 0.05          # undecided rays / pairs
ANGLE = 1e-3        # rad


# ------------------------------------------------------------------ numpy float64 reference
class RefSolid:
    """Planes (unit n, d; inside n.x + d <= 0), face loops and edges of one solid; ok = False where the definition has no answer."""

    def __init__(self, eng, solid):
        self.pos = np.asarray(solid["pos"], np.float32).reshape(-1, 3).astype(np.float64)
        off, nbr = np.asarray(solid["off"], np.int64), np.asarray(solid["nbr"], np.int64)
        nv = self.pos.shape[0]
        self.ok = nv >= 4
        self.loops, self.planes, self.edges = [], np.zeros((0, 4)), np.zeros((0, 2), np.int64)
        if not self.ok:
            return
        rings = [list(nbr[off[v]:off[v + 1]]) for v in range(nv)]
        # every ring entry names a vertex whose ring lists this one back: the walks close
        if any(w < 0 or w >= nv or v not in rings[w] for v in range(nv) for w in rings[v]) or any(len(r) == 0 for r in rings):
            self.ok = False
            return
        try:
            fo, fi = eng.extract_faces(solid)
        except engine.SurtrError:
            self.ok = False
            return
        planes = []
        for f in range(fo.shape[0] - 1):
            loop = np.asarray(fi[fo[f]:fo[f + 1]], np.int64)
            if loop.shape[0] < 3:
                self.ok = False
                return
            loop = np.roll(loop, -int(np.argmin(loop)))
            p0, p1, p2 = self.pos[loop[0]], self.pos[loop[1]], self.pos[loop[2]]
            n = np.cross(p1 - p0, p2 - p0)
            ln = np.linalg.norm(n)
            if not ln > 1e-30:
                self.ok = False
                return
            n = n / ln
            planes.append(np.r_[n, -n.dot(p0)])
            self.loops.append(loop)
        self.planes = np.asarray(planes)
        self.edges = np.asarray(sorted({(min(v, w), max(v, w)) for v in range(nv) for w in rings[v]}), np.int64)
        self.lo, self.hi = self.pos.min(0), self.pos.max(0)

    def ray(self, q):
        """None for a flagged solid; else dict(hit, t, t_exit, normal, inside, margin (miss: > 0), in_box)."""
        if not self.ok:
            return None
        o, d, md = q[:3], q[3:6], q[6]
        den = self.planes[:, :3] @ d
        dist = self.planes[:, :3] @ o + self.planes[:, 3]
        inside = bool((dist <= 0).all())
        t_in, t_ex, ent, rej = 0.0, md, -1, 0.0
        for k in range(den.shape[0]):
            if den[k] == 0:
                if dist[k] > 0:
                    rej = max(rej, dist[k])
                continue
            t = -dist[k] / den[k]
            if den[k] < 0:
                if dist[k] > 0 and (ent < 0 or t > t_in):
                    t_in, ent = t, k
            else:
                t_ex = min(t_ex, t)
        hit = rej == 0.0 and t_in <= t_ex and (inside or ent >= 0)
        # the box, for "a missed piece whose bound the ray crosses"
        a0, a1 = 0.0, md
        with np.errstate(divide="ignore", invalid="ignore"):
            for c in range(3):
                if d[c] == 0:
                    if o[c] < self.lo[c] or o[c] > self.hi[c]:
                        a1 = -1.0
                    continue
                a, b = sorted(((self.lo[c] - o[c]) / d[c], (self.hi[c] - o[c]) / d[c]))
                a0, a1 = max(a0, a), min(a1, b)
        in_box = a0 <= a1
        if hit and not in_box:      # a piece whose box the ray does not cross is not hit
            hit, miss = False, a0 - a1
        else:
            miss = max(rej, t_in - t_ex)
        return dict(hit=hit, t=0.0 if inside else t_in, t_exit=t_ex, inside=inside, in_box=in_box,
                    normal=-d if inside else (self.planes[ent, :3] if ent >= 0 else np.zeros(3)),
                    margin=min(t_ex - t_in, a1 - a0) if hit else miss)

    def dist(self, c):
        """Distance from c to the solid (None: flagged)."""
        if not self.ok:
            return None
        box = float(np.linalg.norm(np.maximum(0.0, np.maximum(self.lo - c, c - self.hi))))
        return max(box, self._dist(c))      # a piece whose box the sphere does not reach is not touched

    def _dist(self, c):
        d = self.planes[:, :3] @ c + self.planes[:, 3]
        if (d <= 0).all():
            return 0.0
        a, b = self.pos[self.edges[:, 0]], self.pos[self.edges[:, 1]]
        e, h = b - a, c - a
        ee = (e * e).sum(1)
        s = np.clip(np.where(ee > 0, (e * h).sum(1) / np.where(ee > 0, ee, 1.0), 0.0), 0.0, 1.0)
        best = float(np.sqrt((((h - s[:, None] * e) ** 2).sum(1)).min()))
        for k in np.nonzero(d > 0)[0]:
            if d[k] >= best:
                continue
            n, loop = self.planes[k, :3], self.loops[k]
            qp = c - d[k] * n
            P = self.pos[loop]
            E = np.roll(P, -1, axis=0) - P
            if (np.cross(E, qp - P) @ n >= 0).all():
                best = float(d[k])
        return best


def resident_reference(eng, ref_eng, n):
    return [RefSolid(ref_eng, eng.download_piece(p, set=1)) for p in range(n)]


def scene_size(refs):
    lo = np.min([r.pos.min(0) for r in refs], axis=0)
    hi = np.max([r.pos.max(0) for r in refs], axis=0)
    return lo, hi, float(np.linalg.norm(hi - lo))


def ref_ray(refs, q, eps):
    """(expected record, decided, acceptable) for one ray: acceptable(piece, t) says whether an undecided ray's answer is one of
    the near-tied ones."""
    res = [r.ray(q) for r in refs]
    hits = [(a["t"], p) for p, a in enumerate(res) if a is not None and a["hit"]]
    hits.sort()
    decided = True
    for p, a in enumerate(res):
        if a is not None and not a["hit"] and a["in_box"] and a["margin"] <= eps:
            decided = False
    if hits:
        t, p = hits[0]
        if res[p]["margin"] <= eps or (len(hits) > 1 and hits[1][0] - t <= eps):
            decided = False
        exp = dict(piece=p, t=t, pos=q[:3] + t * q[3:6], normal=res[p]["normal"], inside=res[p]["inside"])
    else:
        exp = dict(piece=-1)
    sure = [t for t, p in hits if res[p]["margin"] > eps]
    limit = (min(sure) if sure else np.inf) + eps

    def acceptable(piece, t, tol):
        if piece < 0:
            return not sure
        a = res[piece]
        if a is None or not (a["hit"] or a["margin"] <= eps):
            return False
        return a["t"] <= limit and abs(t - a["t"]) <= tol + eps
    return exp, decided, acceptable


def check_rays(refs, rays, got, L, undecided_cap=None):
    eps, tol = 1e-5 * L, 1e-4 * L
    und = 0
    for i, q in enumerate(np.asarray(rays, np.float64)):
        exp, decided, acceptable = ref_ray(refs, q, eps)
        g = got[i]
        assert not (g["reserved"].any()), i
        if not decided:
            und += 1
            assert acceptable(int(g["piece"]), float(g["t"]), tol), (i, g, exp)
            continue
        assert g["piece"] == exp["piece"], (i, g, exp)
        if exp["piece"] < 0:
            assert g["status"] == 0 and g["t"] == 0, (i, g)
            continue
        assert abs(g["t"] - exp["t"]) <= tol, (i, g["t"], exp["t"])
        assert np.linalg.norm(g["pos"] - exp["pos"]) <= tol, (i, g["pos"], exp["pos"])
        assert int(g["status"]) == (engine.RAY_STARTS_INSIDE if exp["inside"] else 0), (i, g, exp)
        n = g["normal"].astype(np.float64)
        cosang = n.dot(exp["normal"]) / (np.linalg.norm(n) * np.linalg.norm(exp["normal"]))
        assert np.arccos(min(1.0, cosang)) <= ANGLE, (i, n, exp["normal"])
        if exp["inside"]:
            assert g["t"] == 0 and (g["pos"] == np.asarray(q[:3], np.float32)).all(), (i, g)
    if undecided_cap is not None:
        assert und <= undecided_cap * len(rays), (und, len(rays))
    return und


def count_undecided_rays(refs, rays, L):
    return sum(0 if ref_ray(refs, q, 1e-5 * L)[1] else 1 for q in np.asarray(rays, np.float64))


def random_rays(lo, hi, L, n=256, seed=20261017):
    """Origins on a sphere around the scene, aimed at seeded points inside the box."""
    rng = np.random.default_rng(seed)
    c = (lo + hi) / 2
    u = rng.normal(size=(n, 3))
    o = c + u / np.linalg.norm(u, axis=1)[:, None] * L
    tgt = lo + rng.random((n, 3)) * (hi - lo)
    d = tgt - o
    d /= np.linalg.norm(d, axis=1)[:, None]
    return np.c_[o, d, np.full(n, 4 * L)].astype(np.float32)


def designed_rays(refs, lo, hi, L):
    """+x through the centre; from inside a piece; away from everything; max_dist just short of / just past the hit; parallel to
    a face just outside / just inside it."""
    c = (lo + hi) / 2
    big = 4 * L

    def f32(q):
        return np.asarray(q, np.float32).astype(np.float64)

    def hits(q):
        return [a for a in (r.ray(f32(q)) for r in refs) if a is not None and a["hit"]]
    out = [np.r_[c - [L, 0, 0], [1, 0, 0], big]]
    first = next(r for r in refs if r.ok)
    if not hits(out[0]):      # a sparse scene: +x through its first piece
        out[0] = np.r_[first.pos.mean(0) - [L, 0, 0], [1, 0, 0], big]
    # from inside a piece: the first whose vertex mean the reference finds inside it
    inner = next(r for r in refs if r.ok and r.ray(f32(np.r_[r.pos.mean(0), [0, 0, 1], big]))["inside"])
    out.append(np.r_[inner.pos.mean(0), [0, 0, 1], big])
    out.append(np.r_[c - [L, 0, 0], [-1, 0, 0], big])
    q = np.asarray(out[0], np.float32).astype(np.float64)
    t = min(a["t"] for a in (r.ray(q) for r in refs) if a is not None and a["hit"])
    out.append(np.r_[q[:6], t - 1e-3 * L])
    out.append(np.r_[q[:6], t + 1e-3 * L])
    n, loop = first.planes[0, :3], first.loops[0]
    fc = first.pos[loop].mean(0)
    d = first.pos[loop[1]] - first.pos[loop[0]]
    d /= np.linalg.norm(d)
    for s in (1e-3, -1e-3):
        out.append(np.r_[fc + n * s * L - d * L, d, big])
    return np.asarray(out, np.float32)


def random_spheres(lo, hi, L, n=32, seed=4242):
    rng = np.random.default_rng(seed)
    c = lo - 0.1 * (hi - lo) + rng.random((n, 3)) * 1.2 * (hi - lo)
    return np.c_[c, rng.random(n) * 0.25 * L].astype(np.float32)


def designed_spheres(refs, lo, hi, L):
    first = next(r for r in refs if r.ok and r.dist(np.asarray(r.pos.mean(0), np.float32).astype(np.float64)) == 0.0)
    c = (lo + hi) / 2
    return np.asarray([np.r_[first.pos.mean(0), 0.01 * L], np.r_[first.pos.mean(0), 0.0], np.r_[c, 2 * L], np.r_[c + 10 * L, 0.1 * L]], np.float32)


def ref_mask(refs, spheres, L, mass=None, min_mass=None):
    """(expected mask, decided mask)."""
    eps = 1e-5 * L
    sp = np.asarray(spheres, np.float32).astype(np.float64)
    exp = np.zeros((sp.shape[0], len(refs)), np.uint8)
    dec = np.ones(exp.shape, bool)
    for s in range(sp.shape[0]):
        for p, r in enumerate(refs):
            d = r.dist(sp[s, :3])
            if d is None:
                continue
            dec[s, p] = abs(d - sp[s, 3]) > eps
            if d <= sp[s, 3]:
                exp[s, p] = 2 if (mass is not None and mass[p]["mass"] <= float(np.float32(min_mass))) else 1
    return exp, dec


def check_mask(exp, dec, got):
    assert got.shape == exp.shape and got.dtype == np.uint8
    assert (got[dec] == exp[dec]).all(), np.argwhere(dec & (got != exp))[:8]
    # an undecided pair: touched or not, and the gate's value when touched
    und = ~dec
    assert np.isin(got[und], (0, 1, 2)).all() and ((got[und] == 0) | (exp[und] == 0) | (got[und] == exp[und])).all()


# ------------------------------------------------------------------ scenes
ROT = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]])       # orthonormal, det 1


def world(rot, shift):
    """WorldMatrix of x -> rot x + shift as the reference stores it (used transposed: the translation is the last column)."""
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = np.asarray(rot, np.float32)
    m[:3, 3] = np.asarray(shift, np.float32)
    return m


def scene_a(E):
    """The 8-cell cube after one event + pieces_from_event: the pieces exist only in HBM and share faces."""
    sc = scenes.cube_scene(n_cells=8)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, sc["n_cells"])
    return eng, eng.pieces_from_event()


def scene_b(E):
    """The 64-cell blob: the piece moved before the event, every fragment moved again once resident (bounds from before are
    stale, many planes per solid)."""
    sc = scenes.blob_scene(64)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    ang = 0.2
    rz = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1]])
    cen = np.asarray(sc["translate"], np.float64)
    eng.transform_pieces([world(rz, cen - rz @ cen)])
    eng.fracture_event(0, sc["n_cells"])
    n = eng.pieces_from_event()
    assert n > 32
    rng = np.random.default_rng(7)
    eng.transform_pieces([world(ROT, [150.0, -40.0, 25.0] + rng.normal(size=3) * 2.0) for _ in range(n)])
    return eng, n


def regular_tetrahedron(shift=(0, 0, 0)):
    p = np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32) + np.asarray(shift, np.float32)
    tris = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 1], [1, 3, 2]], np.int32)
    for t in (tris, tris[:, ::-1].copy()):
        s = engine.neighbors_from_mesh(p, t)
        if engine.moments(s)[0] > 0:
            return s
    raise AssertionError("no orientation with a positive volume")


def hand_made():
    """tetrahedron | sliver Convex with a repeated ring entry | flat tetrahedron (faces of zero normal) | tetrahedron."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "sliver_convex_walk_bound.npz"))
    sliver = {"pos": g["conv_pos"] + np.float32([6, 0, 0]), "off": g["conv_off"], "nbr": g["conv_nbr"]}
    assert any(len(set(r)) < len(r) for r in (list(sliver["nbr"][sliver["off"][v]:sliver["off"][v + 1]]) for v in range(sliver["pos"].shape[0])))
    tet = regular_tetrahedron()
    flat = dict(regular_tetrahedron((0, 0, 6)))
    flat["pos"] = flat["pos"].copy()
    flat["pos"][:, 2] = 6.0
    flat["pos"][3] = flat["pos"][2]                         # two coincident vertices: faces of zero normal
    return [tet, sliver, flat, regular_tetrahedron((-6, 0, 0))]


def scene_c(E):
    solids = hand_made()
    eng = E.Engine(0)
    eng.load_fragments(solids, solids)
    n = eng.pieces_from_event(keep=np.ones(len(solids), np.uint8))
    assert n == len(solids)
    return eng, n


def scene_d(E):
    """306 separate boxes of several sizes, turned, on a jittered lattice: more pieces than one wave and than one workgroup takes
    (the 64-cell scenes leave fewer than 64 resident pieces)."""
    rng = np.random.default_rng(11)
    solids = []
    for i in range(17):
        for j in range(6):
            for k in range(3):
                b = scenes.box_solid(0.4 + 0.5 * rng.random(3), (0, 0, 0), factor=1.0)
                c = np.array([2.5 * i, 2.5 * j, 2.5 * k]) + rng.random(3) * 0.6
                solids.append(dict(b, pos=(b["pos"].astype(np.float64) @ ROT.T + c).astype(np.float32)))
    eng = E.Engine(0)
    eng.upload_pieces(solids, solids)
    return eng, len(solids)


SCENES = {"a": scene_a, "b": scene_b, "c": scene_c, "d": scene_d}


def run_scene_checks(E, name, dev_forms=None):
    """Everything the issue lists for one scene; dev_forms(eng, rays, spheres, mass, min_mass) -> (hits, mask) or None."""
    eng, n = SCENES[name](E)
    ref_eng = E.Engine(0)
    refs = resident_reference(eng, ref_eng, n)
    lo, hi, L = scene_size(refs)
    rays = np.concatenate([random_rays(lo, hi, L), designed_rays(refs, lo, hi, L)])
    # the cap, on the reference alone
    assert count_undecided_rays(refs, rays[:256], L) <= CAP * 256
    spheres = np.concatenate([random_spheres(lo, hi, L), designed_spheres(refs, lo, hi, L)])
    mass = eng.pieces_mass(set=1)
    min_mass = float(np.median(mass["mass"]))
    exp_plain, dec = ref_mask(refs, spheres, L)
    exp_gate, _ = ref_mask(refs, spheres, L, mass, min_mass)
    assert (~dec).sum() <= CAP * dec.size

    got = eng.pieces_raycast(rays)
    print("scene", name, "pieces", n, "L", L, "undecided rays", check_rays(refs, rays[:256], got[:256], L, CAP),
          "undecided pairs", int((~dec).sum()), "of", dec.size)
    check_rays(refs, rays[256:], got[256:], L)
    status = eng.pieces_query_status(n)
    assert [bool(s) for s in status] == [not r.ok for r in refs], (status, [r.ok for r in refs])
    flagged = [p for p, r in enumerate(refs) if not r.ok]
    assert not np.isin(got["piece"], flagged).any()
    # designed rays: away from everything -> none; max_dist just short -> not the hit just past gives
    d = got[256:]
    assert d[0]["piece"] >= 0 and d[1]["status"] == engine.RAY_STARTS_INSIDE and d[2]["piece"] == -1
    assert d[4]["piece"] == d[0]["piece"] and not (d[3]["piece"] == d[0]["piece"] and d[3]["t"] == d[0]["t"])
    # the wave boundaries, and twice the same bits
    for k in (1, 63, 64, 65):
        assert eng.pieces_raycast(rays[:k]).tobytes() == got[:k].tobytes(), k
    assert eng.pieces_raycast(rays).tobytes() == got.tobytes()

    m0 = eng.pieces_overlap(spheres)
    check_mask(exp_plain, dec, m0)
    m1 = eng.pieces_overlap(spheres, mass=mass, min_mass=min_mass)
    check_mask(exp_gate, dec, m1)
    assert ((m1 != 0) == (m0 != 0)).all() and (m1 == 2).any() == bool((exp_gate == 2).any())
    ok = np.array([r.ok for r in refs])
    k = len(spheres) - 4
    assert (m0[k + 2][ok] == 1).all() and not m0[k + 2][~ok].any() and not m0[k + 3].any() and m0[k].any() and m0[k + 1].any()
    assert not m0[:, ~ok].any()
    assert eng.pieces_overlap(spheres, mass=mass, min_mass=min_mass).tobytes() == m1.tobytes()
    assert (eng.pieces_query_status(n) == status).all()
    if dev_forms is not None:
        h2, k0, k1 = dev_forms(eng, n, rays, spheres, mass, min_mass)
        assert h2.tobytes() == got.tobytes() and k0.tobytes() == m0.tobytes() and k1.tobytes() == m1.tobytes()
        eng.set_events_in_flight(6)
        assert eng.pieces_raycast(rays).tobytes() == got.tobytes()
        assert eng.pieces_overlap(spheres, mass=mass, min_mass=min_mass).tobytes() == m1.tobytes()
    eng.close(); ref_eng.close()
    return got, m0, m1


# ------------------------------------------------------------------ CPU tier (emulation)
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_scene_against_reference(emul_engine, name):
    run_scene_checks(emul_engine, name)


def test_flagged_solids_and_their_neighbours(emul_engine):
    """Scene (c) in detail: status per solid; the sound tetrahedra answer as they do alone."""
    eng, n = scene_c(emul_engine)
    solids = hand_made()
    rays = np.asarray([[-10, 0.1, 0.05, 1, 0, 0, 100], [0.3, 0.1, 0, 0, 0, 1, 100], [0.1, 0.05, 20, 0, 0, -1, 100], [6.2, 0.1, -20, 0, 0, 1, 100]], np.float32)
    got = eng.pieces_raycast(rays)
    st = eng.pieces_query_status(n)
    assert st[0] == 0 and st[3] == 0 and st[2] == engine.QUERY_FLAT, st
    # through the far tetrahedron first; from inside the first, past the flat solid at z = 6 without a hit
    assert got[0]["piece"] == 3 and got[1]["piece"] == 0 and got[1]["status"] == engine.RAY_STARTS_INSIDE and got[2]["piece"] == 0, got
    assert not eng.pieces_overlap([[0, 0, 6, 3]])[0][2] and eng.pieces_overlap([[0, 0, 6, 30]])[0].tolist() == [1, 1, 0, 1]
    alone = emul_engine.Engine(0)
    alone.load_fragments([solids[0], solids[3]], [solids[0], solids[3]])
    alone.pieces_from_event(keep=np.ones(2, np.uint8))
    ga = alone.pieces_raycast(rays)
    for a, b in zip(got, ga):
        assert (int(a["piece"]), int(b["piece"])) in ((0, 0), (3, 1), (-1, -1), (1, -1)) and (a["piece"] == 1 or a.tobytes()[4:] == b.tobytes()[4:])
    # rings that do not close cannot become resident: vertex 0 lists one neighbour three times
    broken = dict(regular_tetrahedron((0, 6, 0)))
    nb = broken["nbr"].copy()
    nb[0:3] = [1, 1, 1] if nb[0] != 1 else [2, 2, 2]
    broken["nbr"] = nb
    with pytest.raises(engine.SurtrError) as e:
        alone.load_fragments([solids[0], broken], [solids[0], broken])
    assert e.value.code == engine.E_TOPOLOGY
    # a solid of three vertices cannot become resident, by either route
    tri = {"pos": solids[0]["pos"][:3], "off": np.array([0, 2, 4, 6], np.uint32), "nbr": np.array([1, 2, 2, 0, 0, 1], np.int32)}
    with pytest.raises(engine.SurtrError) as e:
        alone.upload_pieces([solids[0], tri], [solids[0], tri])
    assert e.value.code == engine.E_INVALID
    with pytest.raises(engine.SurtrError) as e:
        alone.load_fragments([solids[0], tri], [solids[0], tri])
    assert e.value.code == engine.E_INVALID
    eng.close(); alone.close()


def test_known_answers(emul_engine):
    """A unit box about the origin: hit distances, normals, positions and the sphere distances are known exactly."""
    box = scenes.box_solid((1, 1, 1), (0, 0, 0), factor=1.0)
    far = scenes.box_solid((1, 1, 1), (4, 0, 0), factor=1.0)
    eng = emul_engine.Engine(0)
    eng.upload_pieces([box, far], [box, far])
    rays = np.asarray([[-3, 0.1, 0.2, 1, 0, 0, 100], [8, 0.1, 0.2, -1, 0, 0, 100], [0.1, 0.2, 5, 0, 0, -1, 100], [0, 0, 0, 0, 1, 0, 100],
                       [-3, 0.1, 0.2, 1, 0, 0, 2.4], [-3, 0.1, 0.2, 1, 0, 0, 2.5], [-3, 0.5, 0, 1, 0, 0, 100], [-3, 0.75, 0, 1, 0, 0, 100],
                       [-3, 0, 0, 0, 1, 0, np.inf]], np.float32)
    g = eng.pieces_raycast(rays)
    assert list(g["piece"]) == [0, 1, 0, 0, -1, 0, 0, -1, -1]
    assert list(g["t"][:4]) == [2.5, 3.5, 4.5, 0.0] and g["t"][5] == 2.5
    assert (g["normal"][0] == [-1, 0, 0]).all() and (g["normal"][1] == [1, 0, 0]).all() and (g["normal"][2] == [0, 0, 1]).all()
    assert (g["normal"][3] == [0, -1, 0]).all() and g["status"][3] == engine.RAY_STARTS_INSIDE and not g["status"][[0, 1, 2, 5]].any()
    assert np.allclose(g["pos"][0], [-0.5, 0.1, 0.2]) and np.allclose(g["pos"][1], [4.5, 0.1, 0.2])
    sp = np.asarray([[0, 0, 0, 0], [2, 0, 0, 1.4], [2, 0, 0, 1.6], [1.5, 1.5, 0, 1.4], [1.5, 1.5, 0, 1.42], [2, 0, 0, 1.5]], np.float32)
    m = eng.pieces_overlap(sp)
    assert m.tolist() == [[1, 0], [0, 0], [1, 1], [0, 0], [1, 0], [1, 1]]
    mass = eng.pieces_mass(set=1)
    assert eng.pieces_overlap(sp, mass=mass, min_mass=20.0).tolist() == [[2, 0], [0, 0], [2, 2], [0, 0], [2, 0], [2, 2]]
    assert eng.pieces_overlap(sp, mass=mass).tolist() == m.tolist()
    eng.close()


def test_errors_and_dev_forms(emul_engine):
    L_ = emul_engine.lib()
    eng = emul_engine.Engine(0)
    ray = np.asarray([[-3, 0, 0, 1, 0, 0, 100]], np.float32)
    for call in (lambda: eng.pieces_raycast(ray), lambda: eng.pieces_overlap([[0, 0, 0, 1]]), lambda: eng.pieces_query_status(1)):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == engine.E_STATE
    box = scenes.box_solid((1, 1, 1), (0, 0, 0), factor=1.0)
    eng.upload_pieces([box], [box])
    for bad in ([0, 0, 0, 0, 0, 0, 1], [0, 0, 0, np.nan, 0, 1, 1], [0, 0, 0, 1, 0, 0, -1], [np.inf, 0, 0, 1, 0, 0, 1]):
        with pytest.raises(engine.SurtrError) as e:
            eng.pieces_raycast(np.asarray([ray[0], bad], np.float32))
        assert e.value.code == engine.E_INVALID
    with pytest.raises(engine.SurtrError) as e:
        eng.pieces_overlap([[0, 0, 0, -1]])
    assert e.value.code == engine.E_INVALID
    # the device forms (the emulation's device memory is host memory): a bad ray is a status bit, a small buffer is refused
    rays = np.asarray([ray[0], [0, 0, 0, 0, 0, 0, 1], ray[0]], np.float32)
    hits = np.zeros(3, engine.RAY_HIT_DTYPE)
    eng.pieces_raycast_dev(3, rays.ctypes.data, hits.ctypes.data, hits.nbytes)
    assert list(hits["piece"]) == [0, -1, 0] and list(hits["status"]) == [0, engine.RAY_INVALID, 0] and hits[0].tobytes() == hits[2].tobytes()
    small = np.full(2 * 48, 0xAB, np.uint8)
    rc = L_.surtr_pieces_raycast_dev(eng._h, ctypes.c_uint32(3), ctypes.c_void_p(rays.ctypes.data), ctypes.c_void_p(small.ctypes.data), ctypes.c_size_t(small.size))
    assert rc == engine.E_CAPACITY and (small == 0xAB).all()
    sp = np.asarray([[0, 0, 0, 1], [9, 9, 9, 1]], np.float32)
    mask = np.full(2, 0xAB, np.uint8)
    eng.pieces_overlap_dev(2, sp.ctypes.data, mask.ctypes.data, 2)
    assert list(mask) == [1, 0]
    mask[:] = 0xAB
    rc = L_.surtr_pieces_overlap_dev(eng._h, ctypes.c_uint32(2), ctypes.c_void_p(sp.ctypes.data), None, ctypes.c_float(0), ctypes.c_void_p(mask.ctypes.data), ctypes.c_size_t(1))
    assert rc == engine.E_CAPACITY and (mask == 0xAB).all()
    with pytest.raises(engine.SurtrError) as e:
        eng.pieces_query_status(0)
    assert e.value.code == engine.E_CAPACITY
    eng.close()


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import json, subprocess, sys, numpy as np
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine, scenes
    import test_pick_queries as T
    case = sys.argv[1]

    def dev_forms(eng, n, rays, spheres, mass, min_mass):
        # the _dev forms on a stream of their own
        st = torch.cuda.Stream()
        eng.set_stream(st.cuda_stream)
        with torch.cuda.stream(st):
            d_r = torch.from_numpy(rays).cuda(); d_s = torch.from_numpy(spheres).cuda()
            d_h = torch.zeros(rays.shape[0] * 48, dtype=torch.uint8, device="cuda")
            d_m = [torch.zeros(spheres.shape[0] * n, dtype=torch.uint8, device="cuda") for _ in (0, 1)]
            d_w = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
            st.synchronize()
            eng.pieces_mass_dev(d_w.data_ptr(), d_w.numel(), set=1)
            eng.pieces_raycast_dev(rays.shape[0], d_r.data_ptr(), d_h.data_ptr(), d_h.numel())
            eng.pieces_overlap_dev(spheres.shape[0], d_s.data_ptr(), d_m[0].data_ptr(), d_m[0].numel())
            eng.pieces_overlap_dev(spheres.shape[0], d_s.data_ptr(), d_m[1].data_ptr(), d_m[1].numel(), dev_mass=d_w.data_ptr(), min_mass=min_mass)
            st.synchronize()
        assert d_w.cpu().numpy().tobytes() == mass.tobytes()
        return (d_h.cpu().numpy().view(engine.RAY_HIT_DTYPE), d_m[0].cpu().numpy().reshape(-1, n), d_m[1].cpu().numpy().reshape(-1, n))

    if case in ("a", "b", "c", "d"):
        T.run_scene_checks(engine, case, dev_forms)
    elif case == "harness":
        T.check_harness(engine, %(root)r)
    print("ok", case)
""")


def check_harness(E, root, exe=None):
    """surtr_harness --pick on scene (a) against Engine.pieces_raycast / pieces_overlap, and PickImpact's contract."""
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    o, d = [-10.0, 0.3, 0.2], [1.0, 0.0, 0.0]
    p = subprocess.run([exe, "--mesh", "cube", "--cells", "8", "--pick", ",".join("%r" % x for x in o + d), "--impact-radius", "3.0"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
    js = json.loads(p.stdout.strip().splitlines()[-1])["pick"]
    eng, n = scene_a(E)
    assert js["pieces"] == n
    hit = eng.pieces_raycast([o + d + [1e30]])[0]
    assert js["raycast"]["piece"] == hit["piece"] >= 0 and np.float32(js["raycast"]["t"]) == hit["t"]
    assert (np.asarray(js["raycast"]["pos"], np.float32) == hit["pos"]).all() and (np.asarray(js["raycast"]["normal"], np.float32) == hit["normal"]).all()
    # ImpactPosition = hit + dir * TargetAdder (0.01), in float
    imp = (hit["pos"] + np.asarray(d, np.float32) * np.float32(0.01)).astype(np.float32)
    assert (np.asarray(js["impact_position"], np.float32) == imp).all()
    mass = eng.pieces_mass(set=1)
    m = eng.pieces_overlap([list(imp) + [1.5]], mass=mass, min_mass=1e-4)[0]
    assert js["overlap"] == [int(x) for x in m]
    # the harness's compounds: piece k in compound k // 2
    assert js["radial"] == sorted({int(k) // 2 for k in np.nonzero(m == 1)[0]})
    assert js["single"] == [int(hit["piece"]) // 2]
    # ConvexRayIntersection (host) on the hit piece agrees with the device
    assert js["host_ray"]["hit"] is True and abs(js["host_ray"]["dist"] - float(hit["t"])) <= 1e-4 * 20
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a", "b", "c", "d"])
def test_gpu_scene_against_reference(name):
    run_gpu_child(GPU_CHILD, name, 120)


@pytest.mark.gpu
def test_gpu_harness_pick():
    run_gpu_child(GPU_CHILD, "harness", 150)
