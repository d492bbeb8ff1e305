"""Per-body poses on the resident scene (scene_dev.hip, query_dev.hip, mass_dev.hip): a rigid pose per compound, ray cast and sphere
overlap that honour it on the device, the overlap gated per body by a body mass taken on the device, the pose baked into the pieces
before an event, and the commit carrying the poses along.

References, none of which runs the code under test:
 * queries -- the numpy float64 reference of test_pick_queries.py (RefSolid) on the downloaded solids, asked per piece in that
   piece's body frame: the world ray or sphere is taken there with A^T in float64, the expected normal is A n';
 * baking -- a second engine that calls surtr_scene_transform_compound / surtr_transform_pieces, which existed before the poses;
 * body mass -- engine.combine_mass (host) over pieces_mass, byte for byte;
 * the click loop -- the two references of test_scene.py (its click helper checks both).
Tolerances are test_pick_queries.py's, with L the posed scene's box diagonal: eps = 1e-5 L decides what float planes can tell apart,
distances 1e-4 L, normals 1e-3 rad; at most 5 % of the random rays / (sphere, piece) pairs may be undecided, asserted on the
reference alone before the engine is looked at.

The lattice is test_pick_queries.scene_d's 306 boxes in compounds of 1, 2, 61, 64, 65, 70 and 43 pieces: boundaries at a wave edge
(64, 128) and one short of / past one, a compound that straddles piece 256 (the second workgroup of the ray kernel).  Every compound
but one is turned about an axis of its own through its centre and moved 24 units away from the one left at the identity.

The CPU tier runs on the one emulation library of tests/emul (conftest's emul_engine); the GPU tier runs the same functions on the
MI355X in child processes under a time limit (helpers.run_gpu_child), plus the _dev forms, two contexts and the harness."""
import ctypes
import json
import os
import subprocess
import textwrap

import numpy as np
import pytest

from helpers import run_gpu_child
from surtr_amd import engine, scenes

import test_pick_queries as PQ
import test_scene as TS

SIZES = [1, 2, 61, 64, 65, 70, 43]
TABLE = np.cumsum([0] + SIZES).astype(np.uint32)
AT_REST = 3                                   # the compound left at the identity
OFFSETS = [(-24, 0, 0), (24, 0, 0), (0, -24, 0), (0, 0, 0), (0, 24, 0), (0, 0, -24), (0, 0, 24)]
AXES = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, 1, 0), (0, 1, 1), (1, 0, 1)]
ANGLES = [0.4, -0.7, 1.1, 0.0, 2.0, -1.3, 0.25]
CAP = PQ.CAP


# ------------------------------------------------------------------ poses and the posed reference
def rotation(axis, angle):
    """Rodrigues in float64."""
    u = np.asarray(axis, np.float64)
    u = u / np.linalg.norm(u)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose_about(rot, centre, shift):
    """x -> rot (x - centre) + centre + shift, rounded to float."""
    centre = np.asarray(centre, np.float64)
    return PQ.world(rot, centre - rot @ centre + np.asarray(shift, np.float64))


def split(W):
    """(A, b) in float64 from the float matrix."""
    W = np.asarray(W, np.float32).astype(np.float64).reshape(4, 4)
    return W[:3, :3], W[:3, 3]


class PosedRef:
    """A RefSolid of test_pick_queries.py behind a pose: asked in its body frame, answers in the world.
    A ray that passes the sphere about the solid's box at more than `slack` (set to 10 eps once L is known) is answered without the
    walk over the planes: no hit, the box not crossed -- which is what the walk would say, 300 times per ray, in Python."""

    def __init__(self, ref, W):
        self.ref, self.ok = ref, ref.ok
        self.A, self.b = split(W)
        self.pos = ref.pos @ self.A.T + self.b
        self.slack = np.inf
        if ref.ok:
            self.centre = tuple(float(x) for x in self.A @ ((ref.lo + ref.hi) / 2) + self.b)
            self.radius = float(np.linalg.norm(ref.hi - ref.lo)) / 2

    def ray(self, q):
        if self.ok and self.slack < np.inf:
            ox, oy, oz, dx, dy, dz, md = q.tolist()
            vx, vy, vz = self.centre[0] - ox, self.centre[1] - oy, self.centre[2] - oz
            t = min(max((vx * dx + vy * dy + vz * dz) / (dx * dx + dy * dy + dz * dz), 0.0), md)
            gap = ((vx - t * dx) ** 2 + (vy - t * dy) ** 2 + (vz - t * dz) ** 2) ** 0.5 - self.radius
            if gap > self.slack:
                return dict(hit=False, t=0.0, t_exit=md, inside=False, in_box=False, normal=np.zeros(3), margin=gap)
        a = self.ref.ray(np.r_[self.A.T @ (q[:3] - self.b), self.A.T @ q[3:6], q[6]])
        return None if a is None else dict(a, normal=self.A @ a["normal"])

    def dist(self, c):
        return self.ref.dist(self.A.T @ (np.asarray(c, np.float64) - self.b))


def compound_of_piece(table):
    return np.repeat(np.arange(len(table) - 1), np.diff(np.asarray(table, np.int64)))


_LAT = {}


def lattice(E):
    """The reference side of the posed lattice, computed once and left unchanged: unposed and posed references, poses, rays and
    spheres with what the reference expects of them.  The caps are asserted here, before any engine answers."""
    if _LAT:
        return _LAT
    eng, n = PQ.scene_d(E)
    assert n == int(TABLE[-1])
    ref_eng = E.Engine(0)
    plain = PQ.resident_reference(eng, ref_eng, n)
    eng.close(); ref_eng.close()
    comp = compound_of_piece(TABLE)
    poses = []
    for c in range(len(SIZES)):
        cen = np.concatenate([plain[p].pos for p in range(TABLE[c], TABLE[c + 1])]).mean(0)
        poses.append(np.eye(4, dtype=np.float32) if c == AT_REST else pose_about(rotation(AXES[c], ANGLES[c]), cen, OFFSETS[c]))
    poses = np.asarray(poses, np.float32)
    assert (poses[AT_REST] == np.eye(4)).all()
    refs = [PosedRef(plain[p], poses[comp[p]]) for p in range(n)]
    # the bodies are apart: their world boxes are disjoint
    box = [(np.min([refs[p].pos.min(0) for p in range(TABLE[c], TABLE[c + 1])], 0), np.max([refs[p].pos.max(0) for p in range(TABLE[c], TABLE[c + 1])], 0))
           for c in range(len(SIZES))]
    for a in range(len(SIZES)):
        for b in range(a):
            assert (box[a][0] > box[b][1]).any() or (box[b][0] > box[a][1]).any(), (a, b)
    lo, hi, L = PQ.scene_size(refs)
    big = 4 * L
    for r in refs:
        r.slack = 10 * 1e-5 * L
    rays = [PQ.random_rays(lo, hi, L)]
    # designed rays: through a body's centre along its turned axes; from inside a posed body; at the place a body was committed in;
    # max_dist short of the first body
    body = 5
    A, _ = split(poses[body])
    mid_box = (box[body][0] + box[body][1]) / 2
    cen = min((refs[p].pos.mean(0) for p in range(TABLE[body], TABLE[body + 1])), key=lambda c: np.linalg.norm(c - mid_box))      # its middle piece's
    designed = [np.r_[cen - 30 * A[:, k], A[:, k], big] for k in range(3)]
    inner = int(TABLE[body]) + 7
    designed.append(np.r_[refs[inner].pos.mean(0), [0, 0, 1], big])
    old = plain[0].pos.mean(0)
    designed.append(np.r_[old + [0, 0, 60], [0, 0, -1], big])
    q0 = np.asarray(designed[0], np.float32).astype(np.float64)
    t0 = min(a["t"] for a in (r.ray(q0) for r in refs) if a is not None and a["hit"])
    designed.append(np.r_[q0[:6], t0 - 1e-3 * L])
    # ... and eight aimed at pieces of every body, so that every pose is asked about
    rng = np.random.default_rng(5)
    for c in range(len(SIZES)):
        for p in rng.integers(TABLE[c], TABLE[c + 1], 8):
            u = rng.normal(size=3)
            u /= np.linalg.norm(u)
            designed.append(np.r_[refs[p].pos.mean(0) - 50 * u, u, big])
    rays = np.concatenate(rays + [np.asarray(designed, np.float32)])
    f64 = rays.astype(np.float64)
    assert [a for a in (r.ray(f64[256 + 3]) for r in refs) if a is not None and a["hit"] and a["inside"]]
    assert any(a["hit"] for a in (r.ray(f64[256 + 4]) for r in plain)) and not any(a["hit"] for a in (r.ray(f64[256 + 4]) for r in refs))
    answers = [PQ.ref_ray(refs, q, 1e-5 * L)[:2] for q in f64]
    decided, expect = np.array([a[1] for a in answers]), [a[0] for a in answers]
    assert (~decided[:256]).sum() <= CAP * 256
    # spheres: seeded ones; one that touches two bodies; one that touches only a body's old place
    mid = (cen + (box[AT_REST][0] + box[AT_REST][1]) / 2) / 2
    spheres = np.concatenate([PQ.random_spheres(lo, hi, L), np.asarray([np.r_[mid, 0.55 * np.linalg.norm(cen - mid) + 8.0], np.r_[old, 0.5]], np.float32)])
    exp, dec = PQ.ref_mask(refs, spheres, L)
    assert (~dec).sum() <= CAP * dec.size
    touched = np.array([[exp[s, TABLE[c]:TABLE[c + 1]].any() for c in range(len(SIZES))] for s in range(len(spheres))])
    assert touched[-2].sum() >= 2 and touched[-2][[AT_REST, body]].all() and not touched[-1].any()
    assert PQ.ref_mask(plain, spheres[-1:], L)[0].any()
    _LAT.update(n=n, plain=plain, refs=refs, poses=poses, comp=comp, L=L, rays=rays, decided=decided, expect=expect, spheres=spheres,
                exp=exp, dec=dec, touched=touched, body=body)
    return _LAT


def lattice_engine(E, posed=True):
    eng, _ = PQ.scene_d(E)
    eng.scene_set_compounds(TABLE)
    if posed:
        eng.scene_set_poses(lattice(E)["poses"])
    return eng


class HostMem:
    """Device memory of the emulation is host memory."""

    def up(self, a):
        return np.ascontiguousarray(a).copy()

    def zeros(self, nbytes, fill=0):
        return np.full(nbytes, fill, np.uint8)

    def ptr(self, a):
        return a.ctypes.data

    def down(self, a):
        return a.copy()

    def sync(self):
        pass


class TorchMem:
    def __init__(self, torch):
        self.torch = torch

    def up(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda()

    def zeros(self, nbytes, fill=0):
        return self.torch.full((nbytes,), fill, dtype=self.torch.uint8, device="cuda")

    def ptr(self, a):
        return a.data_ptr()

    def down(self, a):
        self.sync()
        return a.cpu().numpy()

    def sync(self):
        self.torch.cuda.synchronize()


def overlap_dev(eng, mem, spheres, n, nc, body_mass=None, min_mass=0.0):
    """surtr_scene_overlap_dev -> (piece mask [s, n], body mask [s, nc])."""
    sp = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
    d_s, d_p, d_b = mem.up(sp), mem.zeros(sp.shape[0] * n, 0xAB), mem.zeros(sp.shape[0] * nc, 0xAB)
    d_w = None if body_mass is None else mem.up(np.ascontiguousarray(body_mass, engine.MASS_DTYPE))
    mem.sync()
    eng.scene_overlap_dev(sp.shape[0], mem.ptr(d_s), mem.ptr(d_b), sp.shape[0] * nc, dev_piece_mask=mem.ptr(d_p), piece_capacity=sp.shape[0] * n,
                          dev_body_mass=None if d_w is None else mem.ptr(d_w), min_mass=min_mass)
    return mem.down(d_p).reshape(-1, n), mem.down(d_b).reshape(-1, nc)


def body_masses(eng, set=1):
    """The reference's body masses: the host's parallel-axis sum over the pieces' records."""
    table = eng.scene_compounds()
    return engine.combine_mass(table, np.arange(int(table[-1]), dtype=np.int32), eng.pieces_mass(set=set))


# ------------------------------------------------------------------ test 1: the posed lattice
def run_posed_lattice(E, mem):
    T = lattice(E)
    n, L, rays, refs, comp = T["n"], T["L"], T["rays"], T["refs"], T["comp"]
    eng = lattice_engine(E)
    got = eng.scene_raycast(rays)
    und = PQ.check_rays(refs, rays[:256], got[:256], L, CAP)
    PQ.check_rays(refs, rays[256:], got[256:], L)
    hit = got["piece"] >= 0
    assert (got["compound"][hit] == comp[got["piece"][hit]]).all() and (got["compound"][~hit] == -1).all()
    d = got[256:]
    print("posed lattice: L", L, "undecided rays", und, "hits", int(hit.sum()), "designed", [(int(x["piece"]), int(x["compound"])) for x in d])
    assert (d["compound"][:3] == T["body"]).all() and d[3]["status"] == engine.RAY_STARTS_INSIDE and d[3]["compound"] == T["body"]
    assert (d[3]["pos"] == rays[256 + 3][:3]).all() and (d[3]["normal"] == -rays[256 + 3][3:6]).all() and d[3]["t"] == 0
    assert d[4]["piece"] == -1 and not (d[5]["piece"] == d[0]["piece"] and d[5]["t"] == d[0]["t"])
    assert {int(c) for c in got["compound"][hit]} == set(range(len(SIZES)))          # every body was found where its pose put it
    for k in (1, 63, 64, 65):
        assert eng.scene_raycast(rays[:k]).tobytes() == got[:k].tobytes(), k
    assert eng.scene_raycast(rays).tobytes() == got.tobytes()
    status = eng.pieces_query_status(n)
    assert not status.any()

    spheres, exp, dec = T["spheres"], T["exp"], T["dec"]
    nc = len(SIZES)
    pm, bm = overlap_dev(eng, mem, spheres, n, nc)
    PQ.check_mask(exp, dec, pm)
    union = np.array([[pm[s, TABLE[c]:TABLE[c + 1]].any() for c in range(nc)] for s in range(len(spheres))])
    assert (bm == union.astype(np.uint8)).all()
    assert bm[-2].sum() >= 2 and not bm[-1].any() and not pm[-1].any()
    assert (eng.scene_overlap(spheres) == bm).all()
    # the gate, between two body masses of bodies the reference says are touched
    mass = body_masses(eng)
    sure = np.array([[(exp[s, TABLE[c]:TABLE[c + 1]].astype(bool) & dec[s, TABLE[c]:TABLE[c + 1]]).any() for c in range(nc)] for s in range(len(spheres))])
    ms = np.sort(np.unique(mass["mass"][sure.any(0)]))
    assert ms.shape[0] >= 2
    min_mass = float(np.float32((ms[0] + ms[1]) / 2))
    assert ms[0] < min_mass < ms[1]
    pm2, bm2 = overlap_dev(eng, mem, spheres, n, nc, body_mass=mass, min_mass=min_mass)
    want = np.where(union, np.where(mass["mass"][None, :] <= min_mass, 2, 1), 0).astype(np.uint8)
    assert (pm2 == pm).all() and (bm2 == want).all() and (bm2 == 1).any() and (bm2 == 2).any()
    assert (eng.scene_overlap(spheres, body_mass=mass, min_mass=min_mass) == want).all()
    assert (eng.scene_overlap(spheres, body_mass=eng.scene_mass(), min_mass=min_mass) == want).all()
    eng.close()
    return got, pm, bm2


# ------------------------------------------------------------------ test 2: identity poses
def run_identity(E, mem):
    T = lattice(E)
    n, rays, spheres = T["n"], T["rays"], T["spheres"]
    # (rays and spheres made for the posed scene: the un-posed lattice sits in the middle of it)
    extra = PQ.random_rays(*PQ.scene_size(T["plain"]), n=128, seed=99)
    rays = np.concatenate([rays, extra])
    eng = lattice_engine(E, posed=False)
    want, wmask = eng.pieces_raycast(rays), eng.pieces_overlap(spheres)
    assert (want["piece"] >= 0).sum() >= 64
    for explicit in (False, True):
        if explicit:
            eng.scene_set_poses(np.tile(np.eye(4, dtype=np.float32), (len(SIZES), 1, 1)))
        got = eng.scene_raycast(rays)
        for k in ("piece", "status", "t", "pos", "normal"):
            assert (got[k] == want[k]).all(), (explicit, k)
        hit = want["piece"] >= 0
        assert (got["compound"][hit] == T["comp"][want["piece"][hit]]).all() and (got["compound"][~hit] == -1).all() and not got["reserved"].any()
        pm, bm = overlap_dev(eng, mem, spheres, n, len(SIZES))
        assert (pm == wmask).all() and wmask.any()
        assert (eng.scene_poses() == np.eye(4, dtype=np.float32)).all() and eng.scene_poses().shape == (len(SIZES), 4, 4)
    eng.close()


# ------------------------------------------------------------------ test 3: the poses baked in by the calls there were
def run_baked(E):
    T = lattice(E)
    rays, L = T["rays"], T["L"]
    eng = lattice_engine(E)
    got = eng.scene_raycast(rays)
    baked = lattice_engine(E, posed=False)
    for c in range(len(SIZES)):
        if c != AT_REST:
            baked.scene_transform_compound(c, [T["poses"][c]] * SIZES[c])
    want = baked.pieces_raycast(rays)
    dec = T["decided"]
    assert dec.sum() >= 0.95 * 256
    assert (got["piece"][dec] == want["piece"][dec]).all()
    hit = dec & (want["piece"] >= 0)
    assert hit.sum() >= 16 and (got["compound"][hit] == T["comp"][want["piece"][hit]]).all()
    assert (np.abs(got["t"][hit].astype(np.float64) - want["t"][hit]) <= 1e-4 * L).all()
    eng.close(); baked.close()


# ------------------------------------------------------------------ test 4: body mass
def check_body_mass(eng, clean=True):
    table = eng.scene_compounds()
    out = []
    for s in (0, 1):
        want = engine.combine_mass(table, np.arange(int(table[-1]), dtype=np.int32), eng.pieces_mass(set=s))
        got = eng.scene_mass(set=s)
        assert got.shape == want.shape == (len(table) - 1,) and got.tobytes() == want.tobytes(), s
        assert (got["volume"] > 0).all() and not (clean and got["status"].any())
        out.append(got)
    return out


def run_body_mass(E):
    T = lattice(E)
    eng = lattice_engine(E, posed=False)
    a = check_body_mass(eng)
    eng.scene_set_poses(T["poses"])
    b = check_body_mass(eng)                     # body-frame records: a pose changes nothing
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))
    assert eng.scene_mass(density=0.0).tobytes() == engine.combine_mass(TABLE, np.arange(T["n"], dtype=np.int32), eng.pieces_mass(density=0.0)).tobytes()
    eng.close()
    eng, world = TS.three_bodies(E)
    TS.click_one(E, eng, world)
    table = eng.scene_compounds()
    assert len(table) - 1 >= 4 and int(table[-1]) > len(table) - 1        # bind 0 and the compounds beside it, behind the two bodies left
    check_body_mass(eng, clean=False)
    eng.close()


# ------------------------------------------------------------------ test 5: apply_pose
MOVE = pose_about(rotation((0.2, 1.0, 0.4), 0.6), TS.SHIFT_B, (0.5, 40.0, -1.25))


def run_apply_pose(E):
    eng, _ = TS.three_bodies(E)
    other, _ = TS.three_bodies(E)
    before = TS.snapshot(eng)
    eye = np.eye(4, dtype=np.float32)
    eng.scene_set_poses([eye, MOVE, eye])
    TS.assert_unchanged(eng, before)             # a pose rewrites no vertex
    eng.scene_apply_pose(1)
    other.scene_transform_compound(1, [MOVE])
    _, got = TS.snapshot(eng)
    _, want = TS.snapshot(other)
    for p in range(3):
        for s in (0, 1):
            assert TS.same_solid(got[p][s], want[p][s]), (p, s)
            assert TS.same_solid(got[p][s], before[1][p][s]) == (p != 1)
    assert (eng.scene_poses() == eye).all()
    rays = np.asarray([[10.5, 40.0, 40, 0, 0, -1, 100], [0, 0, 40, 0, 0, -1, 100]], np.float32)
    assert eng.pieces_raycast(rays).tobytes() == other.pieces_raycast(rays).tobytes()       # the derived data was rebuilt
    # the identity: nothing changes, and a pending scene event can still be committed
    cube = TS.bodies(E)["cube"]
    eng.upload_pieces(TS.bodies(E)["meshes"], TS.bodies(E)["convexes"])
    eng.scene_set_compounds([0, 1, 2, 3])
    eng.scene_set_poses([eye, eye, MOVE])
    eng.upload_pattern(cube["face_off"], cube["v012"])
    eng.place_cells(cube["scale"], (cube["translate"] + TS.SHIFT_B).astype(np.float32))
    eng.scene_fracture_event(1, 0, 8, flags=0)
    co, cp = eng.event_regroup()
    snap = TS.snapshot(eng)
    eng.scene_apply_pose(1); eng.scene_apply_pose(0)
    TS.assert_unchanged(eng, snap)
    n, first, n_new, _ = eng.scene_commit(co, cp)
    assert (n, first) == (10, 2) and n_new >= 1
    want = np.tile(eye, (2 + n_new, 1, 1)); want[1] = MOVE
    assert eng.scene_poses().tobytes() == want.tobytes()
    # any other pose forgets the event, as the transform does
    eng.place_cells(cube["scale"], cube["translate"])
    eng.scene_fracture_event(0, 0, 8, flags=0)
    co, cp = eng.event_regroup()
    eng.scene_apply_pose(1)
    with pytest.raises(engine.SurtrError) as e:
        eng.scene_commit(co, cp)
    assert e.value.code == engine.E_STATE
    eng.close(); other.close()


# ------------------------------------------------------------------ test 6: the click loop with motion
def baked_pieces(E, pieces, W):
    """The model's pieces after Poly::Transform by W, through surtr_transform_pieces on an engine of their own."""
    ref = E.Engine(0)
    ref.upload_pieces([p["mesh"] for p in pieces], [p["conv"] for p in pieces])
    ref.transform_pieces([W] * len(pieces))
    out = [{"mesh": ref.download_piece(k, 0), "conv": ref.download_piece(k, 1)} for k in range(len(pieces))]
    ref.close()
    return out


def posed_click(E, eng, world, poses, origin, direction, pattern, radius, min_total=0):
    """Pick on the posed scene, bake the body hit, break it (partial) and commit, against both references of test_scene.py and
    the Python model of the poses.  -> (what scene_commit returned, the compound hit)."""
    d = np.asarray(direction, np.float64)
    hit = eng.scene_raycast([list(origin) + list(d) + [1000.0]])[0]
    target = int(hit["compound"])
    assert hit["piece"] >= 0 and target == TS.compound_of(eng.scene_compounds(), int(hit["piece"]))
    eng.scene_apply_pose(target)
    world[target] = baked_pieces(E, world[target], poses[target])           # reference (a) is given the baked pieces
    pos = np.concatenate([p["mesh"]["pos"] for p in world[target]])
    lo, hi = pos.min(0), pos.max(0)
    place = ((hi - lo).astype(np.float32), ((hi.astype(np.float64) + lo.astype(np.float64)) / 2).astype(np.float32))
    impact = (hit["pos"] + np.asarray(d, np.float32) * np.float32(0.01)).astype(np.float32)
    kw = dict(partial=True, sphere_points=TS.sphere_cloud(impact, radius), origin=impact, radius=radius)
    out = TS.click(E, eng, world, target, pattern, place, None, kw)
    n, first, n_new, _, _ = out
    eye = np.eye(4, dtype=np.float32)
    del poses[target]
    poses.extend([eye] * n_new)
    assert eng.scene_poses().tobytes() == np.asarray(poses, np.float32).tobytes()       # erase, push_back; the others moved down
    assert n >= min_total
    return out, target


def run_click_loop(E):
    eng, world = TS.three_bodies(E)
    eye = np.eye(4, dtype=np.float32)
    blob_pose = pose_about(rotation((0, 0, 1), 0.3), TS.SHIFT_BLOB, (0, 40, 0))
    poses = [eye, MOVE, blob_pose]
    eng.scene_set_poses(poses)
    A, b = split(MOVE)
    was = np.asarray(TS.bodies(E)["convexes"][1]["pos"], np.float64).mean(0)
    centre = A @ was + b
    # where the body was committed nothing is hit any more; where it is now, it alone
    old = eng.scene_raycast([list(was + [0, 0, 40]) + [0, 0, -1, 1000.0]])[0]
    assert old["piece"] == -1 and eng.pieces_raycast([list(was + [0, 0, 40]) + [0, 0, -1, 1000.0]])[0]["piece"] == 1
    (n, first, n_new, _, _), target = posed_click(E, eng, world, poses, centre + [0, 0, 40], (0, 0, -1), TS.bodies(E)["cube"], 3.0)
    assert target == 1 and first == 2 and n_new >= 2 and eng.scene_poses()[1].tobytes() == blob_pose.tobytes()
    # one of the compounds the click made moves, and is clicked where it now is, with the 64-cell pattern
    made = [c for c in range(first, len(world)) if len(world[c]) >= 2] or list(range(first, len(world)))
    c = made[0]
    cen = np.concatenate([p["conv"]["pos"] for p in world[c]]).astype(np.float64).mean(0)
    poses[c] = pose_about(rotation((1, 0, 0), -0.8), cen, (0, -30, 5))
    eng.scene_set_poses(poses)
    A, b = split(poses[c])
    aim = A @ np.asarray(world[c][0]["conv"]["pos"], np.float64).mean(0) + b
    (n2, _, _, _, _), target = posed_click(E, eng, world, poses, aim + [0, 0, 30], (0, 0, -1), TS.bodies(E)["blob"], 1.5, min_total=65)
    assert target == c
    check_body_mass_status_free(eng)
    eng.close()
    return n, n2


def check_body_mass_status_free(eng):
    """scene_mass against the host's sum on whatever the clicks left (fragments may be flagged: no claim on status)."""
    table = eng.scene_compounds()
    for s in (0, 1):
        assert eng.scene_mass(set=s).tobytes() == engine.combine_mass(table, np.arange(int(table[-1]), dtype=np.int32), eng.pieces_mass(set=s)).tobytes()


# ------------------------------------------------------------------ test 7: errors
def run_errors(E):
    L_ = E.lib()
    fresh = E.Engine(0)
    eye = np.eye(4, dtype=np.float32)
    for call in (lambda: fresh.scene_set_poses([eye]), lambda: fresh.scene_poses(), lambda: fresh.scene_apply_pose(0), lambda: fresh.scene_mass(),
                 lambda: fresh.scene_raycast([[0, 0, 9, 0, 0, -1, 100]]), lambda: fresh.scene_overlap([[0, 0, 0, 1]])):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == engine.E_STATE
    fresh.close()
    eng, _ = TS.three_bodies(E)
    good = np.asarray([eye, MOVE, eye], np.float32)
    eng.scene_set_poses(good)
    before = TS.snapshot(eng)

    def refused(code, call):
        with pytest.raises(engine.SurtrError) as e:
            call()
        assert e.value.code == code, e.value
        TS.assert_unchanged(eng, before)
        assert eng.scene_poses().tobytes() == good.tobytes()

    def with_second(W):
        return np.asarray([eye, W, eye], np.float32)
    scaled = MOVE.copy(); scaled[:3, :3] *= np.float32(1.01)
    mirror = MOVE.copy(); mirror[:3, 0] = -mirror[:3, 0]
    nan = MOVE.copy(); nan[1, 3] = np.nan
    inf = MOVE.copy(); inf[0, 0] = np.inf
    row = MOVE.copy(); row[3, 0] = 1e-6
    row2 = MOVE.copy(); row2[3, 3] = np.float32(1.0000001)
    for bad in (scaled, mirror, nan, inf, row, row2):
        refused(engine.E_INVALID, lambda: eng.scene_set_poses(with_second(bad)))
    refused(engine.E_INVALID, lambda: eng.scene_set_poses(good[:2]))
    refused(engine.E_INVALID, lambda: eng.scene_set_poses(np.concatenate([good, good[:1]])))
    refused(engine.E_INVALID, lambda: eng.scene_apply_pose(3))
    for bad in ([0, 0, 0, 0, 0, 0, 1], [0, 0, 0, np.nan, 0, 1, 1], [0, 0, 0, 1, 0, 0, -1], [np.inf, 0, 0, 1, 0, 0, 1]):
        refused(engine.E_INVALID, lambda: eng.scene_raycast(np.asarray([[0, 0, 40, 0, 0, -1, 100], bad], np.float32)))
    refused(engine.E_INVALID, lambda: eng.scene_overlap([[0, 0, 0, -1]]))
    refused(engine.E_INVALID, lambda: eng.scene_overlap([[0, np.nan, 0, 1]]))
    # capacities (the emulation's device memory is host memory; on the GPU these calls return before they touch the pointers)
    n = ctypes.c_uint32(2)
    w = np.full((2, 16), 7, np.float32)
    assert L_.surtr_scene_get_poses(eng._h, ctypes.c_uint32(2), ctypes.byref(n), ctypes.c_void_p(w.ctypes.data)) == engine.E_CAPACITY and n.value == 3 and (w == 7).all()
    n = ctypes.c_uint32(2)
    rec = np.zeros(2, engine.MASS_DTYPE)
    assert L_.surtr_scene_mass(eng._h, ctypes.c_int(1), ctypes.c_float(10), ctypes.byref(n), ctypes.c_void_p(rec.ctypes.data)) == engine.E_CAPACITY and n.value == 3
    n = ctypes.c_uint32(2)
    sp = np.asarray([[0, 0, 0, 1]], np.float32)
    bm = np.full(2, 0xAB, np.uint8)
    assert L_.surtr_scene_overlap(eng._h, ctypes.c_uint32(1), ctypes.c_void_p(sp.ctypes.data), None, ctypes.c_float(0), ctypes.byref(n),
                                  ctypes.c_void_p(bm.ctypes.data)) == engine.E_CAPACITY and n.value == 3 and (bm == 0xAB).all()
    one = ctypes.c_void_p(1)          # never read: the capacity is checked first
    assert L_.surtr_scene_raycast_dev(eng._h, ctypes.c_uint32(3), one, one, ctypes.c_size_t(2 * 48)) == engine.E_CAPACITY
    assert L_.surtr_scene_mass_dev(eng._h, ctypes.c_int(1), ctypes.c_float(10), one, ctypes.c_size_t(2 * 96)) == engine.E_CAPACITY
    assert L_.surtr_scene_overlap_dev(eng._h, ctypes.c_uint32(2), one, None, ctypes.c_float(0), None, ctypes.c_size_t(0), one, ctypes.c_size_t(5)) == engine.E_CAPACITY
    assert L_.surtr_scene_overlap_dev(eng._h, ctypes.c_uint32(2), one, None, ctypes.c_float(0), one, ctypes.c_size_t(5), one, ctypes.c_size_t(6)) == engine.E_CAPACITY
    TS.assert_unchanged(eng, before)
    assert eng.scene_poses().tobytes() == good.tobytes()
    # a commit that is refused leaves the poses alone
    cube = TS.bodies(E)["cube"]
    eng.upload_pattern(cube["face_off"], cube["v012"])
    eng.place_cells(cube["scale"], cube["translate"])
    eng.scene_fracture_event(0, 0, 8, flags=0)
    co, cp = eng.event_regroup()
    dup = cp.copy(); dup[1] = dup[0]
    refused(engine.E_INVALID, lambda: eng.scene_commit(co, dup))
    # who resets the poses
    eng.scene_set_compounds([0, 1, 2, 3])
    assert (eng.scene_poses() == eye).all()
    eng.scene_set_poses(good)
    eng.transform_pieces([eye, eye, eye])
    eng.scene_transform_compound(0, [eye])
    assert eng.scene_poses().tobytes() == good.tobytes()          # explicit bakes leave them alone
    eng.upload_pieces(TS.bodies(E)["meshes"], TS.bodies(E)["convexes"])
    assert eng.scene_poses().shape == (1, 4, 4) and (eng.scene_poses() == eye).all()
    eng.close()


def run_invalid_ray_dev(E, mem):
    """An invalid ray in the _dev form is a status bit, with no body."""
    eng, _ = TS.three_bodies(E)
    eng.scene_set_poses([np.eye(4, dtype=np.float32), MOVE, np.eye(4, dtype=np.float32)])
    A, b = split(MOVE)
    centre = A @ np.asarray(TS.bodies(E)["convexes"][1]["pos"], np.float64).mean(0) + b
    rays = np.asarray([list(centre + [0, 0, 40]) + [0, 0, -1, 100], [0, 0, 0, 0, 0, 0, 1], list(centre + [0, 0, 40]) + [0, 0, -1, 100]], np.float32)
    d_r, d_h = mem.up(rays), mem.zeros(3 * 48, 0xAB)
    mem.sync()
    eng.scene_raycast_dev(3, mem.ptr(d_r), mem.ptr(d_h), 3 * 48)
    hits = mem.down(d_h).view(engine.SCENE_RAY_HIT_DTYPE)
    assert list(hits["piece"]) == [1, -1, 1] and list(hits["compound"]) == [1, -1, 1] and list(hits["status"]) == [0, engine.RAY_INVALID, 0]
    assert hits[0].tobytes() == hits[2].tobytes() and not hits["reserved"].any()
    eng.close()


# ------------------------------------------------------------------ CPU tier (emulation)
def test_posed_lattice_against_reference(emul_engine):
    run_posed_lattice(emul_engine, HostMem())


def test_identity_poses_equal_the_unposed_queries(emul_engine):
    run_identity(emul_engine, HostMem())


def test_posed_queries_equal_baked_pieces(emul_engine):
    run_baked(emul_engine)


def test_body_mass_is_the_hosts_sum_bit_for_bit(emul_engine):
    run_body_mass(emul_engine)


def test_apply_pose_is_the_transform(emul_engine):
    run_apply_pose(emul_engine)


def test_click_loop_with_motion(emul_engine):
    n, n2 = run_click_loop(emul_engine)
    print("resident pieces after click 1:", n, "after click 2:", n2)


def test_errors_leave_table_poses_and_pieces_unchanged(emul_engine):
    run_errors(emul_engine)
    run_invalid_ray_dev(emul_engine, HostMem())


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_scene_poses as T
    case = sys.argv[1]
    mem = T.TorchMem(torch)
    if case in ("posed_lattice", "identity", "invalid_ray_dev"):
        getattr(T, "run_" + case)(engine, mem)
    elif case == "dev_forms":
        T.run_dev_forms(engine, torch)
    elif case == "harness":
        T.check_harness(engine, %(root)r)
    else:
        getattr(T, "run_" + case)(engine)
    print("ok", case)
""")


def run_dev_forms(E, torch):
    """The _dev forms on a stream of their own with the in-flight hint at 6 give the host forms' bytes, and so does a second context."""
    T = lattice(E)
    n, nc, rays, spheres = T["n"], len(SIZES), T["rays"], T["spheres"]
    eng = lattice_engine(E)
    hits = eng.scene_raycast(rays)
    mass = eng.scene_mass()
    min_mass = float(np.median(mass["mass"]))
    body = eng.scene_overlap(spheres, body_mass=mass, min_mass=min_mass)
    assert (body == 1).any() and (body == 2).any()
    results = []
    for k in range(2):
        ctx = lattice_engine(E)
        st = torch.cuda.Stream()
        ctx.set_stream(st.cuda_stream)
        ctx.set_events_in_flight(6)
        with torch.cuda.stream(st):
            d_r, d_s = torch.from_numpy(rays).cuda(), torch.from_numpy(spheres).cuda()
            d_h = torch.zeros(rays.shape[0] * 48, dtype=torch.uint8, device="cuda")
            d_w = torch.zeros(nc * 96, dtype=torch.uint8, device="cuda")
            d_p = torch.zeros(spheres.shape[0] * n, dtype=torch.uint8, device="cuda")
            d_b = torch.zeros(spheres.shape[0] * nc, dtype=torch.uint8, device="cuda")
            st.synchronize()
            ctx.scene_mass_dev(d_w.data_ptr(), d_w.numel())
            ctx.scene_raycast_dev(rays.shape[0], d_r.data_ptr(), d_h.data_ptr(), d_h.numel())
            ctx.scene_overlap_dev(spheres.shape[0], d_s.data_ptr(), d_b.data_ptr(), d_b.numel(), dev_piece_mask=d_p.data_ptr(), piece_capacity=d_p.numel(),
                                  dev_body_mass=d_w.data_ptr(), min_mass=min_mass)
            st.synchronize()
        results.append((d_h.cpu().numpy().tobytes(), d_w.cpu().numpy().tobytes(), d_p.cpu().numpy().tobytes(), d_b.cpu().numpy().tobytes()))
        ctx.close()
    assert results[0] == results[1]
    assert results[0][0] == hits.tobytes() and results[0][1] == mass.tobytes() and results[0][3] == body.tobytes()
    eng.close()


HARNESS_POSE = pose_about(rotation((0, 0, 1), 0.5), (0, 0, 0), (0, 6, 0))
HARNESS_FAR = PQ.world(np.eye(3), (0, 0, 20))       # a body that is not clicked: its pose is kept, and moves down with it


def python_body_click(eng, o, d, r, n_cells, radial):
    """OnMouseDownBodies through the Python calls, in float as the host layer computes it."""
    hit = eng.scene_raycast([list(o) + list(d) + [1000.0]])[0]
    assert hit["piece"] >= 0
    r32 = np.float32(r)
    impact = (hit["pos"] + np.asarray(d, np.float32) * np.float32(0.01)).astype(np.float32)
    mass = eng.scene_mass(set=1)
    body = eng.scene_overlap([list(impact) + [float(r32 / np.float32(2))]], body_mass=mass, min_mass=1e-4)[0]
    picked = [int(c) for c in np.nonzero(body == 1)[0]] if radial else [int(hit["compound"])]
    cloud = (TS.lattice_cloud() * r32 + impact).astype(np.float32)
    made = []
    for comp in sorted(picked, reverse=True):
        made = [c - 1 for c in made]
        eng.scene_apply_pose(comp)
        table = eng.scene_compounds()
        mask = [engine.convex_out_of_sphere(eng.download_piece(p, 1), cloud, impact, float(r32)) for p in range(int(table[comp]), int(table[comp + 1]))]
        eng.place_cells([r32 * np.float32(2)] * 3, impact)
        eng.scene_fracture_event(comp, 0, n_cells, outside=np.asarray(mask, np.uint8) if any(mask) else None, flags=0)
        co, cp = eng.event_regroup(partial=True, sphere_points=cloud, origin=impact, radius=float(r32))
        eng.event_refit()
        n, first, n_new, _ = eng.scene_commit(co, cp)
        made += list(range(first, first + n_new))
    table = eng.scene_compounds()
    return dict(hit_piece=int(hit["piece"]), hit_compound=int(hit["compound"]), body_mask=[int(x) for x in body], compounds_hit=sorted(picked),
                compounds_made=made, table=[int(x) for x in table], mass=[float(x) for x in eng.scene_mass(set=1)["mass"]])


def check_harness(E, root, exe=None):
    """surtr_harness --scene-poses ... --body-clicks ... (FractureEngine::OnMouseDownBodies, and ExecuteFractureRoutine taking the
    stored pose) against the same clicks through the Python calls, RadialMode off and on."""
    exe = exe or os.path.join(root, "surtr_amd", "host", "surtr_harness")
    clicks = [([-10.0, 6.3, 0.2], [1.0, 0.0, 0.0]), ([0.3, 0.2, 10.0], [0.0, 0.0, -1.0])]
    arg = ";".join(",".join("%r" % x for x in o + d) for o, d in clicks)
    pose_arg = ";".join("%d:" % c + ",".join("%r" % float(x) for x in W.reshape(-1)) for c, W in ((1, HARNESS_POSE), (3, HARNESS_FAR)))
    for radial in (False, True):
        cmd = [exe, "--mesh", "cube", "--cells", "8", "--scene-poses", pose_arg, "--body-clicks", arg, "--impact-radius", "4.0"] + (["--radial"] if radial else [])
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-2000:])
        lines = [json.loads(x) for x in p.stdout.strip().splitlines() if x.startswith('{"body_click"')]
        assert len(lines) == len(clicks)
        sc = scenes.cube_scene(8)
        eng = E.Engine(0)
        eng.upload_pieces([sc["mesh"]], [sc["convex"]])
        eng.upload_pattern(sc["face_off"], sc["v012"])
        eng.place_cells(sc["scale"], sc["translate"])
        eng.fracture_event(0, 8)
        n = eng.pieces_from_event()
        eng.scene_set_compounds(list(range(0, n, 2)) + [n])
        poses = np.tile(np.eye(4, dtype=np.float32), ((n + 1) // 2, 1, 1))
        poses[1], poses[3] = HARNESS_POSE, HARNESS_FAR
        eng.scene_set_poses(poses)
        for k, (o, d) in enumerate(clicks):
            want = dict(python_body_click(eng, o, d, 4.0, 8, radial), body_click=k)
            got_poses = np.asarray(lines[k].pop("poses"), np.float32).reshape(-1, 4, 4)
            assert lines[k] == want, (radial, lines[k], want)
            assert got_poses.tobytes() == eng.scene_poses().tobytes()
            assert len(want["compounds_made"]) >= 1 and (not radial or want["body_mask"].count(1) == len(want["compounds_hit"]))
            if k == 0:      # the first click finds the posed body where its pose put it; the far body's pose moved down with it
                assert want["hit_compound"] == 1 and got_poses[2].tobytes() == HARNESS_FAR.tobytes() and (got_poses[[0, 1]] == np.eye(4)).all()
        assert len(want["compounds_hit"]) == (2 if radial else 1)
        eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["posed_lattice", "identity", "baked", "body_mass", "apply_pose", "click_loop", "errors", "invalid_ray_dev", "dev_forms"])
def test_gpu_scene_poses(case):
    run_gpu_child(GPU_CHILD, case, 120)


@pytest.mark.gpu
def test_gpu_harness_body_clicks():
    run_gpu_child(GPU_CHILD, "harness", 150)
