"""Picking on a scene whose bodies have moved: BASELINE configs[3] (bumpy torus x 4096 cells -> pieces_from_event), every resident
piece a body of its own with a random rigid pose about its centre of mass.

Measured: the device time of one posed ray, of 4 096 posed rays, of one gated body sphere and of surtr_scene_mass_dev, and the wall
time of one posed pick (scene_raycast of one ray, scene_mass, scene_overlap with the gate: what PickBodies does).  Beside each:
 * the un-posed query of this build (pieces_raycast / pieces_overlap / pieces_mass) in this process;
 * the route there was for a body that has moved -- bake the pose (scene_transform_compound for one moved body; transform_pieces for
   all of them in one call), then pieces_raycast, pieces_mass read back, combine_mass on the host, pieces_overlap;
 * with --parent-lib PATH (a libsurtr_hip.so built from the parent commit): the un-posed pieces_raycast / pieces_overlap of that
   build and of this one, each in --runs fresh processes, so that the spread between repeated runs of the parent is known.  The
   shared qr_* helpers of query_dev.hip were made templates for the posed kernels: this is what says whether that cost anything.
Device times are HIP events on the context's stream around the _dev calls after a warm-up (median of --reps).
Prints one JSON line; --out FILE writes it there too (profiles/scene_poses_bench.json)."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from surtr_amd import engine as E, scenes as S

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=4096)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--parent-lib", default=None)
ap.add_argument("--lib", default=None, help="bind this library instead of the tree's (the child processes of --parent-lib)")
ap.add_argument("--unposed-only", action="store_true")
args = ap.parse_args()
if args.lib:
    E._use_library_for_tests(args.lib)

st = torch.cuda.Stream()
eng = E.Engine(0, stream=st.cuda_stream)
sc = S.torus_scene(args.cells, eng=eng)
eng.upload_pieces([sc["mesh"]], [sc["convex"]])
eng.upload_pattern(sc["face_off"], sc["v012"])
eng.place_cells(sc["scale"], sc["translate"])
eng.fracture_event(0, sc["n_cells"])
n = eng.pieces_from_event()
mass = eng.pieces_mass(set=1)
lo, hi = mass["com"].min(0), mass["com"].max(0)
L = float(np.linalg.norm(hi - lo))
rng = np.random.default_rng(20261018)
c = (lo + hi) / 2
u = rng.normal(size=(4096, 3))
o = c + u / np.linalg.norm(u, axis=1)[:, None] * L
d = mass["com"][rng.integers(0, n, 4096)] - o
d /= np.linalg.norm(d, axis=1)[:, None]
rays = np.c_[o, d, np.full(4096, 4 * L)].astype(np.float32)


def wall(f):
    f()
    ts = []
    for _ in range(args.reps):
        a = time.perf_counter(); f(); ts.append((time.perf_counter() - a) * 1e3)
    return float(np.median(ts))


def device(f):
    with torch.cuda.stream(st):
        for _ in range(3):
            f()
        st.synchronize()
        ts = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st); f(); b.record(st); b.synchronize()
            ts.append(a.elapsed_time(b))
    return float(np.median(ts))


hit = eng.pieces_raycast(rays[:1])[0]
assert hit["piece"] >= 0
sphere = np.r_[hit["pos"], 0.05 * L].astype(np.float32).reshape(1, 4)
with torch.cuda.stream(st):
    d_r = torch.from_numpy(rays).cuda(); d_s = torch.from_numpy(sphere).cuda()
    d_h = torch.zeros(rays.shape[0] * 48, dtype=torch.uint8, device="cuda")
    d_m = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_b = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_w = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    d_bw = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    st.synchronize()
eng.pieces_mass_dev(d_w.data_ptr(), d_w.numel(), set=1)
res = {
    "scene": "configs[3]: bumpy torus x %d cells, %d resident pieces, one compound each" % (args.cells, n), "pieces": n, "reps": args.reps,
    "unposed_one_ray_device_ms": device(lambda: eng.pieces_raycast_dev(1, d_r.data_ptr(), d_h.data_ptr(), d_h.numel())),
    "unposed_rays_4096_device_ms": device(lambda: eng.pieces_raycast_dev(4096, d_r.data_ptr(), d_h.data_ptr(), d_h.numel())),
    "unposed_one_sphere_gate_device_ms": device(lambda: eng.pieces_overlap_dev(1, d_s.data_ptr(), d_m.data_ptr(), d_m.numel(), dev_mass=d_w.data_ptr())),
    "pieces_mass_dev_device_ms": device(lambda: eng.pieces_mass_dev(d_w.data_ptr(), d_w.numel(), set=1)),
}
if args.unposed_only:
    print(json.dumps(res))
    eng.close()
    sys.exit(0)


def rotation(axis, angle):
    axis = axis / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def pose(rot, centre, shift):
    m = np.eye(4, dtype=np.float32)
    m[:3, :3] = rot.astype(np.float32)
    m[:3, 3] = (centre - rot @ centre + shift).astype(np.float32)
    return m


# every piece a body, turned about its centre of mass by up to half a radian and moved by up to 1 % of the scene
eng.scene_set_compounds(np.arange(n + 1, dtype=np.uint32))
rots = [rotation(rng.normal(size=3), rng.uniform(-0.5, 0.5)) for _ in range(n)]
shifts = rng.normal(size=(n, 3)) * 0.01 * L
poses = np.asarray([pose(rots[k], mass["com"][k], shifts[k]) for k in range(n)], np.float32)
# ... and back again, for the route that bakes: the pieces are where they were after every second call
back = np.asarray([pose(rots[k].T, mass["com"][k] + shifts[k], -shifts[k]) for k in range(n)], np.float32)
eng.scene_set_poses(poses)
phit = eng.scene_raycast(rays[:1])[0]
assert phit["piece"] >= 0 and phit["compound"] == phit["piece"]
psphere = np.r_[phit["pos"], 0.05 * L].astype(np.float32).reshape(1, 4)
d_s.copy_(torch.from_numpy(psphere).cuda())
eng.scene_mass_dev(d_bw.data_ptr(), d_bw.numel(), set=1)
table = np.arange(n + 1, dtype=np.uint32)
members = np.arange(n, dtype=np.int32)
moved = int(phit["compound"])
flip = [0]


def posed_pick():
    h = eng.scene_raycast(rays[:1])[0]
    bm = eng.scene_mass(set=1)
    return eng.scene_overlap(np.r_[h["pos"], 0.05 * L].astype(np.float32).reshape(1, 4), body_mass=bm, min_mass=1e-4)


def old_pick(bake):
    bake()
    h = eng.pieces_raycast(rays[:1])[0]
    pm = eng.pieces_mass(set=1)
    E.combine_mass(table, members, pm)
    return eng.pieces_overlap(np.r_[h["pos"], 0.05 * L].astype(np.float32).reshape(1, 4), mass=pm, min_mass=1e-4)


def bake_one():
    flip[0] ^= 1
    eng.scene_transform_compound(moved, [poses[moved] if flip[0] else back[moved]])


def bake_all():
    flip[0] ^= 1
    eng.transform_pieces(poses if flip[0] else back)


res.update({
    "posed_one_ray_device_ms": device(lambda: eng.scene_raycast_dev(1, d_r.data_ptr(), d_h.data_ptr(), d_h.numel())),
    "posed_rays_4096_device_ms": device(lambda: eng.scene_raycast_dev(4096, d_r.data_ptr(), d_h.data_ptr(), d_h.numel())),
    "posed_one_body_sphere_gate_device_ms": device(lambda: eng.scene_overlap_dev(1, d_s.data_ptr(), d_b.data_ptr(), d_b.numel(), dev_body_mass=d_bw.data_ptr())),
    "scene_mass_dev_device_ms": device(lambda: eng.scene_mass_dev(d_bw.data_ptr(), d_bw.numel(), set=1)),
    "posed_pick_wall_ms": wall(posed_pick),
})
eng.scene_set_poses(np.tile(np.eye(4, dtype=np.float32), (n, 1, 1)))
res.update({
    "bake_one_body_then_pick_wall_ms": wall(lambda: old_pick(bake_one)),
    "bake_all_bodies_then_pick_wall_ms": wall(lambda: old_pick(bake_all)),
    "bake_one_body_wall_ms": wall(bake_one),
    "bake_all_bodies_wall_ms": wall(bake_all),
})
eng.close()

if args.parent_lib:
    keys = ("unposed_one_ray_device_ms", "unposed_rays_4096_device_ms", "unposed_one_sphere_gate_device_ms", "pieces_mass_dev_device_ms")
    for name, lib in (("parent", args.parent_lib), ("this", E.lib_path())):
        runs = []
        for _ in range(args.runs):
            p = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--lib", lib, "--unposed-only", "--cells", str(args.cells),
                                "--reps", str(args.reps)], capture_output=True, text=True)
            if p.returncode != 0:
                sys.exit("child with %s failed (%d): %s" % (lib, p.returncode, p.stderr[-2000:]))
            runs.append(json.loads(p.stdout.strip().splitlines()[-1]))
        for k in keys:
            res["%s_build_%s_runs" % (name, k)] = [r[k] for r in runs]
    for k in keys[:2]:
        a, b = res["parent_build_%s_runs" % k], res["this_build_%s_runs" % k]
        res["%s_parent_spread" % k] = max(a) - min(a)
        res["%s_this_minus_parent_median" % k] = float(np.median(b) - np.median(a))
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
