"""Scene upkeep on the broken configs[3] scene of scripts/bench_scene.py (bumpy torus x 4096 cells, every regrouped compound a body,
every body under a pose of its own): the world bounds of every body, one cull of the light bodies, one append of a body -- each
beside the only route there was before: download_piece of every piece (plus numpy for the bounds; plus upload_pieces,
scene_set_compounds and scene_set_poses for an edit), timed in the same run.

scene_bounds_dev is bracketed by HIP events on the context's stream (device time, poses unchanged between calls) and timed once
more with a scene_set_poses before every call, as a frame does it (host clock around call + synchronisation: the pose upload is in
it).  The edits end in a stream synchronisation, so the host clock around them is a call time.  Medians.  Prints one JSON line;
--out FILE writes it there too.  --emul LIB rehearses the script on the CPU emulation at a small size: no HIP events, and the line
says that it is no measurement."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from surtr_amd import engine as E, scenes as S

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=4096)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--edit-reps", type=int, default=5)
ap.add_argument("--base-reps", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--emul", default=None)
args = ap.parse_args()

if args.emul:
    E._use_library_for_tests(args.emul)
    torch, st = None, None
    eng = E.Engine(0)
else:
    import torch
    assert torch.cuda.is_available(), "no GPU: nothing can be measured here"
    st = torch.cuda.Stream()
    eng = E.Engine(0, stream=st.cuda_stream)

sc = S.torus_scene(args.cells, eng=eng)
eng.upload_pieces([sc["mesh"]], [sc["convex"]])
eng.upload_pattern(sc["face_off"], sc["v012"])
eng.place_cells(sc["scale"], sc["translate"])
eng.scene_fracture_event(0, 0, sc["n_cells"], flags=0)
co, cp = eng.event_regroup()
eng.event_refit()
n0, _, nc0, _ = eng.scene_commit(co, cp)


def random_poses(nc, seed):
    rng = np.random.default_rng(seed)
    out = np.tile(np.eye(4, dtype=np.float32), (nc, 1, 1))
    for c in range(nc):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        w, x, y, z = q
        out[c, :3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
        out[c, :3, 3] = rng.normal(size=3) * 0.05
    return out


def sync():
    if st is not None:
        st.synchronize()


def dev_buffers(n, nc):
    if torch is None:
        b, p = np.zeros(nc * 32, np.uint8), np.zeros(n * 32, np.uint8)
        return b, p, b.ctypes.data, p.ctypes.data
    b, p = torch.zeros(nc * 32, dtype=torch.uint8, device="cuda"), torch.zeros(n * 32, dtype=torch.uint8, device="cuda")
    return b, p, b.data_ptr(), p.data_ptr()


def bounds_times(set):
    table = eng.scene_compounds()
    n, nc = int(table[-1]), len(table) - 1
    keep = dev_buffers(n, nc)
    dev, frame = [], []
    eng.scene_bounds_dev(keep[2], nc * 32, dev_piece=keep[3], piece_capacity=n * 32, set=set)      # (the first call brings the poses over)
    sync()
    for k in range(args.reps):
        if st is not None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
        eng.scene_bounds_dev(keep[2], nc * 32, dev_piece=keep[3], piece_capacity=n * 32, set=set)
        if st is not None:
            b.record(st); b.synchronize()
            dev.append(a.elapsed_time(b))
    for k in range(args.reps):
        poses = random_poses(nc, 100 + k) if k < 4 else poses
        c0 = time.perf_counter()
        eng.scene_set_poses(poses)
        eng.scene_bounds_dev(keep[2], nc * 32, dev_piece=keep[3], piece_capacity=n * 32, set=set)
        sync()
        frame.append((time.perf_counter() - c0) * 1e3)
    return (float(np.median(dev)) if dev else None), float(np.median(frame))


def download_world():
    table = eng.scene_compounds()
    return table, [(eng.download_piece(p, 0), eng.download_piece(p, 1)) for p in range(int(table[-1]))]


def parent_bounds(set):
    """download_piece of every piece of the set, the pose applied in numpy float32, min / max per body."""
    c0 = time.perf_counter()
    table, poses = eng.scene_compounds(), eng.scene_poses()
    lo, hi = np.zeros((len(table) - 1, 3), np.float32), np.zeros((len(table) - 1, 3), np.float32)
    for c in range(len(table) - 1):
        x = np.concatenate([eng.download_piece(p, set)["pos"].reshape(-1, 3) for p in range(int(table[c]), int(table[c + 1]))])
        x = x @ poses[c][:3, :3].T + poses[c][:3, 3]
        lo[c], hi[c] = x.min(0), x.max(0)
    return (time.perf_counter() - c0) * 1e3


def parent_edit(keep_body, extra=None):
    """The edit by the calls there were: every piece comes down, the world is rebuilt on the host and goes up again."""
    c0 = time.perf_counter()
    table, world = download_world()
    poses = eng.scene_poses()
    bodies = [world[int(table[c]):int(table[c + 1])] for c in range(len(table) - 1) if keep_body[c]]
    new_poses = [poses[c] for c in range(len(table) - 1) if keep_body[c]]
    if extra is not None:
        bodies.append(extra); new_poses.append(np.eye(4, dtype=np.float32))
    flat = [p for b in bodies for p in b]
    eng.upload_pieces([m for m, _ in flat], [c for _, c in flat])
    eng.scene_set_compounds(np.cumsum([0] + [len(b) for b in bodies]))
    eng.scene_set_poses(np.asarray(new_poses, np.float32))
    return (time.perf_counter() - c0) * 1e3


nc = len(eng.scene_compounds()) - 1
eng.scene_set_poses(random_poses(nc, 1))
res = {"scene": "configs[3]: bumpy torus x %d cells, %d pieces in %d compounds, every body posed" % (args.cells, n0, nc0), "reps": args.reps}
for s, name in ((0, "mesh"), (1, "convex")):
    d, f = bounds_times(s)
    res["bounds_dev_%s_device_ms" % name] = d
    res["set_poses_and_bounds_dev_%s_wall_ms" % name] = f
    res["parent_route_bounds_%s_ms" % name] = float(np.median([parent_bounds(s) for _ in range(args.base_reps)]))

# one body to append: the first piece of the scene, read once
body = [(eng.download_piece(0, 0), eng.download_piece(0, 1))]
as_piece = [{"mesh": body[0][0], "conv": body[0][1]}]
app, rem, app_alloc = [], [], []
for k in range(args.edit_reps):
    c0 = time.perf_counter()
    first = eng.scene_append([as_piece])
    app.append((time.perf_counter() - c0) * 1e3); app_alloc.append(eng.upload_stats()[1])
    c0 = time.perf_counter()
    eng.scene_remove([first])
    rem.append((time.perf_counter() - c0) * 1e3)
res.update(append_one_body_ms=float(np.median(app)), remove_one_body_ms=float(np.median(rem)), append_allocations=app_alloc)
base_app = []
for k in range(args.base_reps):
    table = eng.scene_compounds()
    base_app.append(parent_edit(np.ones(len(table) - 1, bool), extra=body))
    eng.scene_remove([len(table) - 1])
res["parent_route_append_ms"] = float(np.median(base_app))

# the cull: the lightest fifth of the bodies.  The parent's route to the same scene first (it puts the scene back), then the cull itself.
mass = eng.scene_mass(set=1)
ok = mass["status"] == 0
thr = float(np.float32(np.quantile(mass["mass"][ok], 0.2)))
marked = ok & (mass["mass"] <= np.float32(thr))
table, world = download_world()
poses = eng.scene_poses()
base_cull = []
for k in range(args.base_reps):
    base_cull.append(parent_edit(~marked))
    flat = world
    eng.upload_pieces([m for m, _ in flat], [c for _, c in flat]); eng.scene_set_compounds(table); eng.scene_set_poses(poses)
c0 = time.perf_counter()
reason, removed = eng.scene_cull(min_mass=thr, apply=False)
mark_ms = (time.perf_counter() - c0) * 1e3
c0 = time.perf_counter()
reason, removed = eng.scene_cull(min_mass=thr)
cull_ms = (time.perf_counter() - c0) * 1e3
assert removed == int(marked.sum()) and (reason != 0).sum() == removed
res.update(cull_mark_only_ms=mark_ms, cull_ms=cull_ms, cull_removed=int(removed), cull_bodies_before=int(len(table) - 1),
           pieces_after_cull=int(eng.scene_compounds()[-1]), parent_route_cull_ms=float(np.median(base_cull)))
for a, b in (("bounds_dev_mesh_device_ms", "parent_route_bounds_mesh_ms"), ("bounds_dev_convex_device_ms", "parent_route_bounds_convex_ms"),
             ("append_one_body_ms", "parent_route_append_ms"), ("cull_ms", "parent_route_cull_ms")):
    if res[a]:
        res["ratio_" + b[13:-3]] = res[b] / res[a]
if args.emul:
    res["rehearsal_on_cpu_emulation_not_a_measurement"] = True
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close()
