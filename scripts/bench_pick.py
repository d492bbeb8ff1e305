"""Picking on the resident pieces of BASELINE configs[3] (bumpy torus x 4096 cells -> pieces_from_event): one ray, 4 096 rays and
one sphere with the mass gate through query_dev.hip, against the only route there was before it -- surtr_download_piece for every
piece, then the float64 host loop of tests/test_pick_queries.py.

Device times are HIP events on the context's stream around the _dev calls after a warm-up (median of REPS); the wall time of the
synchronous host forms (copies and synchronisation included) is what is held against the download-and-loop route.
Prints one JSON line; --out FILE writes it there too (profiles/pick_bench.json)."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from surtr_amd import engine as E, scenes as S
import test_pick_queries as T

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=4096)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

st = torch.cuda.Stream()
eng = E.Engine(0, stream=st.cuda_stream)
sc = S.torus_scene(args.cells, eng=eng)
eng.upload_pieces([sc["mesh"]], [sc["convex"]])
eng.upload_pattern(sc["face_off"], sc["v012"])
eng.place_cells(sc["scale"], sc["translate"])
eng.fracture_event(0, sc["n_cells"])
n = eng.pieces_from_event()

# the route of the parent commit: every piece back to the host, then the loop
t0 = time.perf_counter()
solids = [eng.download_piece(p, set=1) for p in range(n)]
t1 = time.perf_counter()
ref_eng = E.Engine(0)
refs = [T.RefSolid(ref_eng, s) for s in solids]
t2 = time.perf_counter()
lo, hi, L = T.scene_size(refs)
rays = T.random_rays(lo, hi, L, n=4096)
q = rays[0].astype(np.float64)
t3 = time.perf_counter()
best = min(((a["t"], p) for p, a in enumerate(r.ray(q) for r in refs) if a is not None and a["hit"]), default=(0.0, -1))
t4 = time.perf_counter()

hit = eng.pieces_raycast(rays[:1])[0]
assert hit["piece"] == best[1], (hit, best)
mass = eng.pieces_mass(set=1)
sphere = np.r_[hit["pos"], 0.05 * L].astype(np.float32).reshape(1, 4)


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


with torch.cuda.stream(st):
    d_r = torch.from_numpy(rays).cuda(); d_s = torch.from_numpy(sphere).cuda()
    d_h = torch.zeros(rays.shape[0] * 48, dtype=torch.uint8, device="cuda")
    d_m = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_w = torch.zeros(n * 96, dtype=torch.uint8, device="cuda")
    st.synchronize()
eng.pieces_mass_dev(d_w.data_ptr(), d_w.numel(), set=1)
res = {
    "scene": "configs[3]: bumpy torus x %d cells, %d resident pieces" % (args.cells, n), "pieces": n, "reps": args.reps,
    "download_all_pieces_ms": (t1 - t0) * 1e3, "host_faces_and_planes_ms": (t2 - t1) * 1e3, "host_one_ray_loop_ms": (t4 - t3) * 1e3,
    "parent_route_one_ray_wall_ms": (t1 - t0 + t2 - t1 + t4 - t3) * 1e3,
    "one_ray_wall_ms": wall(lambda: eng.pieces_raycast(rays[:1])),
    "rays_4096_wall_ms": wall(lambda: eng.pieces_raycast(rays)),
    "one_sphere_gate_wall_ms": wall(lambda: eng.pieces_overlap(sphere, mass=mass)),
    "one_ray_device_ms": device(lambda: eng.pieces_raycast_dev(1, d_r.data_ptr(), d_h.data_ptr(), d_h.numel())),
    "rays_4096_device_ms": device(lambda: eng.pieces_raycast_dev(4096, d_r.data_ptr(), d_h.data_ptr(), d_h.numel())),
    "one_sphere_gate_device_ms": device(lambda: eng.pieces_overlap_dev(1, d_s.data_ptr(), d_m.data_ptr(), d_m.numel(), dev_mass=d_w.data_ptr())),
    "flagged_pieces": int((eng.pieces_query_status(n) != 0).sum()),
}
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close(); ref_eng.close()
