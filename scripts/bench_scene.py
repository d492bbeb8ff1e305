"""One click cycle on a resident scene: BASELINE configs[3] (bumpy torus x 4096 cells) broken into its regrouped compounds, then
clicks on it -- pick (ray cast), scene event on the compound hit (a 64-cell pattern and the impact sphere at the hit), regroup,
refit, commit -- against the only route there was before the scene: download_piece of every piece, the same event on an engine
given the target compound alone, the world rebuilt on the host and uploaded again with upload_pieces.

The scene grows with every click, as it does in use: after WARM clicks the next --reps clicks are timed, each at another place.
Every step is a synchronous call (it ends in a stream synchronisation), so the host clock around it is a call time; the cycle and
the commit are bracketed by HIP events on the context's stream as well.  The commit's two parts (up to the end of the gather
kernel; the swap and derive_set over the whole scene) come from surtr_scene_commit_times.  The baseline takes about a second a
click and is timed --base-reps times.  Medians.  Prints one JSON line; --out FILE writes it there too
(profiles/scene_bench.json).  --emul LIB rehearses the script on the CPU emulation at a small size: no HIP events, and the line
says that it is no measurement."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from surtr_amd import engine as E, scenes as S

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=4096)
ap.add_argument("--click-cells", type=int, default=64)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--base-reps", type=int, default=3)
ap.add_argument("--out", default=None)
ap.add_argument("--emul", default=None)
args = ap.parse_args()
WARM = 3

if args.emul:
    E._use_library_for_tests(args.emul)
    st = None
    eng = E.Engine(0)
else:
    import torch
    assert torch.cuda.is_available(), "no GPU: nothing can be measured here"
    st = torch.cuda.Stream()
    eng = E.Engine(0, stream=st.cuda_stream)

sc = S.torus_scene(args.cells, eng=eng)
click_cells = E.voronoi_cells(S.uniform_seeds(args.click_cells))
click_pattern = E.pattern_from_cells(click_cells)

# the scene: configs[3], every regrouped compound a body
eng.upload_pieces([sc["mesh"]], [sc["convex"]])
eng.upload_pattern(sc["face_off"], sc["v012"])
eng.place_cells(sc["scale"], sc["translate"])
eng.scene_fracture_event(0, 0, sc["n_cells"], flags=0)
co, cp = eng.event_regroup()
eng.event_refit()
n0, _, nc0, _ = eng.scene_commit(co, cp)
eng.upload_pattern(*click_pattern)

lat = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], np.float64)
lat = (lat / np.sqrt((lat * lat).sum(1))[:, None]).astype(np.float32)
L = float(np.linalg.norm(np.asarray(sc["scale"], np.float64)))
R = np.float32(0.04 * L)                      # impact radius: a few fragments across
rng = np.random.default_rng(20261018)
targets = np.asarray(sc["mesh"]["pos"], np.float64)[rng.choice(sc["mesh"]["pos"].shape[0], WARM + args.reps + args.base_reps + 8)]
centre = np.asarray(sc["translate"], np.float64)


def ray_at(k):
    d = targets[k] - centre
    d /= np.linalg.norm(d)
    return np.r_[targets[k] + d * L, -d, 4 * L].astype(np.float32)


def placement(hit, ray):
    impact = (hit["pos"] + ray[3:6] * np.float32(0.01)).astype(np.float32)
    return impact, (lat * R + impact).astype(np.float32)


def device_ms(a, b):
    b.synchronize()
    return a.elapsed_time(b)


def click(k):
    """One cycle on the resident scene -> wall milliseconds per step."""
    ray = ray_at(k)
    t = {}
    if st is not None:
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record(st)
    c0 = time.perf_counter()
    hit = eng.pieces_raycast(ray.reshape(1, 7))[0]
    assert hit["piece"] >= 0
    table = eng.scene_compounds()
    comp = int(np.searchsorted(table, int(hit["piece"]), side="right")) - 1
    impact, cloud = placement(hit, ray)
    c1 = time.perf_counter()
    eng.place_cells([R * np.float32(2)] * 3, impact)
    cnt = eng.scene_fracture_event(comp, 0, args.click_cells, flags=0)
    c2 = time.perf_counter()
    co, cp = eng.event_regroup(partial=True, sphere_points=cloud, origin=impact, radius=float(R))
    c3 = time.perf_counter()
    eng.event_refit()
    eng.event_counts()
    c4 = time.perf_counter()
    if st is not None:
        ev[1].record(st)
    n, first, n_new, _ = eng.scene_commit(co, cp)
    c5 = time.perf_counter()
    if st is not None:
        ev[2].record(st)
        t["cycle_device_ms"] = device_ms(ev[0], ev[2]); t["commit_device_ms"] = device_ms(ev[1], ev[2])
    g, d = eng.scene_commit_times()
    t.update(pick_ms=(c1 - c0) * 1e3, event_ms=(c2 - c1) * 1e3, regroup_ms=(c3 - c2) * 1e3, refit_ms=(c4 - c3) * 1e3, commit_ms=(c5 - c4) * 1e3,
             cycle_ms=(c5 - c0) * 1e3, commit_gather_part_ms=g, commit_derive_part_ms=d, pieces=n, fragments=cnt.n_frag, allocations=eng.upload_stats()[1])
    return t


def baseline_click(k):
    """The same click by the calls there were before the scene: the world lives on the host between clicks."""
    ray = ray_at(k)
    t = {}
    c0 = time.perf_counter()
    hit = eng.pieces_raycast(ray.reshape(1, 7))[0]
    assert hit["piece"] >= 0
    table = eng.scene_compounds()
    comp = int(np.searchsorted(table, int(hit["piece"]), side="right")) - 1
    impact, cloud = placement(hit, ray)
    c1 = time.perf_counter()
    n = int(table[-1])
    world = [(eng.download_piece(p, 0), eng.download_piece(p, 1)) for p in range(n)]
    c2 = time.perf_counter()
    a, b = int(table[comp]), int(table[comp + 1])
    other = E.Engine(0) if st is None else E.Engine(0, stream=st.cuda_stream)
    other.upload_pieces([m for m, _ in world[a:b]], [c for _, c in world[a:b]])
    other.upload_pattern(*click_pattern)
    other.place_cells([R * np.float32(2)] * 3, impact)
    other.fracture_event(0, args.click_cells, flags=0)
    co, cp = other.event_regroup(partial=True, sphere_points=cloud, origin=impact, radius=float(R))
    other.event_refit()
    frags = other.download()
    c3 = time.perf_counter()
    fm, fc = S.fragments_as_pieces(frags)
    new = [[(fm[q], fc[q]) for q in cp[co[i]:co[i + 1]] if fm[q]["pos"].shape[0] >= 4 and fc[q]["pos"].shape[0] >= 4 and not frags["frag_status"][q]]
           for i in range(len(co) - 1)]
    new = [x for x in new if x]
    rebuilt = world[:a] + world[b:] + [p for x in new for p in x]
    sizes = [int(table[i + 1] - table[i]) for i in range(len(table) - 1) if i != comp] + [len(x) for x in new]
    c4 = time.perf_counter()
    eng.upload_pieces([m for m, _ in rebuilt], [c for _, c in rebuilt])
    eng.scene_set_compounds(np.cumsum([0] + sizes))
    c5 = time.perf_counter()
    other.close()
    t.update(pick_ms=(c1 - c0) * 1e3, download_all_pieces_ms=(c2 - c1) * 1e3, event_on_target_ms=(c3 - c2) * 1e3, host_rebuild_ms=(c4 - c3) * 1e3,
             upload_world_ms=(c5 - c4) * 1e3, cycle_ms=(c5 - c0) * 1e3, pieces=len(rebuilt))
    return t


def median_of(rows):
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


for k in range(WARM):
    click(k)
rows = [click(WARM + k) for k in range(args.reps)]
base = [baseline_click(WARM + args.reps + k) for k in range(args.base_reps)]
res = {"scene": "configs[3]: bumpy torus x %d cells, %d pieces in %d compounds; clicks with a %d-cell pattern" % (args.cells, n0, nc0, args.click_cells),
       "reps": args.reps, "base_reps": args.base_reps, "scene_click": median_of(rows), "parent_route_click": median_of(base),
       "pieces_first_timed": rows[0]["pieces"], "pieces_last_timed": rows[-1]["pieces"],
       "allocations_per_commit": [r["allocations"] for r in rows]}
if args.emul:
    res["rehearsal_on_cpu_emulation_not_a_measurement"] = True
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close()
