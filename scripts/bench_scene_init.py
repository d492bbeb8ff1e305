"""InitCompound on a resident scene: scene_fragments (the resident pieces as the current fragments, device to device, triangulated)
against the only route there was before it -- download_piece of those pieces, both sets, then load_fragments and event_triangulate.

The scene is bench_scene.py's: BASELINE configs[3] (bumpy torus x 4096 cells) broken into its regrouped compounds, then clicks with a
64-cell pattern.  Measured, each next to the parent route over the same pieces:
  all          scene_fragments(every compound, EVT_RENDER) alone, and with download()
  click        after each click's commit, the same for only the compounds the commit made
Every timed step ends in a stream synchronisation, so the host clock around it is a call time; the device time of the call comes from
HIP events on the context's stream.  The copy kernel's own time is slot 12 of surtr_kernel_times (set_profiling), taken in reps of its
own, and is set against the bytes it moves: every word of the listed solids is read once and written once.  Medians.  Prints one JSON
line; --out FILE writes it there too (profiles/scene_init_bench.json).  --emul LIB rehearses the script on the CPU emulation at a
small size: no HIP events, and the line says that it is no measurement."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from surtr_amd import engine as E, scenes as S

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=4096)
ap.add_argument("--click-cells", type=int, default=64)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--clicks", type=int, default=8)
ap.add_argument("--base-reps", type=int, default=2)
ap.add_argument("--out", default=None)
ap.add_argument("--emul", default=None)
args = ap.parse_args()
HBM_COPY_TBS = 6.29      # what a float4 copy kernel reaches on this part (79 % of the 8 TB/s of the data sheet)

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
click_pattern = E.pattern_from_cells(E.voronoi_cells(S.uniform_seeds(args.click_cells)))
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
R = np.float32(0.04 * L)
rng = np.random.default_rng(20261018)
targets = np.asarray(sc["mesh"]["pos"], np.float64)[rng.choice(sc["mesh"]["pos"].shape[0], args.clicks + 8)]
centre = np.asarray(sc["translate"], np.float64)


def timed(fn):
    """-> (wall ms, device ms or None) of one call that ends synchronised."""
    if st is not None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
    t0 = time.perf_counter()
    fn()
    wall = (time.perf_counter() - t0) * 1e3
    if st is None:
        return wall, None
    b.record(st)
    b.synchronize()
    return wall, a.elapsed_time(b)


def pieces_of(compounds):
    table = eng.scene_compounds()
    return [p for c in compounds for p in range(int(table[c]), int(table[c + 1]))]


def parent_route(pieces, download):
    m = [eng.download_piece(p, 0) for p in pieces]
    c = [eng.download_piece(p, 1) for p in pieces]
    eng.load_fragments(m, c)
    eng.event_triangulate(False)
    eng.download() if download else eng.event_counts()


def measure(compounds, reps, base_reps):
    """compounds: a list, or None for all.  -> dict of medians."""
    pieces = pieces_of(range(len(eng.scene_compounds()) - 1) if compounds is None else compounds)
    rows = {"call": [], "call_download": [], "parent": [], "parent_download": []}
    for _ in range(reps):
        rows["call"].append(timed(lambda: eng.scene_fragments(compounds)))
        rows["call_download"].append(timed(lambda: (eng.scene_fragments(compounds), eng.download())))
    for _ in range(base_reps):
        rows["parent"].append(timed(lambda: parent_route(pieces, False)))
        rows["parent_download"].append(timed(lambda: parent_route(pieces, True)))
    c = eng.scene_fragments(compounds)
    out = {"pieces": len(pieces), "mesh_verts": int(c.mesh_verts), "conv_verts": int(c.conv_verts), "indices": int(c.n_idx), "flagged": int(c.n_failed)}
    for k, v in rows.items():
        out[k + "_ms"] = float(np.median([w for w, _ in v]))
        if st is not None:
            out[k + "_device_ms"] = float(np.median([d for _, d in v]))
    # the copy kernel alone, with the per-kernel HIP events on (reps of their own: the events cost launches)
    words = 5 * (int(c.mesh_verts) + int(c.conv_verts)) + int(c.mesh_nbrs) + int(c.conv_nbrs)      # pos 3, loff, llen per vertex; the rings
    out["copy_bytes"] = 8 * words                                                                      # read once, written once
    if st is not None:
        eng.set_profiling(True)
        ms, faces = [], []
        for _ in range(reps):
            eng.scene_fragments(compounds)
            ms.append(eng.scene_fragments_ms()); faces.append(eng.kernel_times()["faces"])
        eng.set_profiling(False)
        out["copy_kernel_ms"] = float(np.median(ms)); out["faces_kernel_ms"] = float(np.median(faces))
        out["copy_GBps"] = out["copy_bytes"] / (out["copy_kernel_ms"] * 1e-3) / 1e9
        out["copy_share_of_hbm_copy_rate"] = out["copy_GBps"] / (HBM_COPY_TBS * 1e3)
    return out


def click(k):
    """One click of bench_scene.py on the resident scene -> the compounds its commit made."""
    d = targets[k] - centre
    d /= np.linalg.norm(d)
    ray = np.r_[targets[k] + d * L, -d, 4 * L].astype(np.float32)
    hit = eng.pieces_raycast(ray.reshape(1, 7))[0]
    assert hit["piece"] >= 0
    table = eng.scene_compounds()
    comp = int(np.searchsorted(table, int(hit["piece"]), side="right")) - 1
    impact = (hit["pos"] + ray[3:6] * np.float32(0.01)).astype(np.float32)
    cloud = (lat * R + impact).astype(np.float32)
    eng.place_cells([R * np.float32(2)] * 3, impact)
    eng.scene_fracture_event(comp, 0, args.click_cells, flags=0)
    co, cp = eng.event_regroup(partial=True, sphere_points=cloud, origin=impact, radius=float(R))
    eng.event_refit()
    n, first, n_new, _ = eng.scene_commit(co, cp)
    return list(range(first, first + n_new))


eng.scene_fragments(None); eng.download()      # (warm: the arena and the blob are grown)
res = {"scene": "configs[3]: bumpy torus x %d cells, %d pieces in %d compounds; clicks with a %d-cell pattern" % (args.cells, n0, nc0, args.click_cells),
       "reps": args.reps, "base_reps": args.base_reps, "hbm_copy_rate_TBps_taken_as_full": HBM_COPY_TBS,
       "all": measure(None, args.reps, args.base_reps)}
per_click = []
for k in range(args.clicks):
    made = click(k)
    if made:
        per_click.append(measure(made, max(3, args.reps // 4), 1))
res["clicks"] = len(per_click)
res["click_made_compounds"] = {k: float(np.median([r[k] for r in per_click])) for k in per_click[0]} if per_click else {}
if args.emul:
    res["rehearsal_on_cpu_emulation_not_a_measurement"] = True
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
eng.close()
