"""Cooked hulls on a resident scene: scene_fragments + event_hulls_dev + event_cook_dev (weld, convex hull and coplanar merge of the
points of the solids HullUsable refuses, device to device) against the route it replaces -- download of the refused pieces' points and
scipy.spatial.ConvexHull per piece (Qhull on the host; where scipy is installed).  This is NOT PhysX cooking, which nobody has
measured here: Qhull stands in for "a quickhull the embedder brings".

The scene and the protocol are bench_hulls.py's: BASELINE configs[3] (bumpy torus x 4096 cells) broken into its regrouped compounds,
then clicks with a 64-cell pattern; every timed step ends in a stream synchronisation; medians of --reps after --warmup; without
--child the script starts --runs fresh processes of itself and writes their lines and the spread of every median to --out
(profiles/cook_bench.json).  Measured, for all bodies and for the compounds each click made:
  hulls_and_cook_dev   event_hulls_dev + event_cook_dev with its records (only the refused solids are cooked)
  cook_selected_dev    event_cook_dev alone, with the hull records already on the device
  cook_all_dev         event_cook_dev alone with NULL records (every solid cooked)
  cook_with_download   event_cook(hull records): the host form, with its upload, allocations and download
  qhull                download_piece of the refused pieces + ConvexHull of each
and the share cooked and the share of the cooked that CookedUsable accepts.  --emul LIB rehearses the script on the CPU emulation at a
small size: no HIP events, and the line says that it is no measurement."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=4096)
ap.add_argument("--click-cells", type=int, default=64)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--clicks", type=int, default=8)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--rel-tol", type=float, default=1e-5)
ap.add_argument("--weld-dist", type=float, default=0.0)
ap.add_argument("--plane-tol", type=float, default=7e-6)
ap.add_argument("--out", default=None)
ap.add_argument("--emul", default=None)
ap.add_argument("--child", action="store_true")
args = ap.parse_args()

if not args.child:
    lines = []
    for r in range(args.runs):
        cmd = [sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(p.returncode)          # (a run that failed ends the script: nothing more is started)
        lines.append(json.loads(p.stdout.strip().splitlines()[-1]))
        sys.stderr.write("run %d of %d done\n" % (r + 1, args.runs))

    def spread(sect, k):
        vals = [ln[sect][k] for ln in lines]
        return {"median": float(np.median(vals)), "min": float(min(vals)), "max": float(max(vals))}
    summary = {sect: {k: spread(sect, k) for k, v in lines[0][sect].items() if isinstance(v, float)} for sect in ("all", "click_made_compounds") if lines[0].get(sect)}
    res = {"runs": len(lines), "method": "every number of a run is a median of %d calls after %d warm-ups; `summary` is median / min / max of those medians "
                                        "over %d fresh processes; the Qhull route is Qhull, not PhysX cooking" % (args.reps, args.warmup, len(lines)),
           "summary": summary, "per_run": lines}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

from surtr_amd import engine as E, scenes as S
try:
    from scipy.spatial import ConvexHull
except ImportError:
    ConvexHull = None

if args.emul:
    E._use_library_for_tests(args.emul)
    st = torch = None
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
TOLS = (args.rel_tol, args.weld_dist, args.plane_tol)


def timed(fn):
    """-> (wall ms, device ms or None) of one call that ends synchronised."""
    if st is not None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(st)
    t0 = time.perf_counter()
    fn()
    if st is not None:
        b.record(st)
        b.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    return wall, (a.elapsed_time(b) if st is not None else None)


def dev(nbytes):
    if st is None:
        b = np.zeros(max(nbytes, 1), np.uint8)
        return b, b.ctypes.data
    b = torch.zeros(max(nbytes, 1), dtype=torch.uint8, device="cuda")
    return b, b.data_ptr()


def host(b):
    return b if st is None else b.cpu().numpy()


class Buffers:
    """Device buffers at the capacities that are always enough: the hulls' (conv_nbrs polygons and indices) and the cooker's Euler
    bounds (conv_verts points, 2 conv_verts polygons, 6 conv_verts indices)."""

    def __init__(self, n, v, h):
        self.n, self.v, self.h = n, max(v, 1), max(h, 1)
        self.hull = [dev(48 * (n + 1)), dev(20 * self.h), dev(2 * self.h)]
        self.cook = [dev(64 * (n + 1)), dev(12 * self.v), dev(4 * self.v), dev(20 * 2 * self.v), dev(2 * 6 * self.v)]

    def hulls(self):
        eng.event_hulls_dev(self.hull[0][1], 48 * (self.n + 1), self.hull[1][1], self.h, self.hull[2][1], self.h)

    def cook_dev(self, selected):
        c = self.cook
        eng.event_cook_dev(self.hull[0][1] if selected else 0, TOLS[0], TOLS[1], TOLS[2], c[0][1], 64 * (self.n + 1), c[1][1], self.v, c[2][1], c[3][1], 2 * self.v,
                           c[4][1], 6 * self.v)

    def cook_records(self):
        raw = host(self.cook[0][0])
        return raw[:64].view(E.COOK_DTYPE)[0], raw[64:].view(E.COOK_DTYPE)

    def hull_records(self):
        return host(self.hull[0][0])[48:].view(E.HULL_DTYPE)


def sync():
    if st is not None:
        st.synchronize()


def pieces_of(compounds):
    table = eng.scene_compounds()
    return [p for c in compounds for p in range(int(table[c]), int(table[c + 1]))]


def qhull_route(pieces):
    out = []
    for p in pieces:
        pts = np.asarray(eng.download_piece(p, 1)["pos"], np.float64).reshape(-1, 3)
        try:
            out.append(ConvexHull(pts).vertices.shape[0])
        except Exception:       # (Qhull refuses a flat piece)
            out.append(0)
    return out


def med(rows, skip):
    rows = rows[skip:]
    out = {"ms": float(np.median([w for w, _ in rows]))}
    if st is not None:
        out["device_ms"] = float(np.median([d for _, d in rows]))
    return out


def measure(compounds, reps, warm):
    """compounds: a list, or None for all.  -> dict of medians."""
    pieces = pieces_of(range(len(eng.scene_compounds()) - 1) if compounds is None else compounds)
    c = eng.scene_fragments(compounds, flags=0)
    buf = Buffers(int(c.n_frag), int(c.conv_verts), int(c.conv_nbrs))
    buf.hulls(); sync()
    hrec = buf.hull_records().copy()
    rows = {"hulls_and_cook_dev": [], "cook_selected_dev": [], "cook_all_dev": [], "cook_with_download": []}
    for _ in range(warm + reps):
        rows["hulls_and_cook_dev"].append(timed(lambda: (buf.hulls(), buf.cook_dev(True), sync())))
        rows["cook_selected_dev"].append(timed(lambda: (buf.cook_dev(True), sync())))
        rows["cook_all_dev"].append(timed(lambda: (buf.cook_dev(False), sync())))
        rows["cook_with_download"].append(timed(lambda: eng.event_cook(hrec, *TOLS)))
    hdr_all, rec_all = buf.cook_records()
    hdr_all, rec_all = hdr_all.copy(), rec_all.copy()
    buf.cook_dev(True); sync()
    hdr, rec = buf.cook_records()
    assert hdr["status"] == 0 and hdr["nv_in"] == len(pieces) and hdr_all["status"] == 0
    took = rec[(rec["status"] & E.COOK_SKIPPED) == 0]
    refused = [p for p, r in zip(pieces, hrec) if not E.hull_usable(r, args.rel_tol)]
    assert len(refused) == took.shape[0]
    usable = sum(E.cooked_usable(r, args.plane_tol, args.weld_dist) for r in took)
    out = {"pieces": len(pieces), "conv_verts": int(c.conv_verts), "cooked": int(took.shape[0]), "cooked_share": took.shape[0] / max(1, len(pieces)),
           "cooked_usable_share_of_cooked": usable / max(1, took.shape[0]), "cooked_points": int(hdr["nv"]), "cooked_polygons": int(hdr["n_faces"]),
           "cooked_indices": int(hdr["n_idx"]), "status_or_of_cooked": int(np.bitwise_or.reduce(took["status"])) if took.shape[0] else 0,
           "withheld_of_cooked": int(((took["status"] & E.COOK_WITHHELD) != 0).sum()),
           "all_cooked_usable_share": sum(E.cooked_usable(r, args.plane_tol, args.weld_dist) for r in rec_all) / max(1, len(pieces)),
           "all_withheld": int(((rec_all["status"] & E.COOK_WITHHELD) != 0).sum()),
           "all_withheld_by_status": {name: int(((rec_all["status"] & bit) != 0).sum()) for name, bit in
                                      (("few", E.COOK_FEW), ("degenerate", E.COOK_DEGENERATE), ("nonfinite", E.COOK_NONFINITE), ("large", E.COOK_LARGE),
                                       ("failed", E.COOK_FAILED))}, "rel_tol": args.rel_tol, "plane_tol": args.plane_tol}
    for k, v in rows.items():
        for name, x in med(v, warm).items():
            out[k + "_" + name] = x
    if ConvexHull is not None:
        out["qhull_route_ms"] = med([timed(lambda: qhull_route(refused)) for _ in range(warm + reps)], warm)["ms"]      # (host work: no device time)
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


res = {"scene": "configs[3]: bumpy torus x %d cells, %d pieces in %d compounds; clicks with a %d-cell pattern" % (args.cells, n0, nc0, args.click_cells),
       "reps": args.reps, "warmup": args.warmup, "scipy": ConvexHull is not None, "cook_max_vertices": E.cook_max_vertices(),
       "all": measure(None, args.reps, args.warmup)}
per_click = []
for k in range(args.clicks):
    made = click(k)
    if made:
        per_click.append(measure(made, args.reps, args.warmup))
res["clicks"] = len(per_click)
res["click_made_compounds"] = {k: float(np.median([r[k] for r in per_click])) for k in per_click[0] if not isinstance(per_click[0][k], dict)} if per_click else {}
if args.emul:
    res["rehearsal_on_cpu_emulation_not_a_measurement"] = True
print(json.dumps(res))
eng.close()
