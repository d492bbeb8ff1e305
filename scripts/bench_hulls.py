"""Collision hulls on a resident scene: scene_fragments + event_hulls_dev (face loops, planes and the verdict of every Convex, device to
device) against the only route there was before it -- download_piece(set 1) of every piece, extract_faces per piece, the planes in numpy.

The scene is bench_scene_init.py's: BASELINE configs[3] (bumpy torus x 4096 cells) broken into its regrouped compounds, then clicks with
a 64-cell pattern.  Measured:
  all          scene_fragments(every compound, flags 0) + event_hulls_dev; event_hulls_dev alone; event_hulls with its download
  click        after each click's commit, scene_fragments + event_hulls_dev for only the compounds the commit made
  parent       the host route over the same pieces (few repetitions: it takes seconds)
Every timed step ends in a stream synchronisation, so the host clock around it is a call time; the device time comes from HIP events on
the context's stream.  The kernels' own times are slots 14 (count + scan) and 15 (emit + errors) of surtr_kernel_times, taken in
repetitions of their own.  Medians of --reps after --warmup.  Without --child the script starts --runs fresh processes of itself, one
after the other, and writes their lines and the spread of every median to --out (profiles/hulls_bench.json).  --emul LIB rehearses the
script on the CPU emulation at a small size: no HIP events, and the line says that it is no measurement."""
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
ap.add_argument("--base-reps", type=int, default=2)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--rel-tol", type=float, default=1e-5)
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

    def spread(path):
        vals = []
        for ln in lines:
            v = ln
            for k in path:
                v = v[k]
            vals.append(v)
        return {"median": float(np.median(vals)), "min": float(min(vals)), "max": float(max(vals))}
    summary = {}
    for sect in ("all", "click_made_compounds"):
        if lines[0].get(sect):
            summary[sect] = {k: spread((sect, k)) for k, v in lines[0][sect].items() if isinstance(v, float)}
    res = {"runs": len(lines), "method": "every number of a run is a median of %d calls after %d warm-ups; `summary` is median / min / max of "
                                        "those medians over %d fresh processes" % (args.reps, args.warmup, len(lines)),
           "summary": summary, "per_run": lines}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sys.exit(0)

from surtr_amd import engine as E, scenes as S

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


class Buffers:
    """Device buffers of the capacities that are always enough: one header + a record per fragment, conv_nbrs polygons and indices."""

    def __init__(self, n, h):
        self.n, self.h = n, max(h, 1)
        if st is None:
            self.b = [np.zeros(48 * (n + 1), np.uint8), np.zeros(20 * self.h, np.uint8), np.zeros(2 * self.h, np.uint8)]
            self.p = [x.ctypes.data for x in self.b]
        else:
            self.b = [torch.zeros(48 * (n + 1), dtype=torch.uint8, device="cuda"), torch.zeros(20 * self.h, dtype=torch.uint8, device="cuda"),
                      torch.zeros(2 * self.h, dtype=torch.uint8, device="cuda")]
            self.p = [x.data_ptr() for x in self.b]

    def run(self):
        eng.event_hulls_dev(self.p[0], 48 * (self.n + 1), self.p[1], self.h, self.p[2], self.h)

    def records(self):
        raw = self.b[0] if st is None else self.b[0].cpu().numpy()
        return raw[:48].view(E.HULL_DTYPE)[0], raw[48:].view(E.HULL_DTYPE)


def sync():
    if st is not None:
        st.synchronize()


def pieces_of(compounds):
    table = eng.scene_compounds()
    return [p for c in compounds for p in range(int(table[c]), int(table[c + 1]))]


def newell(pos, loop):
    q = pos[loop].astype(np.float64)
    d = q[1:] - q[0]
    n = np.cross(d[:-1], d[1:]).sum(0)
    ln = np.sqrt((n * n).sum())
    if ln == 0.0:
        return np.zeros(4, np.float32)
    n = n / ln
    t = q @ n
    return np.r_[n, -(t.max() + t.min()) / 2.0].astype(np.float32)


def parent_route(pieces):
    out = []
    for p in pieces:
        s = eng.download_piece(p, 1)
        fo, fi = eng.extract_faces(s)
        out.append([newell(s["pos"], fi[int(fo[f]):int(fo[f + 1])]) for f in range(len(fo) - 1)])
    return out


def med(rows, skip):
    rows = rows[skip:]
    out = {"ms": float(np.median([w for w, _ in rows]))}
    if st is not None:
        out["device_ms"] = float(np.median([d for _, d in rows]))
    return out


def measure(compounds, reps, warm, base_reps):
    """compounds: a list, or None for all.  -> dict of medians."""
    pieces = pieces_of(range(len(eng.scene_compounds()) - 1) if compounds is None else compounds)
    c = eng.scene_fragments(compounds, flags=0)
    buf = Buffers(int(c.n_frag), int(c.conv_nbrs))
    rows = {"fragments_and_hulls_dev": [], "hulls_dev": [], "hulls_with_download": []}
    for _ in range(warm + reps):
        rows["fragments_and_hulls_dev"].append(timed(lambda: (eng.scene_fragments_async(compounds, flags=0), buf.run(), sync())))
        rows["hulls_dev"].append(timed(lambda: (buf.run(), sync())))
        rows["hulls_with_download"].append(timed(lambda: eng.event_hulls()))
    hdr, rec = buf.records()
    assert hdr["status"] == 0 and hdr["nv"] == len(pieces)
    usable = sum(E.hull_usable(r, args.rel_tol) for r in rec)
    out = {"pieces": len(pieces), "conv_verts": int(c.conv_verts), "conv_nbrs": int(c.conv_nbrs), "polygons": int(hdr["n_faces"]), "indices": int(hdr["n_idx"]),
           "withheld": int(((rec["status"] & E.HULL_WITHHELD) != 0).sum()), "flat": int(((rec["status"] & E.HULL_FLAT) != 0).sum()),
           "usable_share_at_rel_tol": usable / max(1, len(pieces)), "rel_tol": args.rel_tol}
    for k, v in rows.items():
        for name, x in med(v, warm).items():
            out[k + "_" + name] = x
    if base_reps:
        for name, x in med([timed(lambda: parent_route(pieces)) for _ in range(base_reps)], 0).items():
            out["parent_" + name] = x
    if st is not None:      # the kernels alone, with the per-kernel HIP events on (reps of their own: the events cost launches)
        eng.set_profiling(True)
        a, b = [], []
        for _ in range(warm + reps):
            buf.run()
            ms = (E.ctypes.c_float * 16)()
            eng._ck(E.lib().surtr_kernel_times(eng._h, ms))
            a.append(ms[14]); b.append(ms[15])
        eng.set_profiling(False)
        out["count_scan_kernels_ms"] = float(np.median(a[warm:])); out["emit_errors_kernels_ms"] = float(np.median(b[warm:]))
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
       "reps": args.reps, "warmup": args.warmup, "base_reps": args.base_reps, "all": measure(None, args.reps, args.warmup, args.base_reps)}
per_click = []
for k in range(args.clicks):
    made = click(k)
    if made:
        per_click.append(measure(made, args.reps, args.warmup, 1))
res["clicks"] = len(per_click)
res["click_made_compounds"] = {k: float(np.median([r[k] for r in per_click])) for k in per_click[0]} if per_click else {}
if args.emul:
    res["rehearsal_on_cpu_emulation_not_a_measurement"] = True
print(json.dumps(res))
eng.close()
