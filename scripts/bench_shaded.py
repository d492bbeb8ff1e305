"""Lit render buffers: event_shaded_dev (face normals per triangle vertex, device to device) against the only route there was before
it -- the event's download plus a host loop that walks the faces again and computes the same buffers.

Two sets of current fragments, both triangulated:
  event   the fragments of a BASELINE configs[3] event (bumpy torus x --cells cells, refit + render)
  click   after the one-event click on eight posed bodies of the resident configs[3] scene (bench_scene_bodies.py's one_event route,
          64-cell pattern): scene_fragments over the compounds the commit made
Measured per set: event_shaded_dev between two HIP events on the context's stream (median of --reps after --warmup), the same with the
LDS tier forced off (set_shade_tier(1): every fragment in global scratch), and the host route once per --base-reps: eng.download(), then
the faces, normals and the common-face rule in numpy over the whole event at once (no Python loop per half-edge: this is the host at its
best, and its tri_face must equal the device's).  `slowest_fragment` names the fragment with the most half-edges and the tier it took.
Without --child the script starts --runs fresh processes of itself, one after the other, each under its own time limit, and writes their
lines and the spread of every median to --out (profiles/shaded_bench.json).  --lib PATH measures another build of the library (the LDS
limit is a compile-time constant); --emul LIB rehearses the script on the CPU emulation at a small size: no measurement."""
import argparse, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=4096)
ap.add_argument("--click-cells", type=int, default=64)
ap.add_argument("--bodies", type=int, default=8)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--warmup", type=int, default=3)
ap.add_argument("--base-reps", type=int, default=2)
ap.add_argument("--runs", type=int, default=3)
ap.add_argument("--lds-limit", type=int, default=2048, help="SURTR_SHADE_LH of the library measured (for the tier named in the output)")
ap.add_argument("--out", default=None)
ap.add_argument("--lib", default=None)
ap.add_argument("--emul", default=None)
ap.add_argument("--child", action="store_true")
args = ap.parse_args()

if not args.child:
    lines = []
    for r in range(args.runs):
        cmd = ["timeout", "-k", "10", "500", sys.executable, os.path.abspath(__file__), "--child"] + [a for a in sys.argv[1:] if a != "--child"]
        p = subprocess.run(cmd, capture_output=True, text=True)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
            sys.exit(p.returncode)          # (a run that failed ends the script: nothing more is started)
        lines.append(json.loads(p.stdout.strip().splitlines()[-1]))
        sys.stderr.write("run %d of %d done\n" % (r + 1, args.runs))
    summary = {}
    for sect in ("event", "click"):
        summary[sect] = {k: {"median": float(np.median([ln[sect][k] for ln in lines])), "min": float(min(ln[sect][k] for ln in lines)),
                             "max": float(max(ln[sect][k] for ln in lines))} for k, v in lines[0][sect].items() if isinstance(v, float)}
    res = {"runs": len(lines), "method": "every number of a run is a median of %d calls after %d warm-ups (host route: of %d); `summary` is median / min / "
                                        "max of those medians over %d fresh processes" % (args.reps, args.warmup, args.base_reps, len(lines)),
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
    import torch      # (before the library: both then share torch's HIP runtime, as engine.lib() arranges for the product library)
    if args.lib:
        E._use_library_for_tests(args.lib)
    assert torch.cuda.is_available(), "no GPU: nothing can be measured here"
    st = torch.cuda.Stream()
    eng = E.Engine(0, stream=st.cuda_stream)


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
    return (time.perf_counter() - t0) * 1e3, (a.elapsed_time(b) if st is not None else None)


def host_route():
    """The download, then faces, normals and the common face of every triangle on the host -> (vnc, tri_face)."""
    ev = eng.download()
    vo, no = ev["mesh_vert_off"].astype(np.int64), ev["mesh_nbr_off"].astype(np.int64)
    nbr, pos = ev["mesh_nbr"].astype(np.int64), ev["mesh_pos"].astype(np.float64)
    V, H = pos.shape[0], nbr.shape[0]
    deg = np.diff(no)
    org = np.repeat(np.arange(V), deg)                                     # global vertex of every half-edge
    base = np.repeat(vo[:-1], np.diff(vo))                                 # first vertex of the fragment of every vertex
    tgt = nbr + base[org]
    # the twin (b -> a) of every (a -> b) by sorted keys, then the slot before it in ring(b)
    key = org * V + tgt
    order = np.argsort(key, kind="stable")
    twin = order[np.searchsorted(key[order], tgt * V + org)]
    slot = twin - no[tgt]
    nxt = no[tgt] + np.where(slot == 0, deg[tgt] - 1, slot - 1)
    lead, jmp = np.arange(H), nxt.copy()
    for _ in range(int(np.ceil(np.log2(max(H, 2))))):
        lead = np.minimum(lead, lead[jmp]); jmp = jmp[jmp]
    q0 = pos[org[lead]]
    t = np.cross(pos[org] - q0, pos[tgt] - q0)
    N = np.zeros((H, 3))
    for c in range(3):
        N[:, c] = np.bincount(lead, t[:, c], H)
    ln = np.sqrt((N * N).sum(1))
    n32 = np.where(ln[:, None] > 0, N / np.where(ln > 0, ln, 1.0)[:, None], 0.0).astype(np.float32)
    is_lead = lead == np.arange(H)
    # face numbers inside the fragment: leaders in id order
    frag_of_he = np.searchsorted(vo, org, side="right") - 1
    fno = np.cumsum(is_lead) - 1
    fno = fno - fno[no[vo[:-1]]][frag_of_he]
    # the common face of every triangle: the faces leaving corner a against the (vertex, face) pairs of the event
    io = ev["idx_off"].astype(np.int64)
    frag_of_idx = np.repeat(np.arange(io.shape[0] - 1), np.diff(io))
    gi = ev["idx"].astype(np.int64) + vo[frag_of_idx]
    a, b, c = gi[0::3], gi[1::3], gi[2::3]
    pairs = np.unique(org * H + lead)
    cnt = deg[a]
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]])
    cand = lead[np.repeat(no[a], cnt) + (np.arange(int(cnt.sum())) - np.repeat(first, cnt))]
    ok = np.isin(np.repeat(b, cnt) * H + cand, pairs) & np.isin(np.repeat(c, cnt) * H + cand, pairs)
    best = np.minimum.reduceat(np.where(ok, cand, H), first)
    assert (best < H).all(), "a triangle without a common face: this scene has none"
    vnc = np.empty((gi.shape[0], 9), np.float32)
    vnc[:, :3] = ev["mesh_pos"][gi]; vnc[:, 3:6] = np.repeat(n32[best], 3, axis=0); vnc[:, 6:] = 0.25
    return vnc, fno[best].astype(np.uint32)


def measure():
    c = eng.event_counts()
    n, nv = int(c.n_frag), int(c.n_idx)
    sizes = (16 * (n + 1), 36 * max(nv, 1), 4 * max(nv // 3, 1))
    if st is None:
        bufs = [np.zeros(b, np.uint8) for b in sizes]; ptrs = [b.ctypes.data for b in bufs]
    else:
        bufs = [torch.zeros(b, dtype=torch.uint8, device="cuda") for b in sizes]; ptrs = [b.data_ptr() for b in bufs]

    def run():
        eng.event_shaded_dev(ptrs[0], sizes[0], ptrs[1], nv, ptrs[2], nv // 3)
        if st is not None:
            st.synchronize()
    out = {"fragments": n, "vertices": nv, "mesh_half_edges": int(c.mesh_nbrs)}
    for name, limit in (("shaded_dev", 0), ("shaded_dev_global_tier_only", 1)):
        eng.set_shade_tier(limit)
        rows = [timed(run) for _ in range(args.warmup + args.reps)][args.warmup:]
        out[name + "_ms"] = float(np.median([w for w, _ in rows]))
        if st is not None:
            out[name + "_device_ms"] = float(np.median([d for _, d in rows]))
    eng.set_shade_tier(0)
    run()
    raw = [b if st is None else b.cpu().numpy() for b in bufs]
    hdr = raw[0][:16].view(E.SHADED_DTYPE)[0]
    assert hdr["status"] == 0 and hdr["n_vertices"] == nv
    rows, got = [], None
    for _ in range(args.base_reps):
        t0 = time.perf_counter(); got = host_route(); rows.append((time.perf_counter() - t0) * 1e3)
    out["host_route_ms"] = float(np.median(rows))
    # (a fragment whose rings list a neighbour twice takes the per-triangle fallback on the device; the host loop above does not know
    #  that rule, and those fragments are left out of the cross-check)
    rec = raw[0][16:16 * (n + 1)].view(E.SHADED_DTYPE)
    plain = np.repeat(rec["status"] == 0, rec["n_vertices"] // 3)
    out["fallback_fragments"] = int((rec["status"] != 0).sum())
    assert np.array_equal(got[1][plain], raw[2][:4 * (nv // 3)].view(np.uint32)[plain]), "the host route and the device disagree on a triangle's face"
    dn = np.abs(got[0][:, 3:6] - raw[1][:36 * nv].view(np.float32).reshape(-1, 9)[:, 3:6])[np.repeat(plain, 3)].max() if plain.any() else 0.0
    out["host_against_device_max_normal_difference"] = float(dn)
    ev = eng.download()
    he = np.diff(ev["mesh_nbr_off"].astype(np.int64)[ev["mesh_vert_off"].astype(np.int64)])
    k = int(he.argmax())
    out["slowest_fragment"] = {"fragment": k, "half_edges": int(he[k]), "tier": "LDS" if he[k] <= args.lds_limit else "global scratch",
                               "fragments_in_global_tier": int((he > args.lds_limit).sum())}
    return out


sc = S.torus_scene(args.cells, eng=eng)
res = {"scene": "configs[3]: bumpy torus x %d cells" % args.cells, "reps": args.reps, "warmup": args.warmup, "lds_limit": args.lds_limit,
       "library": os.path.basename(args.lib or args.emul or E.lib_path())}
eng.upload_pieces([sc["mesh"]], [sc["convex"]])
eng.upload_pattern(sc["face_off"], sc["v012"])
eng.place_cells(sc["scale"], sc["translate"])
eng.fracture_event(0, sc["n_cells"], flags=3)
res["event"] = measure()

# the resident scene, eight posed bodies, one click through one event (bench_scene_bodies.py), then the compounds its commit made
eng.scene_fracture_event(0, 0, sc["n_cells"], flags=0)
co, cp = eng.event_regroup()
eng.event_refit()
eng.scene_commit(co, cp)
eng.upload_pattern(*E.pattern_from_cells(E.voronoi_cells(S.uniform_seeds(args.click_cells))))
lat = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], np.float64)
lat = (lat / np.sqrt((lat * lat).sum(1))[:, None]).astype(np.float32)
L = float(np.linalg.norm(np.asarray(sc["scale"], np.float64)))
R = np.float32(0.04 * L)
aim = np.asarray(sc["mesh"]["pos"], np.float64)[np.random.default_rng(20261020).integers(sc["mesh"]["pos"].shape[0])]
centre = np.asarray(sc["translate"], np.float64)
d = aim - centre
d /= np.linalg.norm(d)
ray = np.r_[aim + d * L, -d, 4 * L].astype(np.float32)
hit = eng.scene_raycast(ray.reshape(1, 7))[0]
assert hit["piece"] >= 0
impact = (hit["pos"] + ray[3:6] * np.float32(0.01)).astype(np.float32)
com = eng.scene_mass(set=1)["com"]
near = np.argsort(((com - impact.astype(np.float64)) ** 2).sum(1), kind="stable")
targets = sorted([int(hit["compound"])] + [int(c) for c in near if int(c) != int(hit["compound"])][:args.bodies - 1], reverse=True)
cloud = (lat * R + impact).astype(np.float32)
eng.scene_apply_poses(targets)
eng.place_cells([R * np.float32(2)] * 3, impact)
mask = eng.scene_outside(targets, cloud, impact, float(R))
eng.scene_fracture_bodies(targets, 0, args.click_cells, outside=mask if mask.any() else None, flags=0)
co, cp, _ = eng.event_regroup_bodies(partial=True, sphere_points=cloud, origin=impact, radius=float(R))
eng.event_refit(); eng.event_counts()
_, first, n_new = eng.scene_commit(co, cp)[:3]
eng.scene_fragments(list(range(first, first + n_new)))
res["click"] = dict(measure(), bodies=len(targets), compounds_made=int(n_new))
if args.emul:
    res["rehearsal_on_cpu_emulation_not_a_measurement"] = True
print(json.dumps(res))
eng.close()
