"""The pattern library, three measurements in one process, medians over --reps:

1. switch: making another pattern the installed one.  pattern_select (device to device) against the two routes there were,
   upload_pattern of the host arrays and build_cells of the seeds, for the reference's two patterns: 128 cells at mean 0.01 and 1024
   cells at mean 1.0 (Src/Surtr.cpp:1806-1807).  Every timed call installs the pattern that is NOT installed; host clock around the
   call and around call + synchronisation.
2. place: place_cells_patterns against place_cells_impacts for eight instances of one pattern (each of the two), call + synchronisation.
3. frame: K = 8 impacts of one frame on eight posed bodies of the scene of scripts/bench_scene_impacts.py (BASELINE configs[3] broken
   into its regrouped compounds), the impacts alternating between two patterns (--frame-cells) and between partial and not partial:
   (a) the sequential cycles -- per impact upload_pattern of its pattern, scene_apply_poses, place_cells, scene_outside when partial,
   scene_fracture_bodies, event_regroup_bodies, event_refit, scene_commit; (b) one event -- place_cells_patterns, scene_outside_impacts
   (the bytes of the impacts that are not partial cleared), scene_fracture_impacts over CELLS_ALL, event_regroup_impacts_partial,
   event_refit, one scene_commit.  Two engines, one per route, the same seeded frames; pieces and fragments must agree every frame.

Prints one JSON line; --out FILE appends it.  --emul LIB rehearses the script on the CPU emulation at a small size: the line then says
that it is no measurement."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from surtr_amd import engine as E, scenes as S

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=4096)
ap.add_argument("--frame-cells", default="64,32")
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--impacts", type=int, default=8)
ap.add_argument("--out", default=None)
ap.add_argument("--emul", default=None)
args = ap.parse_args()
WARM = 3

if args.emul:
    E._use_library_for_tests(args.emul)
    torch = None
    sync = lambda: None
    streams = [None, None]
    engs = [E.Engine(0), E.Engine(0)]
else:
    import torch
    assert torch.cuda.is_available(), "no GPU: nothing can be measured here"
    sync = torch.cuda.synchronize
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    engs = [E.Engine(0, stream=s.cuda_stream) for s in streams]


def timed(call):
    """-> (milliseconds until the call returns, until the device is idle after it)."""
    sync()
    t0 = time.perf_counter()
    call()
    t1 = time.perf_counter()
    sync()
    return (t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3


def med(rows):
    a = np.asarray(rows, np.float64)
    return {"call_ms": float(np.median(a[:, 0])), "call_and_sync_ms": float(np.median(a[:, 1])), "min_call_and_sync_ms": float(a[:, 1].min()),
            "max_call_and_sync_ms": float(a[:, 1].max())}


res = {"reps": args.reps, "warm": WARM}

# ---- 1. switch, 2. place
ref_patterns = [(128, 0.01), (1024, 1.0)] if not args.emul else [(12, 0.01), (24, 1.0)]
eng = E.Engine(0)
pats = []
for n, mean in ref_patterns:
    seeds = S.pattern_seeds(n, mean)
    eng.build_cells(seeds)
    got = eng.download_cells()
    pats.append(dict(seeds=seeds, face_off=got["cell_face_off"], v012=got["v012"], id=eng.pattern_store()))
res["patterns"] = [{"cells": n, "mean": m, "faces": int(p["v012"].shape[0])} for (n, m), p in zip(ref_patterns, pats)]
rows = {k: [[], []] for k in ("pattern_select", "upload_pattern", "build_cells")}
for rep in range(WARM + args.reps):
    for which in (0, 1):           # (the other one is installed: every call is a switch)
        p = pats[which]
        for name, call in (("pattern_select", lambda: eng.pattern_select(p["id"])), ("upload_pattern", lambda: eng.upload_pattern(p["face_off"], p["v012"])),
                           ("build_cells", lambda: eng.build_cells(p["seeds"]))):
            eng.pattern_select(pats[1 - which]["id"])
            t = timed(call)
            if rep >= WARM:
                rows[name][which].append(t)
res["switch"] = {name: {str(ref_patterns[w][0]): med(rows[name][w]) for w in (0, 1)} for name in rows}
K8 = 8
scales = np.float32([[1.0 + 0.1 * i] * 3 for i in range(K8)])
shifts = np.float32([[0.3 * i, 0.0, 0.1 * i] for i in range(K8)])
rows = {k: [[], []] for k in ("place_cells_patterns", "place_cells_impacts")}
for which in (0, 1):
    eng.pattern_select(pats[which]["id"])
    for rep in range(WARM + args.reps):
        for name, call in (("place_cells_patterns", lambda: eng.place_cells_patterns([pats[which]["id"]] * K8, scales, shifts)),
                           ("place_cells_impacts", lambda: eng.place_cells_impacts(scales, shifts))):
            t = timed(call)
            if rep >= WARM:
                rows[name][which].append(t)
    a, b = (eng.place_cells_patterns([pats[which]["id"]] * K8, scales, shifts), eng.download_planes(True))[1], (eng.place_cells_impacts(scales, shifts), eng.download_planes(True))[1]
    assert a.tobytes() == b.tobytes()
res["place_8_instances"] = {name: {str(ref_patterns[w][0]): med(rows[name][w]) for w in (0, 1)} for name in rows}
eng.close()

# ---- 3. the frame
K = args.impacts
frame_cells = [int(x) for x in args.frame_cells.split(",")]
sc = S.torus_scene(args.cells, eng=engs[0])
fpat = [E.pattern_from_cells(E.voronoi_cells(S.uniform_seeds(n, S.SEED + k))) for k, n in enumerate(frame_cells)]
for e in engs:
    e.upload_pieces([sc["mesh"]], [sc["convex"]])
    e.upload_pattern(sc["face_off"], sc["v012"])
    e.place_cells(sc["scale"], sc["translate"])
    e.scene_fracture_event(0, 0, sc["n_cells"], flags=0)
    co, cp = e.event_regroup()
    e.event_refit()
    n0, _, nc0, _ = e.scene_commit(co, cp)
for p in fpat:                    # the one-event engine keeps both patterns resident
    engs[1].upload_pattern(*p)
    engs[1].pattern_store()

lat = np.array([(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], np.float64)
lat = (lat / np.sqrt((lat * lat).sum(1))[:, None]).astype(np.float32)
L = float(np.linalg.norm(np.asarray(sc["scale"], np.float64)))
R = np.float32(0.04 * L)
rng = np.random.default_rng(20261020)
aims = np.asarray(sc["mesh"]["pos"], np.float64)[rng.choice(sc["mesh"]["pos"].shape[0], 4 * K * (WARM + args.reps) + 64)]
centre = np.asarray(sc["translate"], np.float64)
NUDGE = np.eye(4, dtype=np.float32)
NUDGE[:3, 3] = np.float32(1e-4 * L)


def pick(e, first):
    """Untimed: rays from `first` on until K different bodies are hit; impact i takes pattern i % 2 and is partial when i is even."""
    impacts, seen, k = [], set(), first
    while len(impacts) < K:
        d = aims[k] - centre
        d /= np.linalg.norm(d)
        ray = np.r_[aims[k] + d * L, -d, 4 * L].astype(np.float32)
        hit = e.scene_raycast(ray.reshape(1, 7))[0]
        k += 1
        if hit["piece"] < 0 or int(hit["compound"]) in seen:
            continue
        seen.add(int(hit["compound"]))
        i = len(impacts)
        r = np.float32(R * np.float32(0.8 + 0.1 * (i % 4)))
        pos = (hit["pos"] + ray[3:6] * np.float32(0.01)).astype(np.float32)
        impacts.append(dict(target=int(hit["compound"]), origin=pos, radius=float(r), scale=np.float32([r * np.float32(2)] * 3), cloud=(lat * r + pos).astype(np.float32),
                            pattern=i % 2, partial=i % 2 == 0))
    poses = e.scene_poses()
    poses[[im["target"] for im in impacts]] = NUDGE
    e.scene_set_poses(poses)
    return impacts, k


def sequential(e, impacts):
    t0 = time.perf_counter()
    frags, gone = 0, []
    for im in impacts:
        t = [im["target"] - sum(1 for g in gone if g < im["target"])]
        e.upload_pattern(*fpat[im["pattern"]])
        e.scene_apply_poses(t)
        e.place_cells(im["scale"], im["origin"])
        mask = e.scene_outside(t, im["cloud"], im["origin"], im["radius"]) if im["partial"] else None
        frags += e.scene_fracture_bodies(t, 0, frame_cells[im["pattern"]], outside=mask if mask is not None and mask.any() else None, flags=0).n_frag
        kw = dict(partial=True, sphere_points=im["cloud"], origin=im["origin"], radius=im["radius"]) if im["partial"] else {}
        co, cp, _ = e.event_regroup_bodies(**kw)
        e.event_refit(); e.event_counts()
        n = e.scene_commit(co, cp)[0]
        gone.append(im["target"])
    sync()
    return dict(frame_ms=(time.perf_counter() - t0) * 1e3, pieces=n, fragments=frags)


def one_event(e, impacts):
    t0 = time.perf_counter()
    targets = [[im["target"]] for im in impacts]
    clouds, origins, radii = [im["cloud"] for im in impacts], [im["origin"] for im in impacts], [im["radius"] for im in impacts]
    flags = [im["partial"] for im in impacts]
    e.scene_apply_poses([im["target"] for im in impacts])
    e.place_cells_patterns([im["pattern"] for im in impacts], [im["scale"] for im in impacts], origins)
    mask = e.scene_outside_impacts(targets, clouds, origins, radii)
    table = e.scene_compounds()
    at = 0
    for im in impacts:
        m = int(table[im["target"] + 1] - table[im["target"]])
        if not im["partial"]:
            mask[at:at + m] = 0
        at += m
    frags = e.scene_fracture_impacts(targets, 0, E.CELLS_ALL, outside=mask if mask.any() else None, flags=0).n_frag
    co, cp, _ = e.event_regroup_impacts_partial(flags, [c if f else None for c, f in zip(clouds, flags)], origins, radii)
    e.event_refit(); e.event_counts()
    n = e.scene_commit(co, cp)[0]
    sync()
    return dict(frame_ms=(time.perf_counter() - t0) * 1e3, pieces=n, fragments=frags)


at, rows = 0, [[], []]
for rep in range(WARM + args.reps):
    picks = [pick(e, at) for e in engs]
    assert [im["target"] for im in picks[0][0]] == [im["target"] for im in picks[1][0]] and picks[0][1] == picks[1][1], "the two routes' scenes have drifted apart"
    a = sequential(engs[0], picks[0][0])
    b = one_event(engs[1], picks[1][0])
    assert a["pieces"] == b["pieces"] and a["fragments"] == b["fragments"], (a, b)
    if rep >= WARM:
        rows[0].append(a); rows[1].append(b)
    at = picks[0][1]


def frame_summary(r):
    v = np.asarray([x["frame_ms"] for x in r], np.float64)
    return {"frame_ms": float(np.median(v)), "min": float(v.min()), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "max": float(v.max()),
            "fragments": float(np.median([x["fragments"] for x in r]))}


res["frame"] = {"scene": "configs[3]: bumpy torus x %d cells, %d pieces in %d compounds" % (args.cells, n0, nc0), "impacts": K, "pattern_cells": frame_cells,
                "sequential_with_uploads": frame_summary(rows[0]), "one_event": frame_summary(rows[1])}
if args.emul:
    res["rehearsal_on_cpu_emulation_not_a_measurement"] = True
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
for e in engs:
    e.close()
