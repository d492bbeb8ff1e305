"""K impacts of one frame on K disjoint bodies of a resident scene, two ways, alternately in one process: (a) the loop there was -- per
impact, in the order given: scene_apply_poses, place_cells, scene_outside, scene_fracture_bodies, event_regroup_bodies, event_refit,
scene_commit; (b) the one-event route -- scene_apply_poses over all targets, place_cells_impacts, scene_outside_impacts,
scene_fracture_impacts, event_regroup_impacts, event_refit, one scene_commit.

The scene is that of scripts/bench_scene_bodies.py: BASELINE configs[3] (bumpy torus x 4096 cells) broken into its regrouped
compounds.  Two engines hold it, one per route; both are given the same seeded frames with the 64-cell pattern, so they stay the same
scene (tests/test_scene_impacts.py: the two routes leave the same bits).  A frame casts seeded rays until K different bodies are hit;
each hit is an impact with its own point and its own radius on the body it hit, which is given a small pose, as a solver would have:
picking and posing are not timed.  Timed, per route: everything from the pose bake to the end of the last commit, with HIP events on
the context's stream and with the host clock; every step is a synchronous call, so the host clock around a step is its call time.
Per K in --impacts: WARM frames, then --reps timed ones; per figure the median, and for the frame time the 10th and 90th percentile
and the extremes as well.  With --kernels the one-event route of the largest K is run --reps more times under surtr_set_profiling
(a run of its own: the event records slow the host) and the per-kernel medians of surtr_kernel_times are added.
Prints one JSON line; --out FILE appends it there (profiles/scene_impacts_bench.json holds one line per process).  --emul LIB
rehearses the script on the CPU emulation at a small size: no HIP events, and the line says that it is no measurement."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from surtr_amd import engine as E, scenes as S

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=4096)
ap.add_argument("--click-cells", type=int, default=64)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--impacts", default="1,2,4,8")
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--emul", default=None)
args = ap.parse_args()
WARM = 3
KS = [int(x) for x in args.impacts.split(",")]

if args.emul:
    E._use_library_for_tests(args.emul)
    torch = None
    streams = [None, None]
    engs = [E.Engine(0), E.Engine(0)]
else:
    import torch
    assert torch.cuda.is_available(), "no GPU: nothing can be measured here"
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    engs = [E.Engine(0, stream=s.cuda_stream) for s in streams]

sc = S.torus_scene(args.cells, eng=engs[0])
click_pattern = E.pattern_from_cells(E.voronoi_cells(S.uniform_seeds(args.click_cells)))
for eng in engs:      # the scene: configs[3], every regrouped compound a body
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
R = np.float32(0.04 * L)                      # impact radius: a few fragments across; impact i of a frame takes R * (0.8 + 0.1 * (i % 4))
rng = np.random.default_rng(20261020)
frames = (len(KS) + 1) * (WARM + args.reps)
aims = np.asarray(sc["mesh"]["pos"], np.float64)[rng.choice(sc["mesh"]["pos"].shape[0], 4 * max(KS) * frames + 64)]
centre = np.asarray(sc["translate"], np.float64)
NUDGE = np.eye(4, dtype=np.float32)
NUDGE[:3, 3] = np.float32(1e-4 * L)           # the pose a solver left on a body that is about to be hit
at = 0


def pick(eng, first, K):
    """Untimed: rays from `first` on until K different bodies are hit; their poses.  -> (impacts, the next unused aim)."""
    impacts, seen, k = [], set(), first
    while len(impacts) < K:
        d = aims[k] - centre
        d /= np.linalg.norm(d)
        ray = np.r_[aims[k] + d * L, -d, 4 * L].astype(np.float32)
        hit = eng.scene_raycast(ray.reshape(1, 7))[0]
        k += 1
        if hit["piece"] < 0 or int(hit["compound"]) in seen:
            continue
        seen.add(int(hit["compound"]))
        r = np.float32(R * np.float32(0.8 + 0.1 * (len(impacts) % 4)))
        pos = (hit["pos"] + ray[3:6] * np.float32(0.01)).astype(np.float32)
        impacts.append(dict(target=int(hit["compound"]), origin=pos, radius=float(r), scale=np.float32([r * np.float32(2)] * 3), cloud=(lat * r + pos).astype(np.float32)))
    poses = eng.scene_poses()
    poses[[im["target"] for im in impacts]] = NUDGE
    eng.scene_set_poses(poses)
    return impacts, k


class Clock:
    """Host milliseconds per named step, added up over a frame; HIP events around the whole."""

    def __init__(self, stream):
        self.t, self.stream, self.last = {}, stream, None
        if stream is not None:
            self.ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            self.ev[0].record(stream)
        self.c0 = self.last = time.perf_counter()

    def step(self, name):
        now = time.perf_counter()
        self.t[name + "_ms"] = self.t.get(name + "_ms", 0.0) + (now - self.last) * 1e3
        self.last = now

    def done(self):
        self.t["frame_ms"] = (time.perf_counter() - self.c0) * 1e3
        if self.stream is not None:
            self.ev[1].record(self.stream)
            self.ev[1].synchronize()
            self.t["frame_device_ms"] = self.ev[0].elapsed_time(self.ev[1])
        return self.t


def loop(eng, stream, impacts):
    c = Clock(stream)
    frags, gone = 0, []
    for im in impacts:
        t = [im["target"] - sum(1 for g in gone if g < im["target"])]      # (the commits before it moved it down)
        eng.scene_apply_poses(t); c.step("apply_pose")
        eng.place_cells(im["scale"], im["origin"]); c.step("place")
        mask = eng.scene_outside(t, im["cloud"], im["origin"], im["radius"]); c.step("mask")
        frags += eng.scene_fracture_bodies(t, 0, args.click_cells, outside=mask if mask.any() else None, flags=0).n_frag; c.step("event")
        co, cp, _ = eng.event_regroup_bodies(partial=True, sphere_points=im["cloud"], origin=im["origin"], radius=im["radius"]); c.step("regroup")
        eng.event_refit(); eng.event_counts(); c.step("refit")
        n = eng.scene_commit(co, cp)[0]; c.step("commit")
        gone.append(im["target"])
    return dict(c.done(), pieces=n, fragments=frags)


def one_event(eng, stream, impacts):
    c = Clock(stream)
    targets = [[im["target"]] for im in impacts]
    clouds, origins, radii = [im["cloud"] for im in impacts], [im["origin"] for im in impacts], [im["radius"] for im in impacts]
    eng.scene_apply_poses([im["target"] for im in impacts]); c.step("apply_pose")
    eng.place_cells_impacts([im["scale"] for im in impacts], origins); c.step("place")
    mask = eng.scene_outside_impacts(targets, clouds, origins, radii); c.step("mask")
    frags = eng.scene_fracture_impacts(targets, 0, args.click_cells, outside=mask if mask.any() else None, flags=0).n_frag; c.step("event")
    co, cp, _ = eng.event_regroup_impacts(partial=True, sphere_points=clouds, origins=origins, radii=radii); c.step("regroup")
    eng.event_refit(); eng.event_counts(); c.step("refit")
    n = eng.scene_commit(co, cp)[0]; c.step("commit")
    return dict(c.done(), pieces=n, fragments=frags)


def summary(rows):
    out = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    for k in ("frame_ms", "frame_device_ms"):
        if k in rows[0]:
            v = np.asarray([r[k] for r in rows], np.float64)
            out[k[:-3] + "_spread_ms"] = {"min": float(v.min()), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "max": float(v.max())}
    return out


res = {"scene": "configs[3]: bumpy torus x %d cells, %d pieces in %d compounds; frames of K impacts with a %d-cell pattern, each on one posed body" % (args.cells, n0, nc0, args.click_cells),
       "reps": args.reps, "warm": WARM, "by_impacts": {}}
for K in KS:
    rows = [[], []]
    for rep in range(WARM + args.reps):
        picks = [pick(eng, at, K) for eng in engs]
        assert [im["target"] for im in picks[0][0]] == [im["target"] for im in picks[1][0]] and picks[0][1] == picks[1][1], "the two routes' scenes have drifted apart"
        a = loop(engs[0], streams[0], picks[0][0])
        b = one_event(engs[1], streams[1], picks[1][0])
        assert a["pieces"] == b["pieces"] and a["fragments"] == b["fragments"], (a, b)
        if rep >= WARM:
            rows[0].append(a); rows[1].append(b)
        at = picks[0][1]
    res["by_impacts"][str(K)] = {"loop": summary(rows[0]), "one_event": summary(rows[1])}

if args.kernels:      # a run of its own: per-kernel times of the one-event route at the largest K (the loop's engine follows, untimed, to stay the same scene)
    K = max(KS)
    engs[1].set_profiling(True)
    names = None
    rows = []
    for rep in range(args.reps):
        picks = [pick(eng, at, K) for eng in engs]
        loop(engs[0], streams[0], picks[0][0])
        eng = engs[1]
        impacts = picks[1][0]
        targets = [[im["target"]] for im in impacts]
        clouds, origins, radii = [im["cloud"] for im in impacts], [im["origin"] for im in impacts], [im["radius"] for im in impacts]
        eng.scene_apply_poses([im["target"] for im in impacts])
        eng.place_cells_impacts([im["scale"] for im in impacts], origins)
        mask = eng.scene_outside_impacts(targets, clouds, origins, radii)
        eng.scene_fracture_impacts(targets, 0, args.click_cells, outside=mask if mask.any() else None, flags=0)
        co, cp, _ = eng.event_regroup_impacts(partial=True, sphere_points=clouds, origins=origins, radii=radii)
        eng.event_refit(); eng.event_counts()
        kt = eng.kernel_times()
        rows.append([float(x) for x in (kt.values() if isinstance(kt, dict) else kt)])
        names = list(kt.keys()) if isinstance(kt, dict) else None
        eng.scene_commit(co, cp)
        at = picks[0][1]
    med = [float(np.median([r[i] for r in rows])) for i in range(len(rows[0]))]
    res["one_event_kernel_times_ms"] = {"impacts": K, "slots": dict(zip(names, med)) if names else med}
    engs[1].set_profiling(False)
if args.emul:
    res["rehearsal_on_cpu_emulation_not_a_measurement"] = True
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
for eng in engs:
    eng.close()
