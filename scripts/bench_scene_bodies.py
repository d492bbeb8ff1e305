"""One radial click on K bodies of a resident scene, two ways, in one process: (a) the route there was -- per body hit, in descending
compound number: scene_apply_pose, the out-of-sphere mask from download_piece + the host loop, place_cells, scene_fracture_event,
event_regroup, event_refit, scene_commit; (b) the one-event route -- scene_apply_poses, place_cells, scene_outside,
scene_fracture_bodies, event_regroup_bodies, event_refit, one scene_commit.

The scene is that of scripts/bench_scene.py: BASELINE configs[3] (bumpy torus x 4096 cells) broken into its regrouped compounds.
Two engines hold it, one per route; both are given the same seeded clicks with the 64-cell pattern, so they stay the same scene
(tests/test_scene_bodies.py: the two routes leave the same bits).  A click picks with a ray, takes the K compounds whose centres of
mass are nearest to the impact (the one hit among them) and gives each a small pose, as a solver would have: picking and posing are
not timed.  Timed, per route: everything from the pose bake to the end of the commit, with HIP events on the context's stream and
with the host clock; every step is a synchronous call, so the host clock around a step is its call time.  Per K in --bodies:
WARM clicks, then --reps timed ones; medians.  Also the mask alone for one body: scene_outside against download_piece + host loop.
Prints one JSON line; --out FILE appends it there (profiles/scene_bodies_bench.json holds one line per process).  --emul LIB
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
ap.add_argument("--bodies", default="1,2,4,8")
ap.add_argument("--out", default=None)
ap.add_argument("--emul", default=None)
args = ap.parse_args()
WARM = 3
KS = [int(x) for x in args.bodies.split(",")]

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
R = np.float32(0.04 * L)                      # impact radius: a few fragments across
rng = np.random.default_rng(20261019)
aims = np.asarray(sc["mesh"]["pos"], np.float64)[rng.choice(sc["mesh"]["pos"].shape[0], len(KS) * (WARM + args.reps) + 8)]
centre = np.asarray(sc["translate"], np.float64)
NUDGE = np.eye(4, dtype=np.float32)
NUDGE[:3, 3] = np.float32(1e-4 * L)           # the pose a solver left on a body that is about to be hit


def pick(eng, k, K):
    """Untimed: the ray, the impact, the K bodies, their poses.  -> (targets descending, impact, cloud)."""
    d = aims[k] - centre
    d /= np.linalg.norm(d)
    ray = np.r_[aims[k] + d * L, -d, 4 * L].astype(np.float32)
    hit = eng.scene_raycast(ray.reshape(1, 7))[0]
    assert hit["piece"] >= 0
    impact = (hit["pos"] + ray[3:6] * np.float32(0.01)).astype(np.float32)
    com = eng.scene_mass(set=1)["com"]
    order = np.argsort(((com - impact.astype(np.float64)) ** 2).sum(1), kind="stable")
    targets = [int(hit["compound"])] + [int(c) for c in order if int(c) != int(hit["compound"])][:K - 1]
    poses = eng.scene_poses()
    poses[targets] = NUDGE
    eng.scene_set_poses(poses)
    return sorted(targets, reverse=True), impact, (lat * R + impact).astype(np.float32)


class Clock:
    """Host milliseconds per named step, added up over a click; HIP events around the whole."""

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
        self.t["click_ms"] = (time.perf_counter() - self.c0) * 1e3
        if self.stream is not None:
            self.ev[1].record(self.stream)
            self.ev[1].synchronize()
            self.t["click_device_ms"] = self.ev[0].elapsed_time(self.ev[1])
        return self.t


def host_mask(eng, comp, cloud, impact):
    table = eng.scene_compounds()
    return np.asarray([E.convex_out_of_sphere(eng.download_piece(p, 1), cloud, impact, float(R)) for p in range(int(table[comp]), int(table[comp + 1]))], np.uint8)


def sequential(eng, stream, targets, impact, cloud):
    c = Clock(stream)
    frags = 0
    for t in targets:
        eng.scene_apply_pose(t); c.step("apply_pose")
        mask = host_mask(eng, t, cloud, impact); c.step("mask")
        eng.place_cells([R * np.float32(2)] * 3, impact); c.step("place")
        frags += eng.scene_fracture_event(t, 0, args.click_cells, outside=mask if mask.any() else None, flags=0).n_frag; c.step("event")
        co, cp = eng.event_regroup(partial=True, sphere_points=cloud, origin=impact, radius=float(R)); c.step("regroup")
        eng.event_refit(); eng.event_counts(); c.step("refit")
        n = eng.scene_commit(co, cp)[0]; c.step("commit")
    return dict(c.done(), pieces=n, fragments=frags)


def one_event(eng, stream, targets, impact, cloud):
    c = Clock(stream)
    eng.scene_apply_poses(targets); c.step("apply_pose")
    eng.place_cells([R * np.float32(2)] * 3, impact); c.step("place")
    mask = eng.scene_outside(targets, cloud, impact, float(R)); c.step("mask")
    frags = eng.scene_fracture_bodies(targets, 0, args.click_cells, outside=mask if mask.any() else None, flags=0).n_frag; c.step("event")
    co, cp, _ = eng.event_regroup_bodies(partial=True, sphere_points=cloud, origin=impact, radius=float(R)); c.step("regroup")
    eng.event_refit(); eng.event_counts(); c.step("refit")
    n = eng.scene_commit(co, cp)[0]; c.step("commit")
    return dict(c.done(), pieces=n, fragments=frags)


def median_of(rows):
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


res = {"scene": "configs[3]: bumpy torus x %d cells, %d pieces in %d compounds; radial clicks with a %d-cell pattern on K posed bodies" % (args.cells, n0, nc0, args.click_cells),
       "reps": args.reps, "warm": WARM, "by_bodies": {}}
at = 0
for K in KS:
    rows = [[], []]
    for rep in range(WARM + args.reps):
        picks = [pick(eng, at, K) for eng in engs]
        assert picks[0][0] == picks[1][0], "the two routes' scenes have drifted apart"
        a = sequential(engs[0], streams[0], *picks[0])
        b = one_event(engs[1], streams[1], *picks[1])
        assert a["pieces"] == b["pieces"] and a["fragments"] == b["fragments"], (a, b)
        if rep >= WARM:
            rows[0].append(a); rows[1].append(b)
        at += 1
    res["by_bodies"][str(K)] = {"sequential": median_of(rows[0]), "one_event": median_of(rows[1])}

# the mask alone, for one body of several pieces: the largest compound of the scene as it now stands
table = engs[1].scene_compounds()
big = int(np.argmax(np.diff(table.astype(np.int64))))
cen = engs[1].scene_mass(set=1)["com"][big].astype(np.float32)
cloud = (lat * R + cen).astype(np.float32)
dev, host = [], []
for rep in range(WARM + args.reps):
    c0 = time.perf_counter()
    m1 = engs[1].scene_outside([big], cloud, cen, float(R))
    c1 = time.perf_counter()
    m0 = host_mask(engs[1], big, cloud, cen)
    c2 = time.perf_counter()
    assert m0.tobytes() == m1.tobytes()
    if rep >= WARM:
        dev.append((c1 - c0) * 1e3); host.append((c2 - c1) * 1e3)
res["mask_one_body"] = {"pieces": int(table[big + 1] - table[big]), "scene_outside_ms": float(np.median(dev)), "download_and_host_loop_ms": float(np.median(host))}
if args.emul:
    res["rehearsal_on_cpu_emulation_not_a_measurement"] = True
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "a") as f:
        f.write(line + "\n")
for eng in engs:
    eng.close()
