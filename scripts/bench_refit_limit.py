"""Refit time by RefittingPointLimit on one event (torus x 4096 cells by default): the refit kernel's time (slot 2 of
surtr_kernel_times, median of five events) at limits 4, 8 and 20, beside the same step done on the host from a download --
surtr_hull_normals, surtr_kdop_planes and surtr_clip_polyhedron per fragment -- timed on a sample of fragments and scaled."""
import argparse
import json
import statistics
import sys
import time
import os

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from surtr_amd import engine, scenes


def fragment(ev, k, which):
    vo, no = ev[which + "_vert_off"], ev[which + "_nbr_off"]
    a, b = int(vo[k]), int(vo[k + 1])
    return {"pos": ev[which + "_pos"][a:b], "off": (no[a:b + 1] - no[a]).astype(np.uint32), "nbr": ev[which + "_nbr"][int(no[a]):int(no[b])]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, default=4096)
    ap.add_argument("--sample", type=int, default=48)
    a = ap.parse_args()
    sc = scenes.torus_scene(a.cells)
    eng = engine.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]]); eng.upload_pattern(sc["face_off"], sc["v012"]); eng.place_cells(sc["scale"], sc["translate"])
    eng.set_profiling(True)
    out = {"cells": a.cells}
    for limit in (4, 8, 20, 4):
        eng.set_refit_point_limit(limit)
        ms, ev_ms = [], []
        for _ in range(6):
            t0 = time.perf_counter()
            c = eng.fracture_event(0, sc["n_cells"], flags=3)
            ev_ms.append((time.perf_counter() - t0) * 1e3)
            ms.append(eng.kernel_times()["refit"])
        key = "limit%d" % limit if ("limit%d" % limit) not in out else "limit%d_again" % limit
        out[key] = {"refit_ms_median5": statistics.median(ms[1:]), "refit_ms": ms[1:], "event_ms_median5": statistics.median(ev_ms[1:]),
                    "n_frag": c.n_frag, "n_failed": c.n_failed, "status": c.status}
    c = eng.fracture_event(0, sc["n_cells"], flags=0)
    ev = eng.download()
    ks = np.random.default_rng(5).choice(c.n_frag, min(a.sample, c.n_frag), replace=False)
    for limit in (8, 20):
        t0 = time.perf_counter()
        for k in ks:
            mesh, conv = fragment(ev, int(k), "mesh"), fragment(ev, int(k), "conv")
            nrm = engine.hull_normals(mesh["pos"], min(mesh["pos"].shape[0], limit))
            planes = engine.kdop_planes(mesh["pos"], nrm)
            eng.clip_polyhedron(conv, planes)
        per = (time.perf_counter() - t0) * 1e3 / len(ks)
        out["host_limit%d" % limit] = {"ms_per_fragment": per, "ms_scaled_to_event": per * c.n_frag, "sample": int(len(ks)),
                                       "ratio_host_over_device": per * c.n_frag / out["limit%d" % limit]["refit_ms_median5"]}
    eng.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
