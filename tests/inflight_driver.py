#!/usr/bin/env python3
"""Parity of every event of the several-contexts-in-flight arrangement that bench.py measures (a script, not a test module).

bench.py (`setup()` / `step()`, bench.py:223-311) builds E engines, each on a torch stream of its own (`set_stream`), tells each
`set_events_in_flight(E)` and launches steps round-robin -- place_cells, fracture_event_async, pack_dev -- with no host sync in
between.  This driver builds the same scene and the same arrangement, runs R rounds x E contexts of one case, unpacks EVERY blob
and compares it, array by array and bit for bit, with the event of one context run alone (which is checked once against the
oracle).  tests/test_inflight_parity.py runs it in a child process per configuration (GPU_MAX_HW_QUEUES is read when HIP
starts; a hang or fault stays inside a child with a time limit); the CPU tier calls run() in-process on the emulation.

    python tests/inflight_driver.py --case whole --rounds 30 --in-flight 6 --json OUT

Cases:
    whole       every context: the whole event (BASELINE configs[3], 4 096 cells)
    blocks8     context k, round r: the 512-cell block (k + r) % 8 -- cell_begin changes per context and round
    mixed       context 0: 512-cell block, whole, 2 048-cell block, 512, whole, ... (starts small: the growth paths); the others whole
    refracture  BASELINE configs[4]: 256 first-level fragments x 32 cells each through fracture_pairs

Pass A launches everything and synchronises once at the end, every event packing into a blob buffer of its own.  Pass B runs
the same rounds with a synchronisation after each, and reads per event the record clipper's counters (surtr_queue_stats [89]
pairs handed on, [94] pairs the catcher clipped) and the hand-over words (surtr_handover_stats).  The report names every event
that differs; the exit status is non-zero on any mismatch or error.
"""
import argparse
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _d in (ROOT, HERE):
    if _d not in sys.path:
        sys.path.insert(0, _d)

import numpy as np  # noqa: E402

CASES = ("whole", "blocks8", "mixed", "refracture")
FLAGS = 3      # EVT_REFIT | EVT_RENDER, as bench.py's steps


class _Device:
    """Streams, blob buffers and synchronisation: torch on the GPU (as bench.py), plain host memory on the emulation."""

    def __init__(self, emul):
        self.emul = emul
        if not emul:
            import torch
            self.torch = torch
            if not torch.cuda.is_available():
                raise SystemExit("inflight_driver: no HIP device (the engine has no CPU fallback)")
            torch.cuda.set_device(0)

    def stream(self):
        return None if self.emul else self.torch.cuda.Stream()

    def buffer(self, nbytes):
        if self.emul:
            return np.zeros(nbytes, np.uint8)
        return self.torch.empty(nbytes, dtype=self.torch.uint8, device="cuda")

    @staticmethod
    def ptr(buf):
        return buf.ctypes.data if isinstance(buf, np.ndarray) else buf.data_ptr()

    @staticmethod
    def host(buf):
        return buf if isinstance(buf, np.ndarray) else buf.cpu().numpy()

    def sync(self):
        if not self.emul:
            self.torch.cuda.synchronize()


def shapes(case, n_cells, rounds, E):
    """[r][k] -> (cell_begin, cell_end) of the event context k runs in round r (None for refracture: its pair list)."""
    C, b8 = n_cells, n_cells // 8
    out = []
    for r in range(rounds):
        row = []
        for k in range(E):
            if case == "whole":
                row.append((0, C))
            elif case == "blocks8":
                b = (k + r) % 8
                row.append((b * b8, (b + 1) * b8))
            elif case == "mixed":
                row.append([(b8, 2 * b8), (0, C), (C // 2, C)][r % 3] if k == 0 else (0, C))
            else:
                row.append(None)
        out.append(row)
    return out


def _bench_scene(engine, scenes, meshgen, eng, torus, n_cells):
    """bench.py:215-252 on one engine: the piece (rings on the device), the Voronoi pattern built on the device, the ACH convex."""
    verts, tris = meshgen.bumpy_torus(*torus) if torus else meshgen.bumpy_torus()
    sc = scenes.mesh_scene(verts, tris, eng=eng)
    sc["n_cells"] = n_cells
    seeds = scenes.uniform_seeds(n_cells, scenes.SEED)
    eng.build_cells(seeds)
    cells = eng.download_cells()
    sc["seeds"], sc["face_off"], sc["v012"] = seeds, cells["cell_face_off"], cells["v012"]
    sc["convex"], _ = scenes.ach_convex(eng, sc["mesh"]["pos"])
    return sc


def _install(eng, sc):
    """What bench.py's setup() does on every engine (bench.py:248-252)."""
    eng.build_cells(sc["seeds"])
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])       # (second call: steady state of the piece pool)


def _refracture_scene(engine, scenes, meshgen, eng, torus, n_first, n_second):
    """The first level of configs[4] on `eng` and the second level's inputs, as tests/test_refracture.py::_refracture builds them."""
    from test_refracture import _links_symmetric
    sc = scenes.make_scene(*meshgen.bumpy_torus(*torus), n_first)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, n_first, flags=1)
    first = eng.download()
    meshes, convexes = scenes.fragments_as_pieces(first)
    keep = [i for i, m in enumerate(meshes) if m["pos"].shape[0] >= 4 and np.diff(m["off"].astype(np.int64)).min() >= 3 and convexes[i]["pos"].shape[0] >= 4
            and _links_symmetric(m) and _links_symmetric(convexes[i])]
    meshes, convexes = [meshes[i] for i in keep], [convexes[i] for i in keep]
    rs = scenes.refracture_scene(meshes, convexes, n_second)
    rs["pair_cell"] = np.ascontiguousarray(rs["pair_cell"], np.uint32)
    rs["pair_piece"] = np.ascontiguousarray(rs["pair_piece"], np.uint32)
    return {"meshes": meshes, "convexes": convexes, "rs": rs}


def _install_refracture(eng, rf):
    eng.upload_pieces(rf["meshes"], rf["convexes"])
    eng.upload_pattern(rf["rs"]["face_off"], rf["rs"]["v012"])


def _oracle_refracture(engine, oracle, rf, threads):
    """tests/test_refracture.py::_refracture's reference: piece by piece with its own cells, fragment-major."""
    rs, parts = rf["rs"], []
    for p in range(len(rf["meshes"])):
        a, b = int(rs["group_cell_off"][p]), int(rs["group_cell_off"][p + 1])
        f0, f1 = int(rs["face_off"][a]), int(rs["face_off"][b])
        planes = oracle.place_cells(rs["v012"][f0:f1], rs["scales"][p], rs["shifts"][p])
        ev = oracle.event([rf["meshes"][p]], [rf["convexes"][p]], rs["face_off"][a:b + 1] - rs["face_off"][a], planes, threads=threads)
        ev["frag_ids"] = ev["frag_ids"] + np.array([a, p, 0], np.int32)
        parts.append(ev)
    return engine.merge_fragments(parts)


def _first_diff(got, ref):
    """Keys that differ, and the first fragment whose ids, solids or triangles differ (its frag_ids row on either side)."""
    from helpers import fragment
    keys = sorted(k for k in ref if not (got[k].shape == ref[k].shape and np.array_equal(got[k], ref[k])))
    if not keys:
        return keys, None
    ga, ra = got["frag_ids"], ref["frag_ids"]
    for k in range(max(ga.shape[0], ra.shape[0])):
        same = k < ga.shape[0] and k < ra.shape[0] and np.array_equal(ga[k], ra[k])
        for which in ("mesh", "conv"):
            if same:
                a, b = fragment(got, k, which), fragment(ref, k, which)
                same = all(a[n].shape == b[n].shape and np.array_equal(a[n], b[n]) for n in ("pos", "off", "nbr"))
        if same:
            i0, i1, j0, j1 = (int(got["idx_off"][k]), int(got["idx_off"][k + 1]), int(ref["idx_off"][k]), int(ref["idx_off"][k + 1]))
            same = np.array_equal(got["idx"][i0:i1], ref["idx"][j0:j1])
        if not same:
            return keys, {"index": k, "got": ga[k].tolist() if k < ga.shape[0] else None, "ref": ra[k].tolist() if k < ra.shape[0] else None}
    return keys, {"index": None, "got": None, "ref": None}


def run(case, rounds, E, emul_lib=None, torus=None, n_cells=4096, refr=(256, 32, (250, 200)), check_oracle=True, threads=16, log=None):
    """Runs one case; returns the report (a dict).  emul_lib: path of an emulation build (CPU tier), None: libsurtr_hip.so."""
    from surtr_amd import engine, meshgen, scenes
    from oracle import oracle
    from helpers import assert_event_equal, assert_event_equal_flagged
    assert case in CASES, case
    t_start = time.perf_counter()
    say = log or (lambda *a: None)
    dev = _Device(emul_lib is not None)
    if emul_lib is not None:
        engine._use_library_for_tests(emul_lib)
    report = {"case": case, "rounds": rounds, "in_flight": E, "emulation": emul_lib is not None,
              "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "surtr_catch_poll": os.environ.get("SURTR_CATCH_POLL"),
              "events_checked": 0, "events_ok": 0, "bad": [], "error": None}
    try:
        _run(case, rounds, E, dev, engine, meshgen, scenes, oracle, assert_event_equal, assert_event_equal_flagged, torus, n_cells, refr,
             check_oracle, threads, report, say)
    finally:
        if emul_lib is not None:
            engine._use_library_for_tests(None)
    report["wall_s"] = round(time.perf_counter() - t_start, 2)
    report["ok"] = report["error"] is None and not report["bad"] and report["events_checked"] == rounds * E \
        and report.get("pass_b", {}).get("events_checked") == rounds * E
    return report


def _run(case, rounds, E, dev, engine, meshgen, scenes, oracle, assert_event_equal, assert_event_equal_flagged, torus, n_cells, refr,
         check_oracle, threads, report, say):
    # ---- the references: one context alone (hint 1) on every event shape of the case, each checked once against the oracle
    plan = shapes(case, n_cells, rounds, E)
    ref_eng = engine.Engine(0)
    refs, caps = {}, {}
    try:
        if case == "refracture":
            rf = _refracture_scene(engine, scenes, meshgen, ref_eng, refr[2], refr[0], refr[1])
            rs = rf["rs"]
            n_pairs = int(rs["pair_cell"].shape[0])
            _install_refracture(ref_eng, rf)
            ref_eng.place_cells_groups(rs["group_cell_off"], rs["scales"], rs["shifts"])
            ref_eng.fracture_pairs_async(rs["pair_cell"], rs["pair_piece"], flags=FLAGS)
            todo = [None]
        else:
            sc = _bench_scene(engine, scenes, meshgen, ref_eng, torus, n_cells)
            ref_eng.upload_pieces([sc["mesh"]], [sc["convex"]])
            ref_eng.upload_pieces([sc["mesh"]], [sc["convex"]])
            todo = sorted({s for row in plan for s in row})
        for i, shape in enumerate(todo):
            if shape is not None:
                ref_eng.place_cells(sc["scale"], sc["translate"])
                ref_eng.fracture_event_async(shape[0], shape[1], flags=FLAGS)
            c = ref_eng.event_counts()
            if c.status != 0:
                raise RuntimeError("reference event %s: device status %d" % (shape, c.status))
            cap = (engine.blob_bytes(c) + 4095) // 4096 * 4096
            buf = dev.buffer(cap)
            ref_eng.pack_dev(dev.ptr(buf), cap)
            dev.sync()
            rc, ref = engine.unpack_blob(dev.host(buf))
            if rc.status != 0 or (rc.n_failed != 0 and case != "refracture"):
                raise RuntimeError("reference event %s: status %d, %d failed pairs" % (shape, rc.status, rc.n_failed))
            if check_oracle:
                t0 = time.perf_counter()
                if case == "refracture":
                    ps = ref_eng.pair_status(n_pairs)
                    ref["flagged_pairs"] = [(int(rs["pair_cell"][j]), int(rs["pair_piece"][j])) for j in np.nonzero(ps)[0]]
                    assert_event_equal_flagged(ref, _oracle_refracture(engine, oracle, rf, threads))
                    del ref["flagged_pairs"]
                else:
                    planes = oracle.place_cells(sc["v012"], sc["scale"], sc["translate"])
                    orc = oracle.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=True, render=True, threads=threads,
                                       cell_begin=shape[0], cell_end=shape[1])
                    assert_event_equal(ref, orc)
                say("reference %s: %d fragments, oracle agrees (%.1f s)" % (shape, rc.n_frag, time.perf_counter() - t0))
            refs[shape], caps[shape] = ref, cap
    finally:
        ref_eng.close()
    report["references"] = {str(k): int(v["frag_ids"].shape[0]) for k, v in refs.items()}

    # ---- the arrangement: E contexts, a stream each, the hint at E (bench.py:229-235)
    engs, streams = [], []
    try:
        for k in range(E):
            st = dev.stream()
            e = engine.Engine(0)
            if st is not None:
                e.set_stream(st.cuda_stream)
            e.set_events_in_flight(E)
            engs.append(e); streams.append(st)
            if case == "refracture":
                _install_refracture(e, rf)
            else:
                _install(e, sc)
        dev.sync()

        def launch(e, shape, buf):
            if shape is None:
                e.place_cells_groups(rs["group_cell_off"], rs["scales"], rs["shifts"])
                e.fracture_pairs_async(rs["pair_cell"], rs["pair_piece"], flags=FLAGS)
            else:
                e.place_cells(sc["scale"], sc["translate"])
                e.fracture_event_async(shape[0], shape[1], flags=FLAGS)
            e.pack_dev(dev.ptr(buf), caps[shape])

        ok = {"A": 0, "B": 0}

        def check(which, r, k, buf):
            """Unpacks one blob and compares it with its reference; returns False when the device reported an error."""
            shape = plan[r][k]
            c, got = engine.unpack_blob(dev.host(buf))
            ref = refs[shape]
            keys, row = _first_diff(got, ref)
            if c.status != 0 or (c.n_failed != 0 and case != "refracture") or keys:
                report["bad"].append({"pass": which, "round": r, "slot": r * E + k, "context": k, "shape": list(shape) if shape else None,
                                      "status": int(c.status), "n_failed": int(c.n_failed), "keys": keys, "first_frag": row})
            else:
                ok[which] += 1
            return c.status == 0

        # pass A: bench-faithful, every event into a blob of its own, one sync at the end
        t0 = time.perf_counter()
        bufs = [[dev.buffer(caps[plan[r][k]]) for k in range(E)] for r in range(rounds)]
        launched = 0
        try:
            for r in range(rounds):
                for k in range(E):
                    launch(engs[k], plan[r][k], bufs[r][k])
                    launched += 1
        except engine.SurtrError as err:
            report["error"] = "pass A, launch %d: %s" % (launched, err)
        dev.sync()
        report["pass_a"] = {"launch_s": round(time.perf_counter() - t0, 3), "launched": launched}
        device_ok = True
        for i in range(launched):
            r, k = divmod(i, E)
            device_ok = check("A", r, k, bufs[r][k]) and device_ok
            report["events_checked"] += 1
        report["events_ok"] = ok["A"]
        del bufs
        say("pass A: %d / %d events equal their reference" % (report["events_ok"], report["events_checked"]))
        if report["error"] is not None or not device_ok:
            report["error"] = report["error"] or "pass A: a device status was not 0; pass B not run"
            return

        # pass B: the same rounds with a sync after each, and the counters of every event
        per_event, tot = [], {"pushed": 0, "q89": 0, "q94": 0, "poll_claimed": 0, "sweep_cursor": 0}
        bufs = [dev.buffer(max(caps.values())) for _ in range(E)]
        checked_b = 0
        for r in range(rounds):
            try:
                for k in range(E):
                    launch(engs[k], plan[r][k], bufs[k])
            except engine.SurtrError as err:
                report["error"] = "pass B, round %d: %s" % (r, err)
                dev.sync()
                break
            dev.sync()
            device_ok = True
            for k in range(E):
                qs, hs = engs[k].queue_stats(), engs[k].handover_stats()
                shape = plan[r][k]
                n_pairs_k = n_pairs if shape is None else shape[1] - shape[0]
                ev = {"round": r, "context": k, "pushed": hs["pushed"], "main_started": hs["main_started"],
                      "main_signed_off": hs["main_signed_off"], "main_grid": max(1, min(n_pairs_k, hs["max_wg"])),
                      "poll_claimed": hs["poll_claimed"], "sweep_cursor": hs["sweep_cursor"], "q89": int(qs[89]), "q94": int(qs[94])}
                per_event.append(ev)
                for key in tot:
                    tot[key] += ev[key]
                device_ok = check("B", r, k, bufs[k]) and device_ok
                checked_b += 1
                if shape is not None:
                    # the order k_clip_convex took the pairs in must be this event's (most planes first), not a cached one of
                    # another block of the same size: a stale order gives the same fragments, only in a worse schedule
                    po = np.asarray(sc["face_off"], np.int64)
                    want = np.argsort(-(po[shape[0] + 1:shape[1] + 1] - po[shape[0]:shape[1]]), kind="stable").astype(np.uint32)
                    got_order = engs[k].pair_order()
                    if not np.array_equal(got_order, want):
                        report["bad"].append({"pass": "B", "round": r, "slot": r * E + k, "context": k, "shape": list(shape),
                                              "keys": ["pair_order"], "first_frag": None})
            if not device_ok:
                report["error"] = "pass B, round %d: a device status was not 0" % r
                break
        report["pass_b"] = {"events_checked": checked_b, "events_ok": ok["B"], "counters": tot}
        report["per_event"] = per_event
        say("pass B: %d / %d events equal their reference; %s" % (report["pass_b"]["events_ok"], checked_b, tot))
    finally:
        for e in engs:
            e.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--case", choices=CASES, required=True)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--in-flight", type=int, default=6)
    ap.add_argument("--json", required=True, metavar="OUT")
    ap.add_argument("--no-oracle", action="store_true", help="skip the one check of each reference against the oracle")
    args = ap.parse_args()
    report = run(args.case, args.rounds, args.in_flight, check_oracle=not args.no_oracle,
                 log=lambda m: print("inflight_driver: " + m, file=sys.stderr, flush=True))
    with open(args.json, "w") as f:
        json.dump(report, f, indent=1)
    print(json.dumps({k: report[k] for k in ("case", "events_checked", "events_ok", "ok", "error", "wall_s")}), flush=True)
    sys.exit(0 if report["ok"] else 1)


if __name__ == "__main__":
    main()
