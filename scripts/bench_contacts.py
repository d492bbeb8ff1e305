"""surtr_scene_contacts_dev on two scenes: the broken configs[3] scene of scripts/bench_scene.py (bumpy torus x 4096 cells, every
regrouped compound a body, where the fracture left it: neighbours share their cut faces) at a margin of 1 % of the scene's extent,
and the 306-box lattice of tests/test_pick_queries.py in seven compounds at the margin tests/test_contacts.py uses.

The _dev call is bracketed by HIP events on the context's stream (device time of the whole call) and, with surtr_set_profiling, read
by phase from surtr_scene_contacts_times: bounds | body and piece pairs | distances | flag scan, header, gather.  Medians.  Beside
it the time the float64 checker of tests/contact_ref.py takes on the CPU for the same scene (boxes, Qhull, separating axes and
feature distances of every candidate pair), for scale: it is a checker, not a competitor.  Prints one JSON line; --out FILE writes
it there too.  --emul LIB rehearses the script on the CPU emulation at a small size: no HIP events, and the line says that it is no
measurement."""
import argparse, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from surtr_amd import engine as E, scenes as S

ap = argparse.ArgumentParser()
ap.add_argument("--cells", type=int, default=4096)
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--no-checker", action="store_true")
ap.add_argument("--out", default=None)
ap.add_argument("--emul", default=None)
args = ap.parse_args()

if args.emul:
    E._use_library_for_tests(args.emul)
    torch, st = None, None
else:
    import torch
    assert torch.cuda.is_available(), "no GPU: nothing can be measured here"
    st = torch.cuda.Stream()


def new_engine():
    return E.Engine(0) if st is None else E.Engine(0, stream=st.cuda_stream)


def measure(eng, margin):
    h = eng.scene_contacts_totals(margin)
    nbytes = 64 * (int(h["n_records"]) + 1)
    if torch is None:
        buf = np.zeros(nbytes, np.uint8); ptr = buf.ctypes.data
    else:
        buf = torch.zeros(nbytes, dtype=torch.uint8, device="cuda"); ptr = buf.data_ptr()
    eng.set_profiling(True)
    total, phases = [], []
    for k in range(args.reps + 3):
        if st is not None:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(st)
        eng.scene_contacts_dev(margin, ptr, nbytes)
        if st is not None:
            b.record(st); b.synchronize()
            if k >= 3:
                total.append(a.elapsed_time(b)); phases.append(eng.scene_contacts_times())
    eng.set_profiling(False)
    c0 = time.perf_counter()
    rec = eng.scene_contacts(margin)
    host_ms = (time.perf_counter() - c0) * 1e3
    out = {k: int(h[k]) for k in ("n_bodies", "n_pieces", "n_body_pairs", "n_piece_pairs", "n_records")}
    out.update(margin=float(np.float32(margin)), overlap_records=int((rec["status"] & E.CONTACT_OVERLAP != 0).sum()),
               iter_cap_records=int((rec["status"] & E.CONTACT_ITER != 0).sum()), host_form_wall_ms=host_ms)
    if total:
        ph = np.median(np.asarray(phases), 0)
        out.update(dev_call_device_ms=float(np.median(total)), bounds_ms=float(ph[0]), pair_lists_ms=float(ph[1]), distances_ms=float(ph[2]),
                   gather_ms=float(ph[3]))
    return out


def checker_ms(eng, margin):
    import contact_ref as CR
    table = eng.scene_compounds()
    c0 = time.perf_counter()
    pos = [np.asarray(eng.download_piece(p, 1)["pos"], np.float32).reshape(-1, 3) for p in range(int(table[-1]))]
    down = (time.perf_counter() - c0) * 1e3
    c0 = time.perf_counter()
    ref = CR.Reference(pos, table, margin)
    return {"download_ms": down, "checker_ms": (time.perf_counter() - c0) * 1e3, "checker_piece_pairs": len(ref.piece_pairs)}


res = {"reps": args.reps}
# ---- the broken configs[3] scene
eng = new_engine()
sc = S.torus_scene(args.cells, eng=eng)
eng.upload_pieces([sc["mesh"]], [sc["convex"]])
eng.upload_pattern(sc["face_off"], sc["v012"])
eng.place_cells(sc["scale"], sc["translate"])
eng.scene_fracture_event(0, 0, sc["n_cells"], flags=0)
co, cp = eng.event_regroup()
eng.event_refit()
eng.scene_commit(co, cp)
b = eng.scene_bounds(set=1)
L = float((b["hi"].max(0) - b["lo"].min(0)).max())
margin = float(np.float32(0.01 * L))
res["broken_configs3"] = dict(measure(eng, margin), scene="bumpy torus x %d cells, every regrouped compound a body" % args.cells, extent=L)
if not args.no_checker:
    res["broken_configs3"].update(checker_ms(eng, margin))
eng.close()

# ---- the 306-box lattice (test_pick_queries.scene_d) in compounds of 1, 2, 61, 64, 65, 70 and 43 pieces, as it lies
import test_pick_queries as PQ
eng, n = PQ.scene_d(E)
if st is not None:
    eng.set_stream(st.cuda_stream)
eng.scene_set_compounds(np.cumsum([0, 1, 2, 61, 64, 65, 70, 43]))
res["lattice_306"] = measure(eng, 1.08)
if not args.no_checker:
    res["lattice_306"].update(checker_ms(eng, 1.08))
eng.close()
if args.emul:
    res["rehearsal_on_cpu_emulation_not_a_measurement"] = True
line = json.dumps(res)
print(line)
if args.out:
    with open(args.out, "w") as f:
        f.write(line + "\n")
