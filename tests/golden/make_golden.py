"""Generates the committed golden fixtures from the CPU oracle (oracle/surtr_oracle.cpp).

The reference ships no fixtures, so these vectors are the oracle's outputs -- itself pinned by tests/test_oracle_kat.py and,
function by function, by tests/test_reference_compiled.py -- on the BASELINE.json configurations:
  cube8.npz        cfg1, complete inputs (seeds, planes) and complete outputs
  digests.json     cfg2 / cfg3 / cfg4: counts + sha256 of every output array; urchin64 / urchin1024: the deep-lobed mesh of
                   meshgen.urchin (cells with several islands, non-convex faces) at the cell counts of cfg2 / cfg3
  reference_models.npz  the reference's bunny (x70) and cube (x3) as engine.read_obj loads them (tests/test_reference_pin.py);
                   written only by --models DIR, DIR being the reference's Resources/Models
  reference_compiled.npz  inputs and outputs of the reference's own geometry code, compiled by `make -C oracle ref`, on the
                   designed cases and 40 of the random clips of tests/reference_cases.py (tests/test_reference_compiled.py);
                   written only by --reference-compiled, which needs the reference tree
Run from the repo root:  python tests/golden/make_golden.py [--models DIR | --reference-compiled]
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import oracle as O          # noqa: E402
from surtr_amd import scenes            # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("frag_ids", "mesh_vert_off", "mesh_pos", "mesh_nbr_off", "mesh_nbr", "conv_vert_off", "conv_pos", "conv_nbr_off",
        "conv_nbr", "idx_off", "idx")


def digest(ev):
    d = {k: hashlib.sha256(np.ascontiguousarray(ev[k]).tobytes()).hexdigest() for k in KEYS}
    d["n_frag"] = int(ev["frag_ids"].shape[0])
    d["mesh_verts"] = int(ev["mesh_pos"].shape[0])
    d["mesh_nbrs"] = int(ev["mesh_nbr"].shape[0])
    d["conv_verts"] = int(ev["conv_pos"].shape[0])
    d["n_idx"] = int(ev["idx"].shape[0])
    d["mesh_pos_sum"] = float(ev["mesh_pos"].astype(np.float64).sum())
    d["conv_pos_sum"] = float(ev["conv_pos"].astype(np.float64).sum())
    return d


def run(sc, threads=8):
    planes = O.place_cells(sc["v012"], sc["scale"], sc["translate"])
    return planes, O.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=True, render=True, threads=threads)


def models(src):
    from surtr_amd import engine
    bunny = engine.read_obj(os.path.join(src, "lowpoly-bunny-closed.obj"), scale=(70.0,) * 3)
    cube = engine.read_obj(os.path.join(src, "cube.obj"), scale=(3.0,) * 3)
    np.savez_compressed(os.path.join(HERE, "reference_models.npz"), bunny_pos=bunny[0], bunny_tris=bunny[1], cube_pos=cube[0],
                        cube_tris=cube[1])


def reference_compiled():
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from oracle import ref_compiled as RC
    import reference_cases as C
    RC.build()
    cases = C.designed() + C.recorded_random(C.random_clips(O))
    RC.record(os.path.join(HERE, "reference_compiled.npz"), cases, RC.run(cases))
    print("reference_compiled", len(cases), os.path.getsize(os.path.join(HERE, "reference_compiled.npz")))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--models":
        return models(sys.argv[2])
    if len(sys.argv) == 2 and sys.argv[1] == "--reference-compiled":
        return reference_compiled()
    sc = scenes.cube_scene(8)
    planes, ev = run(sc)
    np.savez_compressed(os.path.join(HERE, "cube8.npz"), seeds=sc["seeds"], face_off=sc["face_off"], v012=sc["v012"], planes=planes,
                        mesh_pos=sc["mesh"]["pos"], mesh_off=sc["mesh"]["off"], mesh_nbr=sc["mesh"]["nbr"],
                        **{"out_" + k: ev[k] for k in KEYS})
    out = {}
    for name, sc in (("blob64", scenes.blob_scene(64)), ("blob1024", scenes.blob_scene(1024)), ("torus4096", scenes.torus_scene(4096)),
                     ("urchin64", scenes.urchin_scene(64)), ("urchin1024", scenes.urchin_scene(1024))):
        _, ev = run(sc)
        out[name] = digest(ev)
        print(name, out[name]["n_frag"], out[name]["mesh_verts"], out[name]["n_idx"])
    json.dump(out, open(os.path.join(HERE, "digests.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
