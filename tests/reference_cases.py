"""The cases of tests/test_reference_compiled.py: inputs on which a restatement of the reference's geometry goes wrong.

Only inputs are built here (numpy, the designed solids of faces_ref / regroup_ref, the committed fixtures, fragments of two small
scenes); oracle/ref_compiled.py runs them.  designed(): every case is kept, none may be left out.  random_clips(): 200 clips of the
12-cell blob's and the 8-cell cube's fragments by 1 to 24 random planes, seeds fixed."""
import os

import numpy as np

import faces_ref as R
import regroup_ref as G
from helpers import fragment
from surtr_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
COLOUR = np.asarray((0.5, 0.25, 0.125), np.float32)
F32 = np.float32
ULP = 2.0 ** -23
SEED = 20261021
N_RANDOM = 200
N_RECORDED = 40          # of the random clips, the ones whose reference results are recorded in golden/reference_compiled.npz


def _solid(s):
    return {"pos": np.asarray(s["pos"], F32).reshape(-1, 3), "off": np.asarray(s["off"], np.uint32), "nbr": np.asarray(s["nbr"], np.int32)}


def unit_box():
    return _solid(scenes.box_solid((1, 1, 1), (0, 0, 0), factor=1.0))          # Poly::GetBB: vertex order and rings


def tetrahedron():
    return _solid(G.solid([(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1)], [[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]]))


def u_prism():
    """A prism over a U whose caps are cut into three convex quads.  (ClipPolyhedron relinks along face loops: over a face that is
    itself a U it would tie the two prongs together again.)  Cut below its two prongs it falls into two islands."""
    u = [(0, 0), (3, 0), (3, 3), (2, 3), (2, 1), (1, 1), (1, 3), (0, 3)]
    quads = [(0, 1, 4, 5), (1, 2, 3, 4), (0, 5, 6, 7)]
    faces = [list(q[::-1]) for q in quads] + [[8 + v for v in q] for q in quads] + [[k, (k + 1) % 8, 8 + (k + 1) % 8, 8 + k] for k in range(8)]
    pos = [(x, y, 0) for x, y in u] + [(x, y, 1) for x, y in u]
    return _solid(G.solid(pos, faces))


def _near(planes):
    """Every plane as it is, then with its offset moved: by 1e-12 (inside the reference's 1e-10 band where the offset is 0, rounded
    away elsewhere), by 2e-10 (just outside the band) and by one unit in the last place, each way."""
    out = []
    for p in planes:
        p = np.asarray(p, np.float64)
        out.append(p)
        for dd in (1e-12, -1e-12, 2e-10, -2e-10):
            out.append(p + (0, 0, 0, dd))
        w = max(abs(p[3]), 2.0 ** -126)
        out.append(p + (0, 0, 0, w * ULP))
        out.append(p - (0, 0, 0, w * ULP))
    return np.asarray(out, F32)


def _clip(name, solid, planes):
    return {"name": name, "op": "clip", "solid": solid, "planes": np.asarray(planes, F32).reshape(-1, 4)}


def _solid_ops(name, s, convex=False, limits=(4,)):
    out = [{"name": name + "/faces", "op": "faces", "solid": s}, {"name": name + "/moments", "op": "moments", "solid": s},
           {"name": name + "/render", "op": "render", "solid": s, "convex": False, "colour": COLOUR}]
    if convex:
        out.append({"name": name + "/fan", "op": "render", "solid": s, "convex": True, "colour": COLOUR})
    for lim in limits:
        out.append({"name": name + "/hull%d" % lim, "op": "hull", "points": s["pos"], "limit": min(lim, s["pos"].shape[0])})
    return out


WORLDS = {
    "identity": np.eye(4),
    "shift": [[1, 0, 0, 0.3], [0, 1, 0, -7.25], [0, 0, 1, 1e-3], [0, 0, 0, 1]],
    "rotate-scale": [[0.36, 0.48, -0.8, 2.0], [-0.8, 0.6, 0.0, -1.0], [0.48, 0.64, 0.6, 0.5], [0, 0, 0, 1]],
    "projective": [[1.1, 0.2, 0, 0.3], [0, 0.9, 0.1, 0], [0.3, 0, 1.2, -2], [0.01, 0.02, -0.03, 1.7]],
}
AXES = np.asarray([(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1), (1, -1, 0), (0.3, -0.2, 0.9), (0, 0, 0)], F32)


def designed():
    box, tet, u = unit_box(), tetrahedron(), u_prism()
    cases = []
    # ---- the two plain solids: every op
    for name, s in (("box", box), ("tetrahedron", tet)):
        cases += _solid_ops(name, s, convex=True, limits=(4, 5, 8))
        for w, m in WORLDS.items():
            cases.append({"name": "%s/transform-%s" % (name, w), "op": "transform", "solid": s, "world": np.asarray(m, F32)})
        cases.append({"name": name + "/kdop", "op": "kdop", "points": s["pos"], "normals": AXES, "ach": False, "max_axis_scale": 0.0, "gap_inv": 1.0})
        cases.append({"name": name + "/kdop-ach", "op": "kdop", "points": s["pos"], "normals": AXES, "ach": True, "max_axis_scale": 3.5, "gap_inv": 2000.0})
    # ---- planes through a vertex, an edge, a face; exactly and nearly
    through = {
        "box": {"vertex": [(1, -1, 0.5, -0.25), (1, 1, 1, -1.5), (-1, -1, -1, 1.5), (-1, 1, -0.5, 0.25)],
                "edge": [(1, -1, 0, 0), (1, 1, 0, -1), (-1, -1, 0, 1), (1, 0.5, 0, -0.75)],
                "face": [(1, 0, 0, -0.5), (-1, 0, 0, 0.5), (0, 0, 1, 0.5), (0, 0, -1, -0.5)]},
        "tetrahedron": {"vertex": [(0, 0, 1, -1), (0, 0, -1, 1), (1, -2, 0.5, -0.5), (-1, 2, -0.5, 0.5)],
                        "edge": [(1, -1, 0, 0), (-1, 1, 0, 0), (1, 1, 0, -1), (-1, -1, 0, 1)],
                        "face": [(0, -1, 0, 0), (0, 1, 0, 0), (1, 1, 1, -1), (-1, -1, -1, 1)]},
    }
    for name, s in (("box", box), ("tetrahedron", tet)):
        for what, planes in through[name].items():
            for k, p in enumerate(_near(planes)):
                cases.append(_clip("%s/plane-through-%s-%d" % (name, what, k), s, [p]))
        cases.append(_clip(name + "/removes-everything", s, [(1, 0, 0, 2)]))
        cases.append(_clip(name + "/removes-nothing", s, [(1, 0, 0, -2)]))
        cases.append(_clip(name + "/no-planes", s, np.zeros((0, 4))))
        cases.append(_clip(name + "/zero-plane", s, [(0, 0, 0, 0)]))
        # two planes that meet on an edge inside the solid; the second through the vertices the first one made
        cases.append(_clip(name + "/two-planes-on-an-edge", s, [(1, 0, 0, -0.25), (0, 1, 0, -0.25)]))
        cases.append(_clip(name + "/second-plane-through-new-vertices", s, [(1, 0, 0, -0.25), (1, 1, 0, -0.75), (0, 0, 1, -0.125)]))
        cases.append(_clip(name + "/same-plane-twice", s, [(0.3, -0.2, 0.9, -0.1), (0.3, -0.2, 0.9, -0.1), (-0.3, 0.2, -0.9, 0.1)]))
    # ---- a clip that leaves two islands, cleanly and with the cut in the plane of the U's inner face
    cases += _solid_ops("u-prism", u)
    for k, p in enumerate(_near([(0, -1, 0, 2), (0, -1, 0, 1)])):
        cases.append(_clip("u-prism/two-islands-%d" % k, u, [p]))
    cases.append(_clip("u-prism/two-islands-then-more", u, [(0, -1, 0, 1.5), (0, 0, 1, -0.5), (1, 0, 0.25, -2.5), (-1, 0.125, 0, 0.25)]))
    # ---- the refit: the 2x box of a Mesh (PrepareFracture's Convex) cut by the k-DOP over the Mesh's limited hull
    for name, mesh in (("tetrahedron", tet), ("u-prism", u), ("prism-5", _solid(R.prism_over(R.regular(5)))),
                       ("prism-17", _solid(R.prism_over(R.regular(17)))), ("star-8", _solid(R.prism_over(R.star(8))))):
        lo, hi = mesh["pos"].min(0), mesh["pos"].max(0)
        conv = _solid(scenes.box_solid(hi - lo, (hi + lo) / 2))
        for lim in (4, 9, 16 if name == "prism-17" else 32):          # (the engine's limited hull holds 63 faces: 32 of prism-17's 34 points make more)
            cases.append({"name": "%s/refit-%d" % (name, lim), "op": "refit", "convex": conv, "mesh": mesh, "limit": lim})
    # ---- faces of 3, 4, 5, 17, 64 and 65 vertices (prism caps, pyramid bases), convex ones also as fans
    for n in (3, 4, 5, 17, 64, 65):
        cases += _solid_ops("prism-%d" % n, _solid(R.prism_over(R.regular(n))), convex=True, limits=(4, 9))
        cases += _solid_ops("pyramid-%d" % n, _solid(R.pyramid_over(R.regular(n))), convex=True, limits=())
        cases.append(_clip("prism-%d/clip" % n, _solid(R.prism_over(R.regular(n))), [(0.2, 0.1, 1, -0.6), (1, 0, 0.1, -0.5)]))
    # ---- the ear clipper: a reflex corner, three collinear vertices, a whole collinear face, stars and a spiral
    ell = [(0, 0), (2, 0), (2, 1), (1, 1), (1, 2), (0, 2)]
    straight = [(0, 0), (1, 0), (2, 0), (2, 2), (0, 2)]
    for name, poly in (("reflex-corner", ell), ("three-collinear", straight), ("collinear-5", R.collinear(5)), ("star-8", R.star(8)),
                       ("star-64", R.star(64)), ("spiral-17", R.spiral(17)), ("spiral-65", R.spiral(65))):
        for r in (0, 1, len(poly) - 1):
            cases += _solid_ops("%s-r%d" % (name, r), _solid(R.prism_over(R.rotated(poly, r))), limits=())
    # ---- neighbour rings from triangle soups: closed, open, non-manifold
    z = np.load(os.path.join(HERE, "golden", "reference_models.npz"))
    cube_pos, cube_tris = z["cube_pos"], z["cube_tris"]
    tet_tris = [(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)]
    soups = {
        "cube": (cube_pos, cube_tris),
        "tetrahedron": (tet["pos"], tet_tris),
        "tetrahedron-inside-out": (tet["pos"], [t[::-1] for t in tet_tris]),
        "open-cube": (cube_pos, cube_tris[:-2]),
        "one-triangle": (tet["pos"][:3], [(0, 1, 2)]),
        "two-triangles": (tet["pos"], [(0, 1, 2), (0, 3, 1)]),
        "unused-vertex": (np.concatenate([tet["pos"], [[5, 5, 5]]]), tet_tris),
        # two tetrahedra that share one vertex; three triangles on one edge (more than two candidates at a fan step: the reference
        # would loop without progress, so no soup here has them)
        "bow-tie": (np.concatenate([tet["pos"], -tet["pos"][1:]]), tet_tris + [(0, 4, 5), (0, 6, 4), (4, 6, 5), (0, 5, 6)]),
        "fin": (np.concatenate([tet["pos"], [[0, -1, 0]]]), [(0, 1, 2), (0, 1, 3), (0, 1, 4)]),
    }
    for name, (p, t) in soups.items():
        cases.append({"name": "soup/" + name, "op": "neighbours", "pos": np.asarray(p, F32), "tris": np.asarray(t, np.int32)})
    return cases


def golden_cases(oracle):
    """The committed fixtures that are valid solids.  The clips of the degenerate ones (stale IDs, walks that do not end) only where
    the oracle says the reference stays inside its arrays, and their face walks only where the oracle's walk ends."""
    cases = []
    z = np.load(os.path.join(HERE, "golden", "cube8.npz"))
    cube = {"pos": z["mesh_pos"], "off": z["mesh_off"], "nbr": z["mesh_nbr"]}
    cases += _solid_ops("golden/cube8", _solid(cube), convex=True)
    cases.append(_clip("golden/cube8/cell0", _solid(cube), z["planes"][int(z["face_off"][0]):int(z["face_off"][1])]))
    z = np.load(os.path.join(HERE, "golden", "reference_models.npz"))
    cases.append({"name": "golden/bunny/neighbours", "op": "neighbours", "pos": z["bunny_pos"], "tris": z["bunny_tris"]})
    for name in ("degenerate_ach_cube", "degenerate_mesh_stale_id", "degenerate_sliver_convex", "degenerate_walk_bound_convex",
                 "pinched_face_fragment", "sliver_convex_walk_bound", "nonterminating_faces_fragment", "refit_invalid_in_reference"):
        z = np.load(os.path.join(HERE, "golden", name + ".npz"))
        for which in ("mesh", "conv"):
            s = _solid({"pos": z[which + "_pos"], "off": z[which + "_off"], "nbr": z[which + "_nbr"]})
            if "planes" in z.files:
                oracle.links_off_the_array(reset=True)
                oracle.clip(s, z["planes"])
                if oracle.links_off_the_array(reset=True) == 0:
                    cases.append(_clip("golden/%s/%s-clip" % (name, which), s, z["planes"]))
        if "conv_pos" in z.files:
            mesh, conv = (_solid({"pos": z[w + "_pos"], "off": z[w + "_off"], "nbr": z[w + "_nbr"]}) for w in ("mesh", "conv"))
            oracle.links_off_the_array(reset=True)
            oracle.refit(conv, mesh, 4)
            if oracle.links_off_the_array(reset=True) == 0:
                cases.append({"name": "golden/%s/refit" % name, "op": "refit", "convex": conv, "mesh": mesh, "limit": 4})
        if name == "pinched_face_fragment":
            cases += _solid_ops("golden/" + name, _solid({"pos": z["mesh_pos"], "off": z["mesh_off"], "nbr": z["mesh_nbr"]}), limits=(4,))
    return cases


_FRAGMENTS = {}


def scene_fragments(oracle):
    """(mesh, convex) of every fragment of scenes.blob_scene(12) and scenes.cube_scene(8), un-refitted, as the oracle's event
    leaves them: the inputs of the random clips and of the refits."""
    if not _FRAGMENTS:
        out = []
        for sc in (scenes.blob_scene(12), scenes.cube_scene(8)):
            planes = oracle.place_cells(sc["v012"], sc["scale"], sc["translate"])
            ev = oracle.event([sc["mesh"]], [sc["convex"]], sc["face_off"], planes, refit=False, render=False, threads=1)
            for k in range(ev["frag_ids"].shape[0]):
                out.append((_solid(fragment(ev, k, "mesh")), _solid(fragment(ev, k, "conv"))))
        _FRAGMENTS["all"] = out
    return _FRAGMENTS["all"]


def fragment_cases(oracle):
    """Every op on the two scenes' fragments: faces with reflex corners (the blob's Meshes), the refit at three point limits."""
    cases = []
    for k, (mesh, conv) in enumerate(scene_fragments(oracle)):
        cases += _solid_ops("fragment-%d/mesh" % k, mesh, limits=(4, 9))
        cases += _solid_ops("fragment-%d/convex" % k, conv, convex=True, limits=())
        for lim in (4, 9, 32):
            cases.append({"name": "fragment-%d/refit-%d" % (k, lim), "op": "refit", "convex": conv, "mesh": mesh, "limit": lim})
    return cases


def random_clips(oracle, n=N_RANDOM, seed=SEED):
    """n clips of a fragment (Mesh or Convex, in turn) by 1 to 24 planes.  A plane goes through a point of the fragment's box
    (stretched by a quarter) with a uniform direction; one plane in four goes through a vertex of the fragment instead, its
    offset rounded to float32 from the float32 dot product.  Fifteen planes in sixteen are turned so that they keep the middle of
    the box: most clips leave a solid that the later planes cut again."""
    frags = scene_fragments(oracle)
    rng = np.random.RandomState(seed)
    cases = []
    for c in range(n):
        mesh, conv = frags[rng.randint(len(frags))]
        s = mesh if c % 2 == 0 else conv
        lo, hi = s["pos"].min(0).astype(np.float64), s["pos"].max(0).astype(np.float64)
        planes = []
        for _ in range(rng.randint(1, 25)):
            nrm = rng.normal(size=3)
            nrm = nrm / np.linalg.norm(nrm)
            through_vertex = rng.randint(4) == 0
            p = s["pos"][rng.randint(s["pos"].shape[0])].astype(np.float64) if through_vertex else lo + (hi - lo) * (rng.uniform(size=3) * 1.5 - 0.25)
            if rng.randint(16) != 0 and np.dot(nrm, (lo + hi) / 2 - p) > 0:
                nrm = -nrm
            nrm = nrm.astype(F32)
            if through_vertex:
                q = p.astype(F32)
                d = -F32(F32(F32(nrm[0] * q[0]) + F32(nrm[1] * q[1])) + F32(nrm[2] * q[2]))
            else:
                d = F32(-np.dot(nrm.astype(np.float64), p))
            planes.append((nrm[0], nrm[1], nrm[2], d))
        cases.append(_clip("random-%03d" % c, s, planes))
    return cases


def recorded_random(cases):
    """The N_RECORDED random clips whose reference results are recorded: the first 39 of a solid of at most 64 vertices (Convexes,
    the cube's Meshes) and the first of a larger one (the blob's Meshes), which keeps the fixture small."""
    small = [c for c in cases if c["solid"]["pos"].shape[0] <= 64][:39]
    large = [c for c in cases if c["solid"]["pos"].shape[0] > 64][:1]
    return sorted(small + large, key=lambda c: c["name"])
