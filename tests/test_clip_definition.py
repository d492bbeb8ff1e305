"""The fracture event's clip against the float64 definition of cell n solid (tests/clip_ref.py), on every clipper a pair can take.

Every scene is first held against the definition with the oracle's event (the restated reference): that is the test of the scene
and where the constants come from.  Then the same checkers run on the engine, route by route, each run asserting from the
device counters that the route it names took pairs.

SCENES (the planes are oracle.place_cells' float32 planes, or written out, given to the engine with upload_planes):
  cube     a   meshgen.cube() x 8 cells
  blob     a   meshgen.blob(2, scale=3) x 64 cells
  grid     b   the cube [-1, 1]^3 x 4 axis-aligned cells through its vertices, edges and face centres (in-plane vertices)
  torus    c   meshgen.bumpy_torus(40, 24) x 64 cells (genus 1: caps with holes)
  tori     d   that torus and a quarter-size copy beside it in one piece x 48 cells (islands, cells that keep nothing)
  urchin   d   meshgen.urchin() x 64 cells (several islands per pair)
  whole    e   the blob in a cell that holds it whole, a cell that misses it and a half-space, in one event
  far      f   torus translated by (1000, -500, 250)
  second   g   the regular fragments of torus, each fractured by 6 cells of its own (fracture_pairs)
  torus60  c   meshgen.bumpy_torus(60, 40) x 32 cells: bands that leave the small-capacity record clipper no room
  halves       the cube [-1, 1]^3 halved by an oblique plane: the scene the mutations are made on

MEASURED on the oracle's event (the restated reference, never a kernel or the emulation): the largest |dJ| / (eps . L . A_c . L^k)
for k = 0, 1, 2; the largest vertex residual of (b), (c) / (eps . L); the Convex without refit: volume, first integrals (over
eps . L . A . L^k), Euclidean Hausdorff distance . sin(theta_min) / (eps . L); the refit: cover, inside, tight, each / (eps . L), over
the faces held to them; the faces excused as narrow / as needles; the seconds the scene's reference took where the figures were
taken (one CPU thread):
  scene      k=0    k=1    k=2    vertex   Convex: vol  first  Hausdorff   refit: cover inside tight  narrow needles   reference
  cube       0.329  0.245  0.199  2.78             0.59   0.455  3.95              4.36  4.00   -      14     0         0.01 s
  blob       0.232  0.139  0.086  2.95             0.538  0.307  15.76             3.35  2.54   1.87   54     54        0.3 s
  grid       0      0      0      0                0      0      0                 0     0      -      0      0         0.01 s
  torus      0.241  0.177  0.132  2.73             0.329  0.274  10.77             5.45  3.38   1.76   62     66        1.9 s
  tori       0.099  0.024  0.012  1.96             0.122  0.065  5.53              1.29  3.68   0.88   28     74        2.7 s
  urchin     0.235  0.135  0.078  2.28             0.564  0.496  12.81             2.55  3.51   1.20   11     33        2.0 s
  whole      0.054  0.006  0.005  1.57             0.004  0.068  0.94              1.07  0.80   1.40   0      0         0.02 s
  far        0.218  0.000  0.000  3.32             ('e-scene': vertices of Convex n C 1.3e-3 apart, 100 tau = 0.095)
                                                                                   4.66  2.81   2.68   69     54        2.0 s
  second     0.317  0.178  0.135  3.28             ('e-scene': the input Convexes are refitted ones, vertices 2e-7 apart)
                                                                                   6.27  4.17   1.86   546    622       2.9 s
  torus60    0.121  0.073  0.046  2.33             0.456  0.342  3.81              3.31  3.00   2.09   29     33        2.3 s
  halves     0.020  0.047  0.008  0.67             0.022  0.191  1.56              1.91  2.59   1.32   0      0         0.01 s
  RefittingPointLimit 12 (oracle.refit on every fragment):  blob  5.68  4.84  2.41  216  260;  torus  5.62  4.17  2.73  209  382
K = 2 (clip_ref.K, check (a)): four times 0.329, rounded up to a power of two.  K_E = 4 (check (e)): four times 0.59.  K_V = 16: four
times 3.32, the Mesh vertices of (b) and (c), which is what the residual of an interpolated point is; every Convex figure above is
held to tau = K_V eps L as it stands and is no part of the derivation (the largest, 15.76, is a Hausdorff distance: tau / sin(theta_min)
knows the angle of two planes, not the conditioning of three).  K_W = 4: the widest face below the needle bound that misses plain
tau is 0.79 tau wide (blob).  K_N = 64: the least elongated face that misses plain tau has D / w = 210 (torus at limit 12; 351 on
second at limit 4), a quarter of it as a power of two.  K_P = 8: four times 1.02 (per scene at the end of this file).
second: the term A_c . p of its (a) bound is up to 7.7 eps L A_c (p: the pieces' polygon faces are planar to that many float32
roundings), four times the K term; the oracle's event needs none of it (its ratios above are without the term).
far: the first and second integrals are taken about the centre of the scene's box while L^k is 1 000^k: their ratios vanish.
A pair without a fragment has no A_c: its bound takes the area of the triangles of S that no single plane of the cell separates from
it, plus 2^-40 L^3 L^k for the float64 sums of the reference (clip_ref.FLOOR); a cell that misses S is held to that floor alone.

LAMINAE AND NEGATIVE ISLANDS (reference-faithful deviations from (c) and (d)).  The reference's solids have no
face with a hole: the cap of a plane through the torus is two loops, the outer one covering the hole and the inner one taking it
back.  Later planes of the cell can cut both where S is not, and what is left there is two coincident sheets: zero volume,
vertices off S with winding number 0, rings that list a neighbour twice.  And the island split can separate the inner loop's part
from the outer's: an island of negative volume beside one that is too large by as much.  The integrals (a) hold unchanged (they
are per pair, and the sheets cancel), (b) holds unchanged; in (c) a vertex off S with winding number 0 is admitted only with its
twin of the other sheet within tau; (d)'s Euler and volume rules are not applied to a fragment whose rings list a neighbour twice,
and an island whose volume is not positive (beyond what float32 vertices resolve over its own area) is reported, not refused.
The oracle produces all of them.  LAMINAE and NEGATIVE below name every such fragment, scene by scene, and every run on every route
asserts exactly those sets: one more, one fewer or another one fails the test.  So it does for FLAT (islands whose volume is below
what their vertices resolve) and SHEETS: lamina flaps hang on ordinary fragments too, so the twin rule of (c) is open to every
fragment, but every fragment in which a vertex passed by it is reported and must be one of the named.

WHAT A BROKEN ENGINE LOOKS LIKE (tried once, by hand, on the emulation; dropping an island in the island split was not tried).  With the general clipper's cut point scaled by 1 + 1e-5 (clip_core.h, PlaneLineIntersection) the
emulation fails 25 of the 26 default-plan and route tests here in check (a), while the criteria of test_torus_4096_properties
evaluated on the same event still pass (volume sum off by 1.1e-5 of the whole, worst plane residual 5.1e-5, both under its 1e-4).
Classifying an in-plane vertex as clipped instead (side_of returning -1 for |s| < 1e-10) changes no test here, and should not: the
set is the same, the definition is blind to measure zero.
"""
import functools
import os
import time

import numpy as np
import pytest

import clip_ref as R
from helpers import run_gpu_child, solid_is_polyhedron
from surtr_amd import engine as E
from surtr_amd import meshgen, scenes

HERE = os.path.dirname(os.path.abspath(__file__))
LAMINAE = {"torus": [(17, 0, 0), (18, 0, 0), (30, 0, 0)], "far": [(17, 0, 0), (18, 0, 0), (30, 0, 0)],
           "second": [(84, 14, 0), (209, 34, 0)], "torus60": [(17, 0, 0)]}
NEGATIVE = {"tori": [(13, 0, 1)]}
# islands whose volume is below what float32 vertices resolve over their own area (K eps L A): two sheets that differ by roundings
FLAT = {"torus": [(40, 0, 0)], "far": [(40, 0, 0)], "second": [(8, 1, 0), (216, 36, 0), (217, 36, 0), (219, 36, 0), (220, 36, 0)]}
# fragments in which (c) let a vertex off S pass as one sheet of a lamina (winding number 0, its twin within tau)
_TORUS_SHEETS = [(2, 0, 0), (7, 0, 0), (15, 0, 0), (17, 0, 0), (18, 0, 0), (20, 0, 0), (24, 0, 0), (30, 0, 0), (40, 0, 0), (42, 0, 0), (60, 0, 0)]
SHEETS = {"torus": _TORUS_SHEETS, "far": _TORUS_SHEETS, "second": [(3, 0, 0), (101, 16, 0)],
          "tori": [(13, 0, 0), (13, 0, 1), (18, 0, 0), (20, 0, 0), (22, 0, 0), (24, 0, 0), (25, 0, 0), (27, 0, 0), (30, 0, 0), (40, 0, 0)],
          "torus60": [(2, 0, 0), (7, 0, 0), (15, 0, 0), (17, 0, 0), (20, 0, 0), (30, 0, 0), (31, 0, 0)]}


# ------------------------------------------------------------------ scenes
def _cells(cells):
    off, planes = [0], []
    for c in cells:
        planes += c
        off.append(len(planes))
    return np.array(off, np.uint32), np.array(planes, np.float32)


def _box(lo, hi):
    return [[-1, 0, 0, lo[0]], [1, 0, 0, -hi[0]], [0, -1, 0, lo[1]], [0, 1, 0, -hi[1]], [0, 0, -1, lo[2]], [0, 0, 1, -hi[2]]]


def _placed(v, t, n_cells):
    from oracle import oracle as O
    sc = scenes.make_scene(v, t, n_cells)
    return {"meshes": [sc["mesh"]], "convexes": [sc["convex"]], "plane_off": np.asarray(sc["face_off"], np.uint32),
            "planes": O.place_cells(sc["v012"], sc["scale"], sc["translate"]), "pairs": None}


def _given(v, t, cells, convex):
    off, planes = _cells(cells)
    return {"meshes": [E.neighbors_from_mesh(v, t)], "convexes": [convex], "plane_off": off, "planes": planes, "pairs": None}


def _two_tori():
    v, t = meshgen.bumpy_torus(40, 24)
    return np.concatenate([v, v * np.float32(0.25) + np.float32([4, 0, 0])]), np.concatenate([t, t + len(v)])


def _far_torus():
    v, t = meshgen.bumpy_torus(40, 24)
    return (v + np.float32([1000, -500, 250])).astype(np.float32), t


def _grid_cells():
    return [_box((ix, iy, -1), (ix + 1, iy + 1, 1)) for ix in (-1, 0) for iy in (-1, 0)]


def _second_level():
    """g: the regular fragments of the oracle's event on torus (chosen as test_refracture._refracture chooses its pieces, and
    without the named laminae), each with 6 cells of its own placed in its bounding box.
    The engine places these cells itself (place_cells_groups) while the reference takes oracle.place_cells' planes: that the two
    are the same bits is test_refracture's and test_gpu_parity's business, and a difference would fail here loudly, in (c).
    The scene is built from an oracle event, in the GPU child too: the oracle's library is what __graft_entry__.build() made."""
    from oracle import oracle as O
    from test_refracture import _links_symmetric
    first = oracle_event(O, built("torus")[0], refit=True)
    meshes, convexes = scenes.fragments_as_pieces(first)
    keep = [i for i, m in enumerate(meshes) if m["pos"].shape[0] >= 4 and np.diff(m["off"].astype(np.int64)).min() >= 3 and convexes[i]["pos"].shape[0] >= 4
            and _links_symmetric(m) and _links_symmetric(convexes[i]) and not R.has_doubled_neighbour(m)]
    meshes, convexes = [meshes[i] for i in keep], [convexes[i] for i in keep]
    rs = scenes.refracture_scene(meshes, convexes, 6)
    planes = []
    for p in range(len(meshes)):
        a, b = int(rs["group_cell_off"][p]), int(rs["group_cell_off"][p + 1])
        planes.append(O.place_cells(rs["v012"][int(rs["face_off"][a]):int(rs["face_off"][b])], rs["scales"][p], rs["shifts"][p]))
    return {"meshes": meshes, "convexes": convexes, "plane_off": np.asarray(rs["face_off"], np.uint32), "planes": np.concatenate(planes),
            "pairs": list(zip(rs["pair_cell"].tolist(), rs["pair_piece"].tolist())), "pattern": rs}


BUILDERS = {
    "cube": lambda: _placed(*meshgen.cube(), 8),
    "blob": lambda: _placed(*meshgen.blob(2, scale=3), 64),
    "grid": lambda: _given(*meshgen.cube(1.0), _grid_cells(), scenes.box_solid([2, 2, 2], [0, 0, 0])),
    "torus": lambda: _placed(*meshgen.bumpy_torus(40, 24), 64),
    "tori": lambda: _placed(*_two_tori(), 48),
    "urchin": lambda: _placed(*meshgen.urchin(), 64),
    "whole": lambda: _given(*meshgen.blob(2, scale=3), [_box((-4, -4, -4), (4, 4, 4)), _box((10, -1, -1), (12, 1, 1)),
                                                         _box((-4, -4, -4), (4, 4, 4)) + [[0.6, 0.48, 0.64, -0.25]]],
                            scenes.box_solid([7, 7, 7], [0, 0, 0])),
    "far": lambda: _placed(*_far_torus(), 64),
    "second": _second_level,
    # (for the mutations: the cube [-1, 1]^3 halved by an oblique plane, few large faces, every cut vertex on one plane only)
    "halves": lambda: _given(*meshgen.cube(1.0), [_box((-2, -2, -2), (2, 2, 2)) + [[0.6, 0.48, 0.64, -0.125]],
                                                   _box((-2, -2, -2), (2, 2, 2)) + [[-0.6, -0.48, -0.64, 0.125]]], scenes.box_solid([2, 2, 2], [0, 0, 0])),
    # (c again, with bands that leave the small-capacity record clipper of libsurtr_emul_rec.so no room)
    "torus60": lambda: _placed(*meshgen.bumpy_torus(60, 40), 32),
}


@functools.lru_cache(maxsize=None)
def built(name):
    """(scene dict, clip_ref.Scene with the reference of every pair, seconds the reference took)."""
    sc = BUILDERS[name]()
    t = time.time()
    ref = R.Scene(sc["meshes"], sc["plane_off"], sc["planes"], sc["pairs"])
    return sc, ref, time.time() - t


def oracle_event(oracle, sc, refit=False):
    if sc["pairs"] is None:
        return oracle.event(sc["meshes"], sc["convexes"], sc["plane_off"], sc["planes"], refit=refit, render=False, threads=4)
    parts, po = [], sc["plane_off"].astype(np.int64)      # a pair list: piece by piece, its own cells
    for p in range(len(sc["meshes"])):
        cells = sorted(c for c, q in sc["pairs"] if q == p)
        a, b = cells[0], cells[-1] + 1
        assert cells == list(range(a, b))
        ev = oracle.event([sc["meshes"][p]], [sc["convexes"][p]], po[a:b + 1] - po[a], sc["planes"][po[a]:po[b]], refit=refit, render=False, threads=4)
        ev["frag_ids"] = ev["frag_ids"] + np.array([a, p, 0], np.int32)
        parts.append(ev)
    return E.merge_fragments(parts)


def engine_event(engine_mod, sc, flags=0, in_flight=None, limit=None):
    """One event of the scene on the engine bound to engine_mod; the environment is read when the context is made, when the pieces
    are uploaded and when the event is planned, so whoever sets a switch sets it before this call."""
    eng = engine_mod.Engine(0)
    try:
        if in_flight:
            eng.set_events_in_flight(in_flight)
        if limit:
            eng.set_refit_point_limit(limit)
        eng.upload_pieces(sc["meshes"], sc["convexes"])
        if "pattern" in sc:      # (g: the engine places the cells of every group itself)
            rs = sc["pattern"]
            eng.upload_pattern(rs["face_off"], rs["v012"])
            eng.place_cells_groups(rs["group_cell_off"], rs["scales"], rs["shifts"])
        else:
            eng.upload_planes(sc["plane_off"], sc["planes"])
        n_cells, n_pieces = len(sc["plane_off"]) - 1, len(sc["meshes"])
        if sc["pairs"] is None:
            c = eng.fracture_event(0, n_cells, flags=flags)
            pairs = [(j // n_pieces, j % n_pieces) for j in range(n_cells * n_pieces)]
        else:
            pairs = [tuple(p) for p in sc["pairs"]]
            c = eng.fracture_pairs([p[0] for p in pairs], [p[1] for p in pairs], flags=flags)
        qs = np.array(eng.queue_stats(), np.int64)
        got = eng.download()
        ps = eng.pair_status(len(pairs))
    finally:
        eng.close()
    assert c.status == 0 and c.n_pairs == len(pairs)
    got["flagged_pairs"] = [pairs[j] for j in np.nonzero(ps)[0]]
    got["n_failed"] = int(c.n_failed)
    return got, qs


def hold(name, ev, **kw):
    """check_event on a scene, and the scene's laminae are the named ones."""
    sc, ref, _ = built(name)
    out = R.check_event(ref, ev, flagged_pairs=ev.get("flagged_pairs", ()), n_failed=ev.get("n_failed", 0), **kw)
    assert out["laminae"] == LAMINAE.get(name, []), (name, out["laminae"])
    assert out["negative"] == NEGATIVE.get(name, []), (name, out["negative"])
    assert out["flat"] == FLAT.get(name, []), (name, out["flat"])
    if "c" in kw.get("checks", "abcd"):
        assert out["sheets"] == SHEETS.get(name, []), (name, out["sheets"])
    return out


# ------------------------------------------------------------------ the reference itself
def test_unit_box_has_volume_one():
    box = scenes.box_solid((1, 1, 1), (0, 0, 0), factor=1.0)
    J = R.surface_J(box["pos"].astype(np.float64), R.fan_triangles(box), np.zeros(3))
    assert np.allclose(J, [1, 0, 0, 0, 1 / 12, 1 / 12, 1 / 12, 0, 0, 0], rtol=0, atol=1e-15)


def test_integrals_are_test_mass_properties_formulas():
    from test_mass_properties import tet_integrals
    rng = np.random.RandomState(5)
    P = rng.uniform(-2, 2, (40, 3))
    T = rng.randint(0, 40, (90, 3))
    assert np.allclose(R.tet_J(P[T[:, 0]], P[T[:, 1]], P[T[:, 2]]).sum(0), tet_integrals(P, T), rtol=1e-12, atol=1e-12)


def test_convex_clip_known_answers():
    """A box cut by a diagonal plane (a prism: half of it), a corner cut off (a tetrahedron of known integrals), moved origins."""
    box = R.box_faces([0, 0, 0], [1, 2, 3])
    assert np.allclose(R.body_J(box), [6, 3, 6, 9, 2, 8, 18, 3, 9, 4.5], rtol=1e-14)
    half = R.convex_clip(box, [[1.0, -0.5, 0, 0]])               # x <= y / 2
    assert abs(R.body_J(half)[0] - 3.0) < 1e-14
    corner = R.convex_clip(box, [[-1.0, -1.0, -1.0, 0.5]])       # keeps x + y + z >= 1/2: the box less the corner tetrahedron of legs 1/2
    assert abs(R.body_J(corner)[0] - (6.0 - 0.125 / 6.0)) < 1e-14
    tet = R.convex_clip(box, [[1.0, 1.0, 1.0, -0.5]])
    a = 0.5
    assert np.allclose(R.body_J(tet)[:7], [a ** 3 / 6, a ** 4 / 24, a ** 4 / 24, a ** 4 / 24, a ** 5 / 60, a ** 5 / 60, a ** 5 / 60], rtol=1e-13)
    assert np.allclose(R.body_J(tet)[7:], a ** 5 / 120, rtol=1e-13)
    assert R.convex_clip(box, [[1.0, 0, 0, 0.5]]) == []


def test_reference_of_a_cube_in_half_spaces_is_exact():
    """S n C where both are boxes: the reference's integrals against the closed form, and the choice of O does not matter."""
    v, t = meshgen.cube(1.0)
    mesh = E.neighbors_from_mesh(v, t)
    off, planes = _cells([_box((-0.25, -3, -3), (0.5, 0.75, 3)), _box((2, 2, 2), (3, 3, 3))])
    for origin in (np.zeros(3), np.array([0.3, -0.2, 5.0])):
        ref = R.reference_integrals(mesh, off, planes, origin)
        want = R.shift_J(R.body_J(R.box_faces([-0.25, -1, -1], [0.5, 0.75, 1]))[None], -origin[None])[0]
        assert np.allclose(ref[0], want, rtol=0, atol=1e-13), (ref[0], want)
        assert np.abs(ref[1]).max() < 1e-14


# ------------------------------------------------------------------ the scenes: the oracle alone passes every check
@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_oracle_passes_every_check(oracle, name):
    sc, ref, seconds = built(name)
    ev = oracle_event(oracle, sc)
    m = {}
    hold(name, ev, measure=m)
    print("%s: reference %.2f s, %d fragments, L %.4g, ratios %r" % (name, seconds, ev["frag_ids"].shape[0], ref.L, {k: round(v, 3) for k, v in m.items()}))
    # the constants are four times what the restated reference needs, at the least
    assert 4 * max(m["a0"], m["a1"], m["a2"]) <= R.K and 4 * m["v"] <= R.K_V, m


def test_second_level_planarity_term(oracle):
    """g: what the term A_c . p adds to the (a) bound, and that the oracle's event does not need it (its ratios without the term
    stay where the triangle meshes' are): the pieces' faces are planar to a few float32 roundings, p <= 8 eps L."""
    sc, ref, _ = built("second")
    assert len(sc["meshes"]) >= 40 and max(len(l) for loops in ref.loops for l in loops) > 3       # polygon faces
    assert 0 < max(ref.planarity) <= 8 * R.EPS * ref.L
    m = {}
    hold("second", oracle_event(oracle, sc), measure=m)
    assert max(m["a0"], m["a1"], m["a2"]) <= 1.0


# ------------------------------------------------------------------ CPU tier: every route on the emulation
def _counters_default(qs, n):
    assert qs[16:32].sum() + qs[65:71].sum() + qs[88] + qs[94] > 0


def _counters_wave_off(qs, n):
    assert qs[88] == 0 and qs[89] == 0 and qs[16:32].sum() + qs[65:71].sum() > 0


def _counters_wave_on(qs, n):
    assert qs[88] > 0, "the record clipper took no pair"


def _counters_handed(qs, n):
    assert qs[88] > 0 and qs[89] > 0 and qs[94] > 0, (qs[88], qs[89], qs[94])      # taken, handed on mid-way, clipped by the catcher


def _counters_swept(qs, n):
    assert qs[89] > 0 and qs[94] >= qs[89], (qs[89], qs[94])                        # nobody polls: the sweep takes every hand-over


def _counters_wave_big(qs, n):
    assert qs[88] > 0 and qs[16 + 14] + qs[16 + 15] > 0, (qs[88], qs[16:32].tolist())


def _counters_half(qs, n):
    assert qs[65:71].sum() > 0, "no pair went to the half-size kernel"


def _counters_quota0(qs, n):
    assert qs[16 + 14] + qs[16 + 15] == 0 and qs[16:30].sum() > 0, qs[16:32].tolist()    # no band admitted to the whole-CU kernel


def _counters_rec0(qs, n):
    assert qs[88] > 0 and qs[91] == 0, (qs[88], qs[91])                              # record clipper on images, no record image


def _counters_sorted0(qs, n):
    assert qs[92] == 0 and qs[88] > 0, (qs[92], qs[88])


def _counters_split0(qs, n):
    assert qs[94] == 0 and qs[16:32].sum() + qs[65:71].sum() + qs[88] > 0, qs[94]      # no catcher: the one-kernel arrangement


def _counters_front_par(on):
    def check(qs, n):
        # (ahead of the pre-pass k_clip_convex queues the pairs by pre-pass class; beside it the pre-pass takes them by index)
        assert (qs[48:64].sum() == 0) if on else (qs[48:64].sum() > 0), qs[48:64].tolist()
    return check


def _counters_small(qs, n):
    assert qs[84] > 0 or qs[16 + 14] + qs[16 + 15] > 0, qs[16:32].tolist()             # bands beyond the (tiny) LDS topology


def _counters_lean(on):
    def check(qs, n):
        assert qs[80] + qs[81] == n
        assert (qs[125] > 0) if on else (qs[125] == 0 and qs[87] == 0), (qs[125], qs[87])      # the second tier's ticket
    return check


# (id, scene, emulation library, environment, what the counters must show)
ROUTES = [
    ("wave0", "torus", "libsurtr_emul.so", {"SURTR_WAVE": "0"}, _counters_wave_off),
    ("wave1", "torus", "libsurtr_emul.so", {"SURTR_WAVE": "1"}, _counters_wave_on),
    ("wave1_little_room", "torus60", "libsurtr_emul_rec.so", {"SURTR_WAVE": "1"}, _counters_handed),
    ("wave1_little_room_no_poll", "torus60", "libsurtr_emul_rec.so", {"SURTR_WAVE": "1", "SURTR_CATCH_POLL": "0"}, _counters_swept),
    ("wave_big", "torus", "libsurtr_emul_mid.so", {"SURTR_WAVE": "1", "SURTR_WAVE_BIG": "1"}, _counters_wave_big),
    ("half", "torus", "libsurtr_emul.so", {"SURTR_HALF": "1"}, _counters_half),
    ("big_quota0", "torus", "libsurtr_emul_mid.so", {"SURTR_BIG_QUOTA": "0"}, _counters_quota0),
    ("rec0", "torus", "libsurtr_emul.so", {"SURTR_WAVE": "1", "SURTR_REC": "0"}, _counters_rec0),
    ("prep_sorted0", "torus", "libsurtr_emul.so", {"SURTR_WAVE": "1", "SURTR_PREP_SORTED": "0"}, _counters_sorted0),
    ("split0", "torus", "libsurtr_emul.so", {"SURTR_WAVE": "1", "SURTR_SPLIT": "0"}, _counters_split0),
    ("front_par0", "torus", "libsurtr_emul.so", {"SURTR_FRONT_PAR": "0"}, _counters_front_par(False)),
    ("front_par1", "torus", "libsurtr_emul.so", {"SURTR_FRONT_PAR": "1"}, _counters_front_par(True)),
    ("wide_global", "torus", "libsurtr_emul_small.so", {}, _counters_small),
    ("wide_global_islands", "tori", "libsurtr_emul_small.so", {}, _counters_small),
    ("cvx_lean0", "blob", "libsurtr_emul.so", {"SURTR_CVX_LEAN": "0"}, _counters_lean(False)),
    ("cvx_lean1", "blob", "libsurtr_emul.so", {"SURTR_CVX_LEAN": "1"}, _counters_lean(True)),
]


def _bound(emul_lib_path, lib):
    E._use_library_for_tests(os.path.join(os.path.dirname(emul_lib_path), lib))
    return E


def run_route(engine_mod, name, counters, flags=0, convex=True, **kw):
    """One event of a scene on the engine as bound and switched by the caller: the counters show the route, the Mesh fragments
    pass (a)-(d), the Convex fragments (e) without refit or (f) with it."""
    sc, ref, _ = built(name)
    got, qs = engine_event(engine_mod, sc, flags=flags, **kw)
    counters(qs, len(ref.pairs))
    hold(name, got)
    if convex:
        check_convexes(name, got, refit=bool(flags & 1), limit=kw.get("limit") or 4)
    return got, qs


@functools.lru_cache(maxsize=None)
def convex_scene(name):
    sc, ref, _ = built(name)
    return R.ConvexScene(ref, sc["convexes"])


# (e) needs a Convex n C without two vertices closer than 100 tau.  far: tau is 700 times the torus's while the cells are the same
# size.  second: the input Convexes are refitted ones, with vertices where four planes meet within rounding.  check (e) says so
# itself ('e-scene'), and that it does is asserted; (f) runs on both.
NO_E = ("far", "second")
# (f): the faces of the refitted Convexes excused from cover and tight as faces without a plane (narrower than K_W tau; needles with
# D >= K_N w), per (scene, RefittingPointLimit): the oracle's numbers, and every route has to come to the same.
NARROW = {("blob", 4): (54, 54), ("cube", 4): (14, 0), ("far", 4): (69, 54), ("grid", 4): (0, 0), ("halves", 4): (0, 0),
          ("second", 4): (546, 622), ("tori", 4): (28, 74), ("torus", 4): (62, 66), ("torus60", 4): (29, 33), ("urchin", 4): (11, 33),
          ("whole", 4): (0, 0), ("blob", 12): (216, 260), ("torus", 12): (209, 382)}      # (limit 12: oracle.refit fragment by fragment)


def check_convexes(name, ev, refit, limit=4, pin=True, **kw):
    """(e) or (f); a lamina has no Convex to speak of (a flat Mesh fragment's slabs leave nothing of it)."""
    if not refit and name in NO_E:
        with pytest.raises(R.CheckFailed) as e:
            R.check_convex_clip(convex_scene(name), ev)
        assert e.value.check == "e-scene", e.value
        return None
    skip = set(LAMINAE.get(name, []))
    keep = np.array([tuple(r) not in skip for r in ev["frag_ids"].tolist()], bool)
    if not keep.all():
        ks = np.nonzero(keep)[0]
        parts = {"frag_ids": ev["frag_ids"][ks]}
        for pre in ("mesh", "conv"):
            solids = [R.fragment(ev, int(k), pre) for k in ks]
            nv = np.cumsum([0] + [s["pos"].shape[0] for s in solids])
            parts[pre + "_vert_off"] = nv
            parts[pre + "_pos"] = np.concatenate([s["pos"] for s in solids])
            parts[pre + "_nbr_off"] = np.concatenate([[0]] + [s["off"][1:] + o for s, o in zip(solids, np.cumsum([0] + [len(s["nbr"]) for s in solids]))])
            parts[pre + "_nbr"] = np.concatenate([s["nbr"] for s in solids])
        ev = parts
    if not refit:
        return R.check_convex_clip(convex_scene(name), ev, **kw)
    narrow = R.check_refit(convex_scene(name), ev, **kw)
    if pin:
        assert narrow == NARROW[(name, limit)], (name, limit, narrow)
    return narrow


@pytest.mark.parametrize("name", sorted(set(BUILDERS) - {"torus60"}))
def test_default_plan_on_every_scene(emul_engine, name):
    run_route(emul_engine, name, _counters_default)


@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_every_route_delivers_the_definition(emul_lib_path, monkeypatch, route):
    _, name, lib, env, counters = route
    for k, v in env.items():
        monkeypatch.setenv(k, v)      # (before the context exists: SURTR_WAVE_BIG is read when it is made, SURTR_HALF at the upload, the rest per event)
    try:
        run_route(_bound(emul_lib_path, lib), name, counters)
    finally:
        E._use_library_for_tests(None)


@pytest.mark.parametrize("name", sorted(BUILDERS))
def test_convex_scenes_with_the_oracle(oracle, name):
    """(e) and (f) on the restated reference first; the ratios behind K_E (e0, e1), K_V (f_inside) and K_W (f_width: the widest face
    that misses plain tau, in tau) are printed."""
    sc, ref, _ = built(name)
    m = {}
    check_convexes(name, oracle_event(oracle, sc, refit=False), refit=False, measure=m)
    check_convexes(name, oracle_event(oracle, sc, refit=True), refit=True, measure=m)
    print(name, {k: round(float(v), 3) for k, v in m.items()})
    # (K_V comes from the Mesh vertices of (b) and (c); the Convex figures are held to tau as it is and are no part of its derivation)
    if name not in NO_E:
        assert 4 * max(m["e0"], m["e1"]) <= R.K_E and m["e_h"] <= R.K_V, m
    assert 4 * m.get("f_width", 0.0) <= R.K_W and m.get("f_needle", np.inf) >= 4 * R.K_N * 0.8, m      # (210 against 4 x 64: a power of two)


@pytest.mark.parametrize("limit", [4, 12])
@pytest.mark.parametrize("name", ["blob", "torus"])
def test_refit_delivers_the_definition(emul_engine, name, limit):
    """(f) with k_refit (RefittingPointLimit 4) and k_refit_n (12): the Mesh clip is the same event, the Convex is refitted."""
    sc, ref, _ = built(name)
    got, qs = engine_event(emul_engine, sc, flags=1, limit=limit)
    assert qs[82] + qs[83] > 0 and qs[95] == 0, (qs[82], qs[83], qs[95])      # refits done, none left un-refitted
    hold(name, got)
    check_convexes(name, got, refit=True, limit=limit)
    if limit > 4:       # more normals, a tighter Convex: k_refit_n did run with its own limit
        got4, _ = engine_event(emul_engine, sc, flags=1, limit=4)
        assert got["conv_pos"].shape[0] > got4["conv_pos"].shape[0]


# ------------------------------------------------------------------ the checker has teeth
def _copy(ev):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in ev.items()}


def _refused(name, ev, check):
    """The named check, run alone, refuses the event."""
    with pytest.raises(R.CheckFailed) as e:
        R.check_event(built(name)[1], ev, checks=check)
    assert e.value.check == check, e.value
    return e.value


def _cut_vertices(name, ev):
    """(index into mesh_pos, fragment, cell, the plane it lies on, its neighbours' indices) of the vertices cut by exactly one plane."""
    sc, ref, _ = built(name)
    keys = set(ref.keys[0])
    out = []
    for k, (c, p, i) in enumerate(ev["frag_ids"].tolist()):
        a = int(ev["mesh_vert_off"][k])
        f = R.fragment(ev, k)
        cp = ref.cell_planes(c)
        s = f["pos"].astype(np.float64) @ cp[:, :3].T + cp[:, 3]
        for v in range(f["pos"].shape[0]):
            on = np.nonzero(np.abs(s[v]) <= ref.tau)[0]
            if f["pos"][v].tobytes() not in keys and on.size == 1:
                out.append((a + v, k, c, cp[on[0]], [a + int(u) for u in f["nbr"][f["off"][v]:f["off"][v + 1]]]))
    return out


def test_moved_cut_vertices_are_refused(oracle):
    """One cut vertex moved by 64 tau along the input edge it was cut on: it stays on S, so only the integrals (a) can see it.
    What (a) resolves is a volume of K eps L A_c; the move changes the fragment's volume by 64 tau times a third of the cap
    triangle at that vertex, which is more than twice the bound for most cut vertices of this scene: (a) must refuse every one of
    those (and may pass the vertices between two close neighbours).  Moved by 64 tau off its plane: (c), always."""
    sc, ref, _ = built("halves")
    ev = oracle_event(oracle, sc)
    hold("halves", ev)
    keys = set(ref.keys[0])
    cuts = _cut_vertices("halves", ev)
    assert len(cuts) >= 6
    moved = 0
    for g, k, c, plane, nbrs in cuts:
        old = [u for u in nbrs if ev["mesh_pos"][u].tobytes() in keys]
        if not old:
            continue
        d = ev["mesh_pos"][old[0]].astype(np.float64) - ev["mesh_pos"][g].astype(np.float64)      # (towards the kept end of its edge)
        bad = _copy(ev)
        bad["mesh_pos"][g] = (bad["mesh_pos"][g].astype(np.float64) + 64 * ref.tau * d / np.linalg.norm(d)).astype(np.float32)
        vol = [R.surface_J(R.fragment(e, k)["pos"].astype(np.float64), R.fan_triangles(R.fragment(e, k)), ref.origin)[0] for e in (ev, bad)]
        area = sum(R.surface_area(R.fragment(ev, j)["pos"].astype(np.float64), R.fan_triangles(R.fragment(ev, j)))
                   for j in np.nonzero(ev["frag_ids"][:, 0] == c)[0])
        if abs(vol[1] - vol[0]) > 2 * ref.bound(area)[0]:
            _refused("halves", bad, "a")
            moved += 1
        n = plane[:3] / np.linalg.norm(plane[:3])
        for sign in (1.0, -1.0):
            bad = _copy(ev)
            bad["mesh_pos"][g] = (bad["mesh_pos"][g].astype(np.float64) + sign * 64 * ref.tau * n).astype(np.float32)
            _refused("halves", bad, "c")
    assert moved >= 4, moved


def test_island_in_the_neighbouring_cells_pair_is_refused(oracle):
    sc, ref, _ = built("urchin")
    ev = oracle_event(oracle, sc)
    ids = ev["frag_ids"]
    k = int(np.nonzero(ids[:, 2] == 1)[0][0])                      # a second island
    c = int(ids[k, 0])
    other = int(ids[ids[:, 0] != c][0, 0])
    bad = _copy(ev)
    bad["frag_ids"][k] = [other, 0, int((ids[:, 0] == other).sum())]
    _refused("urchin", bad, "a")


def _without_vertex(ev, k, v, unlink):
    """The event with vertex v of Mesh fragment k taken out of the arrays.  unlink: its neighbours forget it (the hole closes
    into one face); otherwise their rings keep the entry, which now names whatever vertex slid into its place."""
    f = R.fragment(ev, k)
    a = int(ev["mesh_vert_off"][k])
    h0 = int(ev["mesh_nbr_off"][a])
    nv = f["pos"].shape[0]
    rings = [f["nbr"][f["off"][u]:f["off"][u + 1]].tolist() for u in range(nv)]
    new = []
    for u in range(nv):
        if u == v:
            continue
        r = [w for w in rings[u] if not (unlink and w == v)]
        new.append([w - 1 if w > v else (w if w < v else min(v, nv - 2)) for w in r])
    out = _copy(ev)
    out["mesh_pos"] = np.delete(ev["mesh_pos"], a + v, 0)
    vo = ev["mesh_vert_off"].astype(np.int64).copy()
    vo[k + 1:] -= 1
    out["mesh_vert_off"] = vo
    flat = np.array([w for r in new for w in r], ev["mesh_nbr"].dtype)
    h1 = int(ev["mesh_nbr_off"][a + nv])
    out["mesh_nbr"] = np.concatenate([ev["mesh_nbr"][:h0], flat, ev["mesh_nbr"][h1:]])
    no = ev["mesh_nbr_off"].astype(np.int64)
    mine = h0 + np.cumsum([0] + [len(r) for r in new])
    out["mesh_nbr_off"] = np.concatenate([no[:a], mine[:-1], no[a + nv:] - (h1 - h0) + len(flat)])
    return out


def test_dropped_interior_vertex_is_refused(oracle):
    """An input vertex deep inside its cell taken out of its fragment: (b) misses it however cleanly it was unlinked (then the
    hole closes into a face and the shape is a polyhedron: (d) has nothing to say); with the links left, (d) refuses it too."""
    sc, ref, _ = built("blob")
    ev = oracle_event(oracle, sc)
    hold("blob", ev)
    keys = {key: v for v, key in enumerate(ref.keys[0])}
    found = None
    for k, (c, p, i) in enumerate(ev["frag_ids"].tolist()):
        cp = ref.cell_planes(c)
        f = R.fragment(ev, k)
        for v in range(f["pos"].shape[0]):
            key = f["pos"][v].tobytes()
            if key in keys and ((ref.pos64[0][keys[key]] @ cp[:, :3].T + cp[:, 3]) < -ref.tau).all():
                found = (k, v)
                break
        if found:
            break
    assert found
    _refused("blob", _without_vertex(ev, found[0], found[1], unlink=True), "b")
    _refused("blob", _without_vertex(ev, found[0], found[1], unlink=False), "d")


def test_swapped_cells_are_refused(oracle):
    sc, ref, _ = built("blob")
    ev = oracle_event(oracle, sc)
    ids = ev["frag_ids"]
    c0, c1 = int(ids[0, 0]), int(ids[-1, 0])
    assert c0 != c1
    bad = _copy(ev)
    bad["frag_ids"][ids[:, 0] == c0, 0] = c1
    bad["frag_ids"][ids[:, 0] == c1, 0] = c0
    _refused("blob", bad, "a")
    _refused("blob", bad, "c")


def _push_face(ev, k, j, loops, normal, by):
    out = _copy(ev)
    a = int(ev["conv_vert_off"][k])
    for v in loops[j]:
        out["conv_pos"][a + v] = (out["conv_pos"][a + v].astype(np.float64) + by * normal).astype(np.float32)
    return out


def test_pushed_refit_planes_are_refused(oracle):
    """Every face of every refitted Convex of blob that is held to cover and tight and is no given plane (a slab of the k-DOP),
    pushed inward by 64 tau: the Mesh sticks out (cover); pushed outward: it touches nothing any more (tight)."""
    sc, ref, _ = built("blob")
    C = convex_scene("blob")
    ev = oracle_event(oracle, sc, refit=True)
    R.check_refit(C, ev)
    done = 0
    for k, (c, p, i) in enumerate(ev["frag_ids"].tolist()):
        f, m = R.fragment(ev, k, "conv"), R.fragment(ev, k, "mesh")
        fp, loops = R.newell_planes(f)
        cpos, mpos = f["pos"].astype(np.float64), m["pos"].astype(np.float64)
        pl = C.all_planes((c, p))
        sc_ = cpos @ pl[:, :3].T + pl[:, 3]
        w = R.face_widths(cpos, loops)
        for j, l in enumerate(loops):
            D = np.sqrt(((mpos - cpos[l].mean(0)) ** 2).sum(1).max())
            # (a slab, well away from every given plane so that the push does not turn it into one, and held to the checks)
            if (np.abs(sc_[l]).max(0) <= 256 * ref.tau).any() or w[j] < 2 * R.K_W * ref.tau or D >= R.K_N * w[j] / 2:
                continue
            with pytest.raises(R.CheckFailed) as e:
                R.check_refit(C, _push_face(ev, k, j, loops, fp[j, :3], -64 * ref.tau), only=("cover",), fragments=(k,))
            assert e.value.check == "f-cover"
            with pytest.raises(R.CheckFailed) as e:
                R.check_refit(C, _push_face(ev, k, j, loops, fp[j, :3], 64 * ref.tau), only=("tight",), fragments=(k,))
            assert e.value.check == "f-tight"
            done += 1
    assert done >= 100, done


# ------------------------------------------------------------------ the planes as given: their conditioning
# Largest deviation / conditioning per scene: cube 1.02, blob 0.81, torus 0.95, tori 0.48, urchin 0.85, far 0.00 (L / edge is 10^4
# there and the deviation no larger than elsewhere), torus24 0.76.  The largest deviation itself: 4.99e-5, on torus24.
K_P = 8.0      # four times 1.02, rounded up to a power of two


def plane_deviation(v012, scale, shift, planes):
    """Per face: how far the float32 placed plane (the reference's ConstructFacePlane from a face's first three placed vertices) is
    from the float64 plane through the same three float32 points, in normalised coefficients (the offset relative to the size
    of the points' coordinates), and the conditioning of the three points: eps / sin(angle at v0) . L / shortest of the two
    edges at v0, L the largest absolute coordinate among them."""
    v = np.asarray(v012, np.float32).reshape(-1, 3, 3)
    p = ((v * np.asarray(scale, np.float32)).astype(np.float32) + np.asarray(shift, np.float32)).astype(np.float32).astype(np.float64)
    a, b = p[:, 0] - p[:, 1], p[:, 0] - p[:, 2]
    n = np.cross(a, b)
    ln = np.linalg.norm(n, axis=1)
    n /= ln[:, None]
    w = -np.einsum("ij,ij->i", n, p[:, 0])
    L = np.abs(p).max((1, 2))
    la, lb = np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1)
    pl = np.asarray(planes, np.float32).astype(np.float64)
    dev = np.maximum(np.abs(pl[:, :3] - n).max(1), np.abs(pl[:, 3] - w) / L)
    cond = R.EPS / (ln / (la * lb)) * L / np.minimum(la, lb)
    return dev, cond


@pytest.mark.parametrize("name", ["cube", "blob", "torus", "tori", "urchin", "far", "torus24"])
def test_placed_planes_are_as_good_as_their_three_points(oracle, name):
    """The float32 placed planes differ from the float64 plane through the same three placed points by up to 4.99e-5 in normalised
    coefficients where the three points are close together or nearly in line: within K_P times the conditioning, never more.  This
    is why the clip is defined on the planes as given, and why neighbouring cells do not share a bisector to better than this."""
    mesh = {"cube": meshgen.cube, "blob": lambda: meshgen.blob(2, scale=3), "torus": lambda: meshgen.bumpy_torus(40, 24), "tori": _two_tori,
            "urchin": meshgen.urchin, "far": _far_torus, "torus24": lambda: meshgen.bumpy_torus(24, 12)}[name]()
    n = {"cube": 8, "tori": 48, "torus24": 32}.get(name, 64)
    sc = scenes.make_scene(*mesh, n)
    planes = oracle.place_cells(sc["v012"], sc["scale"], sc["translate"])
    dev, cond = plane_deviation(sc["v012"], sc["scale"], sc["translate"], planes)
    print(name, "largest deviation %.3g, largest ratio to the conditioning %.3f" % (dev.max(), (dev / cond).max()))
    assert 4 * (dev / cond).max() <= K_P
    assert (dev <= K_P * cond).all()


# ------------------------------------------------------------------ a designed literal-clipper input: the flag rule
def test_designed_degenerate_input_is_flagged_or_right(emul_engine, oracle):
    """tests/golden/degenerate_walk_bound_convex.npz (a sliver piece whose relink walk runs into the reference's step bound) cut
    by its own planes: a pair the engine flags is excused only if the restated reference's own result for it is no polyhedron;
    every other pair must deliver the integrals of the definition."""
    z = np.load(os.path.join(HERE, "golden", "degenerate_walk_bound_convex.npz"))
    mesh = {"pos": z["mesh_pos"], "off": z["mesh_off"], "nbr": z["mesh_nbr"]}
    conv = {"pos": z["conv_pos"], "off": z["conv_off"], "nbr": z["conv_nbr"]}
    planes = np.asarray(z["planes"], np.float32).reshape(-1, 4)
    sc = {"meshes": [mesh], "convexes": [conv], "plane_off": np.array([0, planes.shape[0]], np.uint32), "planes": planes, "pairs": None}
    got, qs = engine_event(emul_engine, sc, flags=0)
    ref_ev = oracle_event(oracle, sc)
    for pair in got["flagged_pairs"]:
        mine = [k for k, r in enumerate(ref_ev["frag_ids"].tolist()) if (r[0], r[1]) == pair]
        assert not mine or any(not solid_is_polyhedron(dict(R.fragment(ref_ev, k, w), off=R.fragment(ref_ev, k, w)["off"].astype(np.uint32)))
                               or R.has_doubled_neighbour(R.fragment(ref_ev, k, w)) for k in mine for w in ("mesh", "conv")), pair
    # (the piece is two coincident sheets: its rings list neighbours twice, S n C has no volume and the pair no fragment)
    ref = R.Scene(sc["meshes"], sc["plane_off"], sc["planes"])
    assert abs(ref.ref[(0, 0)][0]) <= ref.bound(ref.area[0])[0]
    R.check_event(ref, got, flagged_pairs=got["flagged_pairs"], n_failed=got["n_failed"], allow_flags=True, checks="a")


# ------------------------------------------------------------------ GPU tier
# Per child (one scene): the reference once, then one new Engine per route.  Measured on the emulation for the same case: torus60
# 2.3 s for the reference + 8 events of 0.4 s each = 6 s, second 5.7 s, the other scenes 0.1 .. 3.7 s: the children get ten times
# that, 30 s at the least.
# (the device's pre-pass kernel takes pieces of 2 048 vertices and more, and only its bands reach the record clipper: scene c's routes
#  run on its 2 400-vertex version)
def _counters_small_piece(qs, n):
    assert qs[88] == 0 and qs[89] > 0, (qs[88], qs[89])      # forced on, it finishes no pair: each is handed on to the general clipper


GPU_ROUTES = {
    "torus": [("wave1_below_the_prepass", {"SURTR_WAVE": "1"}, {}, _counters_small_piece)],
    "torus60": [("wave0", {"SURTR_WAVE": "0"}, {}, _counters_wave_off), ("wave1", {"SURTR_WAVE": "1"}, {}, _counters_wave_on),
              ("half", {"SURTR_HALF": "1"}, {}, _counters_half), ("cvx_lean0", {"SURTR_CVX_LEAN": "0"}, {}, _counters_lean(False)),
              ("cvx_lean1", {"SURTR_CVX_LEAN": "1"}, {}, _counters_lean(True)), ("in_flight6", {}, {"in_flight": 6}, _counters_wave_on)],
}


def gpu_case(name, lib=None):
    """What a child of the GPU tier runs: the scene under the default plan without and with refit, then the scene's routes.
    (lib: an emulation library instead of the device, to time the same case on the CPU.)"""
    E._use_library_for_tests(lib)
    t = time.time()
    built(name)
    print("%s: reference %.2f s" % (name, time.time() - t))
    for flags in (0, 1):
        run_route(E, name, _counters_default, flags=flags)
    failed = []
    for rid, env, kw, counters in GPU_ROUTES.get(name, []):
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            t = time.time()
            run_route(E, name, counters, flags=1, **kw)
            print("%s %s: %.2f s" % (name, rid, time.time() - t))
        except AssertionError as e:      # (a check that refuses, not an error of the engine: the other routes still say what they have to)
            failed.append((rid, repr(e)[:600]))
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    assert not failed, failed
    print("ok " + name)


_CHILD = """
import sys
sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
import test_clip_definition as T
T.gpu_case(sys.argv[1])
"""


@pytest.mark.gpu
@pytest.mark.parametrize("name,seconds", [("cube", 30), ("blob", 30), ("grid", 30), ("torus", 60), ("torus60", 90), ("tori", 60), ("urchin", 60),
                                          ("whole", 30), ("far", 60), ("second", 90)])
def test_gpu_delivers_the_definition(gpu_engine, name, seconds):
    run_gpu_child(_CHILD, name, seconds)
