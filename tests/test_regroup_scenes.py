"""Compound regrouping (surtr_event_regroup, regroup_dev.hip) on scenes whose answer is known by construction.

Every scene is built from explicit face loops (Convex = Mesh = the same solid) and handed to four implementations that must give
the same compounds: the plain reference of tests/regroup_ref.py (float64, all pairs of faces, union-find), the oracle's
restatement of HandleConvexIsland, the host version (surtr_regroup) and the device step (Engine.event_regroup) -- on the
single-lane emulation here, on the GPU in the tests marked gpu, which run the same families.

Robustness is a condition on the INPUT, asserted on the plain reference before anything is compared: a scene is either exact
(every coordinate a short dyadic rational and every plane axis-aligned, so every product of the rule is exact in float32; the
deliberate on-the-threshold cases are of this kind) or every decision the reference takes is at least 100 float32 roundings of
its quantity away from its threshold.  No case is skipped or filtered.

The races of k_rg_labels_all (1024 threads, atomicMin, a two-slot `changed` flag) do not exist on the emulation, which runs the
kernel with one thread: the chains of 1500 pieces in the gpu tier are their only check.

Runtime of the CPU tier of this module: see RUNTIME below (measured once, one core)."""
import numpy as np
import pytest

import regroup_ref as R
from surtr_amd import scenes

RUNTIME = "about 65 s on one core for the 13 tests not marked gpu (38 s of it test_long_chain: six chains of 1500 boxes), 19 s on an MI355X for the 13 that are"


# ---- running one scene through the four implementations ------------------------------------------------------------------------
def _lists(off, flat):
    return [flat[int(off[i]):int(off[i + 1])].tolist() for i in range(len(off) - 1)]


def _axis_aligned(pieces):
    for p in pieces:
        pos = np.asarray(p["pos"], np.float64)
        for loop in p["faces"]:
            n = np.cross(pos[loop[1]] - pos[loop[0]], pos[loop[2]] - pos[loop[0]])
            if np.count_nonzero(n) != 1:
                return False
    return True


def assert_robust(pieces, info, exact, extra_points=()):
    m = info["margins"]
    if exact:
        assert R.is_dyadic([p["pos"] for p in pieces] + [np.asarray(e, np.float64).reshape(-1, 3) for e in extra_points], squares=bool(extra_points))
        assert _axis_aligned(pieces)
        # what is left inexact in such a scene is the square root of the sphere test: on the threshold exactly, or well off it
        assert m.ratio["vertex"] >= 100.0, ("vertex", m.margin, m.ratio)
    else:
        assert m.smallest_ratio() >= 100.0 and not any(m.zeros.values()), (m.margin, m.ratio, m.zeros)


def load(eng, pieces, cells):
    ids = np.zeros((len(pieces), 3), np.int32)
    ids[:, 0] = cells
    eng.load_fragments(pieces, pieces, ids)


def four_ways(engine_mod, oracle, pieces, cells, exact=True, eng=None, **sphere):
    """-> (compounds as lists, info of the reference, stats of the device step).  sphere: partial, sphere_points, origin, radius."""
    cells = np.asarray(cells, np.int32)
    ref_kw = {("cloud" if k == "sphere_points" else k): v for k, v in sphere.items()}
    ro, rp, info = R.regroup(pieces, cells, **ref_kw)
    assert_robust(pieces, info, exact, [sphere[k] for k in ("sphere_points", "origin") if sphere.get(k) is not None and len(sphere[k])])
    oo, op = oracle.regroup(pieces, cells, **sphere)
    ho, hp = engine_mod.regroup(pieces, cells, **sphere)
    own = eng is None
    eng = engine_mod.Engine(0) if own else eng
    try:
        load(eng, pieces, cells)
        do, dp = eng.event_regroup(**sphere)
        stats = eng.regroup_stats()
    finally:
        if own:
            eng.close()
    want = _lists(ro, rp)
    assert _lists(oo, op) == want, "oracle"
    assert _lists(ho, hp) == want, "host"
    assert _lists(do, dp) == want, "device"
    assert stats["pieces"] == len(pieces) and stats["faces"] == sum(len(p["faces"]) for p in pieces)
    assert stats["face_points"] == sum(len(f) for p in pieces for f in p["faces"])
    assert stats["edges"] == info["touching_face_pairs"] and stats["edges"] <= stats["cap_edges"] == 16 * stats["faces"] + 1024
    assert stats["out_of_sphere"] == info["out_of_sphere"]
    return want, info, stats


def expected_from_blocks(cells, blocks):
    """The compounds of pieces whose islands are known: bind 0, per run of equal cells the island of its lowest piece, then the
    other islands, run by run, each by its lowest piece."""
    runs, extra = [[]], []
    start = 0
    for p in range(1, len(cells) + 1):
        if p == len(cells) or cells[p] != cells[p - 1]:
            groups = {}
            for q in range(start, p):
                groups.setdefault(blocks[q], []).append(q)
            g = sorted(groups.values(), key=lambda s: s[0])
            runs.append(g[0])
            extra += g[1:]
            start = p
    return runs + extra


B = R.box
JOINED, SPLIT = [[], [0, 1]], [[], [0], [1]]


def tilted_pair(angle):
    """A unit box and a smaller one whose facing side is turned away by `angle` about the line x = 1, y = 0."""
    c, s = np.cos(angle), np.sin(angle)
    rot = np.array([[c, s, 0.0], [-s, c, 0.0], [0.0, 0.0, 1.0]])        # turns the normal (-1, 0, 0) into (-c, s, 0)
    b = R.moved(R.moved(B((1, .25, .25), (2, .75, .75)), shift=(-1, 0, -.5)), matrix=rot, shift=(1, 0, .5))
    return [B((0, 0, 0), (1, 1, 1)), b]


# Every answer below follows from the rule as tests/regroup_ref.py states it (strict `> 0` for a point in a polygon, planes compared
# by their distance from the ORIGIN); several are not what geometry would say.  DESIGN.md section 3.6 records them.
PREDICATE_EDGES = {
    # the two facing squares coincide: every vertex lies on the other's edges, none strictly inside
    "identical_faces": ([B((0, 0, 0), (1, 1, 1)), B((1, 0, 0), (2, 1, 1))], SPLIT, True),
    # staggered by half in both directions of the plane: a vertex of each lies strictly inside the other
    "half_staggered": ([B((0, 0, 0), (1, 1, 1)), B((1, .5, .5), (2, 1.5, 1.5))], JOINED, True),
    "shared_edge_only": ([B((0, 0, 0), (1, 1, 1)), B((1, 1, 0), (2, 2, 1))], SPLIT, True),
    "shared_corner_only": ([B((0, 0, 0), (1, 1, 1)), B((1, 1, 1), (2, 2, 2))], SPLIT, True),
    # staggered by half in ONE direction: the faces overlap in half a square, but every vertex in range lies on an edge
    "vertex_on_edge": ([B((0, 0, 0), (1, 1, 1)), B((1, .5, 0), (2, 1.5, 1))], SPLIT, True),
    # no vertex of the large face is in the small one: only the second direction ("one more chance") finds it
    "small_face_inside_large": ([B((0, -3, -3), (1, 3, 3)), B((1, -1, -1), (2, 1, 1))], JOINED, True),
    "large_face_around_small": ([B((1, -1, -1), (2, 1, 1)), B((0, -3, -3), (1, 3, 3))], JOINED, True),
    # the faces cross like a plus: they overlap, but no vertex of either lies in the other
    "plus_overlap": ([B((0, -1, -3), (1, 1, 3)), B((1, -3, -1), (2, 3, 1))], SPLIT, True),
    "gap_inside_window": ([B((0, 0, 0), (1, 1, 1)), B((1 + 2.0 ** -10, .5, .5), (2, 1.5, 1.5))], JOINED, True),      # 2^-10 < 1e-3
    "gap_outside_window": ([B((0, 0, 0), (1, 1, 1)), B((1 + 2.0 ** -9, .5, .5), (2, 1.5, 1.5))], SPLIT, True),       # 2^-9 > 1e-3
    "tilt_0.01": (tilted_pair(0.01), JOINED, False),       # 1 - cos 0.01 = 5.0e-5 < 1e-4
    "tilt_0.02": (tilted_pair(0.02), SPLIT, False),        # 1 - cos 0.02 = 2.0e-4
    # two units apart, but the planes x = 1 and x = -1 are equally far from the origin, the normals are opposite and the squares
    # overlap once projected along the normal: joined
    "mirrored_overlapping": ([B((1, 0, 0), (2, 1, 1)), B((-2, -.5, -.5), (-1, .5, .5))], JOINED, True),
    "mirrored_apart": ([B((1, 0, 0), (2, 1, 1)), B((-2, 5, 5), (-1, 6, 6))], SPLIT, True),
}


def check_predicate_edges(engine_mod, oracle):
    for name, (pieces, want, exact) in PREDICATE_EDGES.items():
        got, info, _ = four_ways(engine_mod, oracle, pieces, [0, 0], exact=exact)
        assert got == want, (name, got)
        assert (info["touching_face_pairs"] > 0) == (want == JOINED), name
    m = R.regroup(*[PREDICATE_EDGES["shared_edge_only"][0], [0, 0]])[2]["margins"]
    assert m.zeros["right"] > 0                       # the on-the-threshold cases really are on it
    assert R.regroup(PREDICATE_EDGES["gap_inside_window"][0], [0, 0])[2]["margins"].margin["window"] == 1e-3 - 2.0 ** -10


def check_walk_returns_the_builders_loops(engine_mod, oracle):
    """The rings derived from the face loops give ExtractFaces the same loops in the same sense (up to where a loop starts)."""
    eng = engine_mod.Engine(0)
    for s in (B((0, 0, 0), (1, 2, 3)), R.prism(7), tilted_pair(0.01)[1]):
        fo, fi = eng.extract_faces(s)
        got = [fi[fo[k]:fo[k + 1]].tolist() for k in range(len(fo) - 1)]

        def canon(loop):
            k = loop.index(min(loop))
            return tuple(loop[k:] + loop[:k])
        assert sorted(map(canon, got)) == sorted(map(canon, s["faces"]))
    eng.close()


# ---- brick bond ----------------------------------------------------------------------------------------------------------------
def brick_lattice(nx=6, ny=6, nz=4, x_gap=True, z_gap=True):
    """Unit boxes, every other layer shifted by half a box in x and y, so that a box rests on a quarter of each of four boxes
    below (within a layer boxes share whole faces, which the rule does not join).  Gaps: the boxes of the upper half of x moved
    4 away, the upper half of the layers lifted by a half.  -> pieces, (i, j, k) of each, island of each."""
    pieces, ijk, block = [], [], []
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                far, high = x_gap and i >= nx // 2, z_gap and k >= nz // 2
                x, y, z = i + .5 * (k % 2) + (4 if far else 0), j + .5 * (k % 2), k + (.5 if high else 0)
                pieces.append(B((x, y, z), (x + 1, y + 1, z + 1)))
                ijk.append((i, j, k))
                block.append(2 * int(far) + int(high))
    return pieces, ijk, block


def check_brick_bond(engine_mod, oracle):
    pieces, ijk, block = brick_lattice()
    n = len(pieces)
    assert n == 144
    # one cell: the four islands the gaps leave
    got, info, _ = four_ways(engine_mod, oracle, pieces, np.zeros(n, np.int32))
    assert got == expected_from_blocks([0] * n, block) and len(got) == 1 + 4
    # slabs of two rows as cells: boxes of the shifted layers rest on rows of the next slab (contact across cells, which must not
    # join anything), so every slab falls into its own four islands
    for run_order in ([0, 1, 2], [2, 0, 1]):
        rng = np.random.RandomState(5)
        order = []
        for c in run_order:
            mine = [p for p in range(n) if ijk[p][1] // 2 == c]
            order += [mine[q] for q in rng.permutation(len(mine))]
        ps, cells, bl = [pieces[p] for p in order], [ijk[p][1] // 2 for p in order], [(ijk[p][1] // 2, block[p]) for p in order]
        got, info, _ = four_ways(engine_mod, oracle, ps, cells)
        assert got == expected_from_blocks(cells, bl) and len(got) == 1 + 12
    # without cells the same contacts do join: the set of a face is what keeps them apart
    got, _, _ = four_ways(engine_mod, oracle, *[brick_lattice(x_gap=False, z_gap=False)[0], np.zeros(n, np.int32)])
    assert got == [[], list(range(n))]


# ---- chains --------------------------------------------------------------------------------------------------------------------
def chain(n, at=(0.0, 0.0, 0.0)):
    """Box t rests on a quarter of box t - 1 (up and down in turn): t touches t - 1 and t + 1 and nothing else."""
    return [B((at[0] + .5 * t, at[1] + .5 * (t % 2), at[2] + (t % 2)), (at[0] + .5 * t + 1, at[1] + .5 * (t % 2) + 1, at[2] + (t % 2) + 1)) for t in range(n)]


def check_long_chain(engine_mod, oracle, n):
    links = chain(n)
    numberings = {"along": np.arange(n), "against": np.arange(n)[::-1], "random": np.random.RandomState(11).permutation(n)}
    for name, where in numberings.items():            # piece p is link where[p]
        pieces = [links[t] for t in where]
        got, info, stats = four_ways(engine_mod, oracle, pieces, np.zeros(n, np.int32))
        assert got == [[], list(range(n))], name
        assert stats["edges"] == n - 1 and 2 <= stats["rounds"] < n + 8, (name, stats)
        if name == "against":
            # Piece p's neighbours are p - 1 and p + 1.  With every thread in step, after round r every label is max(p - o_r, 0)
            # with o_1 = 2 (the sweep takes p - 1, the jump p - 2) and o_r = 2 (o_(r-1) + 1): the sweep takes the neighbour's
            # label, the jump doubles the reach.  Labels only ever decrease and that state is monotone in p, so a thread
            # that reads a newer label only gets there sooner.  o_r >= 2^r: ceil(log2 n) rounds and the one that changes
            # nothing.  Without the jump the same chain takes a round per piece.
            assert stats["rounds"] <= int(np.ceil(np.log2(n))) + 1, stats
        cut = n // 2 + 3                               # one brick removed: two chains
        keep = [p for p in range(n) if where[p] != cut]
        got, info, stats = four_ways(engine_mod, oracle, [pieces[p] for p in keep], np.zeros(n - 1, np.int32))
        side = [int(where[p] > cut) for p in keep]
        assert got == expected_from_blocks([0] * (n - 1), side) and len(got) == 3, name
        assert stats["edges"] == n - 3 and 2 <= stats["rounds"] < n + 7, (name, stats)


def check_many_short_chains(engine_mod, oracle):
    pieces, cells, block = [], [], []
    for c in range(300):
        links = chain(5, at=(0.0, 4.0 * c, 0.0))
        if c % 7 == 3:                                 # the middle box lifted off: [0, 1], [2], [3, 4]
            links[2] = R.moved(links[2], shift=(0, 0, 8))
        pieces += links
        cells += [c] * 5
        block += [0, 0, 1, 2, 2] if c % 7 == 3 else [0] * 5
    got, info, stats = four_ways(engine_mod, oracle, pieces, cells)
    assert got == expected_from_blocks(cells, block) and len(got) == 1 + 300 + 2 * 43
    assert stats["edges"] == 4 * 300 - 2 * 43 and stats["rounds"] >= 2


# ---- wide windows --------------------------------------------------------------------------------------------------------------
def check_flat_layer(engine_mod, oracle):
    """40 x 40 boxes side by side: 1600 faces share every |d| with equal or opposite normals, and none touches (whole faces)."""
    pieces = [B((i, j, 0), (i + 1, j + 1, 1)) for j in range(1, 41) for i in range(1, 41)]
    got, info, stats = four_ways(engine_mod, oracle, pieces, np.zeros(1600, np.int32))
    assert got == [[]] + [[p] for p in range(1600)] and stats["edges"] == 0


def check_slab_with_many_boxes(engine_mod, oracle):
    """One face with 256 partners."""
    pieces = [B((0, 0, 0), (32, 32, 1))] + [B((2 * i + .5, 2 * j + .5, 1), (2 * i + 1.5, 2 * j + 1.5, 2)) for j in range(16) for i in range(16)]
    got, info, stats = four_ways(engine_mod, oracle, pieces, np.zeros(257, np.int32))
    assert got == [[], list(range(257))] and stats["edges"] == 256


# ---- limits --------------------------------------------------------------------------------------------------------------------
def check_limit_half_edges(engine_mod, oracle):
    """RG_MAXH = 4096 half-edges of one Convex: a prism of 682 sides (4092) is regrouped, one of 700 (4200) is refused with
    SURTR_E_CAPACITY -- the host version has no such limit -- and the context then serves a small scene."""
    rest = [B((-.25, -.25, 1), (.25, .25, 2)), B((3, 3, 0), (4, 4, 1))]
    eng = engine_mod.Engine(0)
    big = R.prism(682)
    assert big["nbr"].shape[0] == 4092
    got, info, stats = four_ways(engine_mod, oracle, [big] + rest, [0, 0, 0], exact=False, eng=eng)
    assert got == [[], [0, 1], [2]]
    too_big = R.prism(700)
    assert too_big["nbr"].shape[0] == 4200
    load(eng, [too_big] + rest, [0, 0, 0])
    with pytest.raises(engine_mod.SurtrError) as e:
        eng.event_regroup()
    assert e.value.code == engine_mod.E_CAPACITY
    ho, hp = engine_mod.regroup([too_big] + rest, np.zeros(3, np.int32))
    ro, rp, _ = R.regroup([too_big] + rest, np.zeros(3, np.int32))
    assert _lists(ho, hp) == _lists(ro, rp) == [[], [0, 1], [2]]
    got, _, _ = four_ways(engine_mod, oracle, *[PREDICATE_EDGES["half_staggered"][0], [0, 0]], eng=eng)
    assert got == JOINED
    eng.close()


def check_limit_edges_of_a_stack_of_thin_plates(engine_mod, oracle):
    """cap_edges = 16 * faces + 1024 pairs of touching faces.  400 plates 2^-18 thick, every other one shifted by half: each
    large face has up to 262 partners within the 1e-3 window (the rule compares |d|, not contact).  The device step answers
    SURTR_E_CAPACITY, having counted exactly the pairs the reference finds; host and oracle have no such limit."""
    t = 2.0 ** -18
    pieces = [B((k * t, .5 * (k % 2), .5 * (k % 2)), ((k + 1) * t, .5 * (k % 2) + 1, .5 * (k % 2) + 1)) for k in range(400)]
    cells = np.zeros(400, np.int32)
    ro, rp, info = R.regroup(pieces, cells)
    assert_robust(pieces, info, True)
    assert _lists(ro, rp) == [[], list(range(400))]
    ho, hp = engine_mod.regroup(pieces, cells)
    oo, op = oracle.regroup(pieces, cells)
    assert _lists(ho, hp) == _lists(oo, op) == _lists(ro, rp)
    eng = engine_mod.Engine(0)
    load(eng, pieces, cells)
    with pytest.raises(engine_mod.SurtrError) as e:
        eng.event_regroup()
    stats = eng.regroup_stats()
    assert e.value.code == engine_mod.E_CAPACITY
    assert stats["edges"] == info["touching_face_pairs"] > stats["cap_edges"] == 16 * 2400 + 1024
    got, _, _ = four_ways(engine_mod, oracle, *[PREDICATE_EDGES["half_staggered"][0], [0, 0]], eng=eng)
    assert got == JOINED
    eng.close()


# ---- the impact sphere ---------------------------------------------------------------------------------------------------------
ORIGIN = np.float32([2, 1, 0])
TARGET = 5 * 6 + 5          # box (5, 5, 0) of the lattice: its nearest vertex (5, 5, 0) is at (3, 4, 0) from ORIGIN, 5 exactly
ON_FACE = np.float32([5, 5.5, .5])          # on the plane x = 5 of that box (and inside no other box that is out of the sphere)


def sphere_lattice():
    pieces, ijk, _ = brick_lattice(x_gap=False, z_gap=False)
    cells = [j // 2 for (_, j, _) in ijk]
    order = sorted(range(len(pieces)), key=lambda p: (cells[p], p))
    return [pieces[p] for p in order], [cells[p] for p in order], order.index(TARGET)


def cloud_of(n, where):
    """n points far below the lattice, with ON_FACE first, last or absent."""
    far = np.float32([[(q % 64) / 8.0, q // 64, -8.0] for q in range(n)]).reshape(-1, 3)
    if n and where == "first":
        far[0] = ON_FACE
    if n and where == "last":
        far[n - 1] = ON_FACE
    return far


def check_sphere(engine_mod, oracle):
    pieces, cells, target = sphere_lattice()
    n = len(pieces)
    eng = engine_mod.Engine(0)
    out_without = None
    for ns in (0, 1, 63, 64, 65, 257, 1000):
        for where in ("first", "last", "absent") if ns > 1 else ("first", "absent") if ns else ("absent",):
            cloud = cloud_of(ns, where)
            got, info, stats = four_ways(engine_mod, oracle, pieces, cells, eng=eng, partial=True, sphere_points=cloud, origin=ORIGIN, radius=5.0)
            m = info["margins"]
            assert m.zeros["vertex"] > 0 and (where == "absent" or m.zeros["cloud"] > 0)       # a vertex at the radius, a point on a plane
            # the strict `< radius` keeps the target's vertex out of the sphere, so only the cloud point can hold the box back
            assert (target in info["out_pieces"]) == (where == "absent"), (ns, where)
            if where == "absent":
                out_without = out_without or info["out_of_sphere"]
                assert info["out_of_sphere"] == out_without and 0 < out_without < n
            else:
                assert info["out_of_sphere"] == out_without - 1
    # every fragment in the sphere / none of them: compounds untouched / all emptied and erased, bind 0 falls into its islands
    got, info, _ = four_ways(engine_mod, oracle, pieces, cells, eng=eng, partial=True, sphere_points=cloud_of(65, "absent"), origin=ORIGIN, radius=64.0)
    assert info["out_of_sphere"] == 0 and got[0] == [] and len(got) == 1 + 3
    got, info, _ = four_ways(engine_mod, oracle, pieces, cells, eng=eng, partial=True, sphere_points=cloud_of(65, "absent"),
                             origin=np.float32([-16, -16, -16]), radius=1.0)
    assert info["out_of_sphere"] == n and got == [list(range(n))]       # (the lattice without gaps or cells is one island)
    eng.close()


# ---- pieces the event kept out, and what is left of a mask afterwards ---------------------------------------------------------
def _two_cubes_event(engine_mod, outside):
    sc = scenes.cube_scene(n_cells=8)
    eng = engine_mod.Engine(0)
    eng.upload_pieces([sc["mesh"], sc["mesh"]], [sc["convex"], sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    c = eng.fracture_event(0, sc["n_cells"], outside=np.asarray(outside, np.uint8), flags=0)
    return eng, c


def check_event_that_keeps_every_piece_out(engine_mod, oracle):
    """A real event whose mask keeps every piece: no fragment at all, the resident pieces alone are regrouped (from the CSR
    copies of the pieces, not from the arena)."""
    pieces, _, block = brick_lattice()
    sc = scenes.cube_scene(n_cells=8)
    eng = engine_mod.Engine(0)
    eng.upload_pieces(pieces, pieces)
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    c = eng.fracture_event(0, sc["n_cells"], outside=np.ones(len(pieces), np.uint8), flags=0)
    assert c.n_frag == 0
    n = len(pieces)
    for sphere in ({}, {"partial": True, "sphere_points": cloud_of(65, "absent"), "origin": ORIGIN, "radius": 5.0}):
        do, dp = eng.event_regroup(**sphere)
        ref_kw = {("cloud" if k == "sphere_points" else k): v for k, v in sphere.items()}
        ro, rp, info = R.regroup(pieces, np.zeros(n, np.int32), n_outside=n, **ref_kw)
        assert_robust(pieces, info, True)
        ho, hp = engine_mod.regroup(pieces, np.full(n, -1, np.int32), n_outside=n, **sphere)
        oo, op = oracle.regroup(pieces, np.full(n, -1, np.int32), n_outside=n, **sphere)
        assert _lists(do, dp) == _lists(ho, hp) == _lists(oo, op) == _lists(ro, rp) == expected_from_blocks([0] * n, block)[1:]
        assert eng.regroup_stats()["edges"] == info["touching_face_pairs"]
    eng.close()


def check_mask_does_not_outlive_its_event(engine_mod, oracle):
    """include/surtr_hip.h, surtr_event_regroup, State.  In both sequences the resident piece count equals the length of the mask,
    which is all the earlier guard looked at."""
    pair = PREDICATE_EDGES["half_staggered"][0]
    # (1) fragments loaded from the host are nobody's event: the mask is dropped
    eng, c = _two_cubes_event(engine_mod, [1, 0])
    assert c.n_frag >= 2
    got, _, _ = four_ways(engine_mod, oracle, pair, [0, 0], eng=eng)
    assert got == JOINED
    eng.close()
    # (2) the event's fragments replace the pieces: the piece the mask kept out is gone, its compounds cannot be formed
    eng, c = _two_cubes_event(engine_mod, [1, 0])
    do, dp = eng.event_regroup()
    assert dp.shape[0] == c.n_frag + 1 and 0 in _lists(do, dp)[0]           # before: piece 0, then the fragments
    keep = np.zeros(c.n_frag, np.uint8)
    keep[:2] = 1
    assert eng.pieces_from_event(keep) == 2
    with pytest.raises(engine_mod.SurtrError) as e:
        eng.event_regroup()
    assert e.value.code == engine_mod.E_STATE
    eng.close()
    # ... while a mask that kept nothing out needs no piece
    eng, c = _two_cubes_event(engine_mod, [0, 0])
    before = eng.event_regroup()
    keep = np.zeros(c.n_frag, np.uint8)
    keep[:2] = 1
    assert eng.pieces_from_event(keep) == 2
    after = eng.event_regroup()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    eng.close()


def check_stats_start_from_zero(engine_mod, oracle):
    eng = engine_mod.Engine(0)
    assert set(eng.regroup_stats().values()) == {0}
    eng.close()


CPU_CHAIN, GPU_CHAIN = 1500, 1500
FAMILIES = {
    "predicate_edges": check_predicate_edges,
    "walk_returns_the_builders_loops": check_walk_returns_the_builders_loops,
    "brick_bond": check_brick_bond,
    "many_short_chains": check_many_short_chains,
    "flat_layer": check_flat_layer,
    "slab_with_many_boxes": check_slab_with_many_boxes,
    "limit_half_edges": check_limit_half_edges,
    "limit_edges_of_a_stack_of_thin_plates": check_limit_edges_of_a_stack_of_thin_plates,
    "sphere": check_sphere,
    "event_that_keeps_every_piece_out": check_event_that_keeps_every_piece_out,
    "mask_does_not_outlive_its_event": check_mask_does_not_outlive_its_event,
    "stats_start_from_zero": check_stats_start_from_zero,
}


def _cpu(check):
    def test(emul_engine, oracle):
        check(emul_engine, oracle)
    return test


def _gpu(check):
    @pytest.mark.gpu
    def test(gpu_engine, oracle):
        check(gpu_engine, oracle)
    return test


for _name, _check in FAMILIES.items():
    globals()["test_" + _name] = _cpu(_check)
    globals()["test_gpu_" + _name] = _gpu(_check)


def test_long_chain(emul_engine, oracle):
    check_long_chain(emul_engine, oracle, CPU_CHAIN)


@pytest.mark.gpu
def test_gpu_long_chain(gpu_engine, oracle):
    """More pieces than the 1024 threads of k_rg_labels_all, numbered along the chain, against it and at random: the only check
    of that kernel's races (the emulation runs it with one thread)."""
    check_long_chain(gpu_engine, oracle, GPU_CHAIN)
