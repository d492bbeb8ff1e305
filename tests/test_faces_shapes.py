"""k_faces (face extraction, the four ear clippers, the fan, the per-face compaction) on designed faces of every size, against
tests/faces_ref.py: the ear-clipping rule restated in np.float32 (bit for bit), and in float64 what a valid ear clipping is.

Per solid (check_solid): (a) extract_faces returns the designed loops up to rotation and exactly the oracle's; (b) the indices of
triangulate(is_convex=False) equal oracle.render's and, face by face, ear_clip_f32's; (c) replay_check passes on every face that did
not stall; (d) a stalled face has no triangles and the other faces of its solid are untouched; (e) on convex solids is_convex=True
gives the fan (f0, fv, fv+1); (f) vnc is position, zero normal, colour.  Before the engine is asked, conditions() asserts from the
reference alone that the case is what it was designed to be (margins, refusals, stalls, the pinch).

Which clipper a face reaches on the GPU is decided by its length: 3..4 ear_clip_small, 5..64 ear_clip_face_wave, 65..256
ear_clip_face_wave_k<4>, above 256 the serial ear_clip_face.  On the emulation 3..8 go to ear_clip_small and everything longer to
ear_clip_face.  Which route the face search takes is decided by the fragment: ROUTES names the solid on each side of each limit.

A pinched loop (two vertices at one position) gets, by counting alone, two triangles of no area -- one per lobe, each holding both
carriers: that is what all three implementations write, and replay_check is told which pair it is and demands
exactly that.

The CPU tier runs on the emulation library (conftest's emul_engine).  The GPU tier runs the same lists on the MI355X in three child
processes under a time limit (helpers.run_gpu_child); the children import the lists from this module."""
import functools
import textwrap

import numpy as np
import pytest

import faces_ref as R
from helpers import run_gpu_child

SIZES = (4, 5, 8, 9, 63, 64, 65, 66, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 300, 600)
FAMILIES = {"regular": R.regular, "star": R.star, "spiral": R.spiral, "collinear": R.collinear, "pinched": R.pinched}
COLOUR = (0.5, 0.25, 0.125)
FL_V, FL_H, FL_J = 1024, 4096, 2048           # k_faces: LDS topology up to FL_V vertices and FL_H half-edges, jumps and ear staging up to FL_J


def rotations(n):
    return (0, 1, 63, 64, n - 1) if n >= 64 else (0,)


def _shape_groups():
    g = {}
    for n in SIZES:
        g["regular-%d" % n] = ["regular-%d-r%d" % (n, r) for r in rotations(n)]
        if n % 2 == 0 and n >= 8:             # (a "star" of four corners is a rhombus)
            g["star-%d" % n] = ["star-%d-r%d" % (n, r) for r in rotations(n)]
        if n >= 8:
            g["spiral-%d" % n] = ["spiral-%d-r%d" % (n, r) for r in rotations(n)]
    for n in (5, 9, 65, 257):                 # one per clipper: small, wave (serial on the emulation), four per lane, serial
        g["collinear-%d" % n] = ["collinear-%d-r0" % n]
    for n in (8, 12, 70, 260):
        g["pinched-%d" % n] = ["pinched-%d-r0" % n]
    return g


SHAPE_GROUPS = _shape_groups()
SHAPES = [c for g in SHAPE_GROUPS.values() for c in g]


def _prisms(*polys):
    return R.union([R.prism_over(p) for p in polys])


# name -> (builder, vertices, half-edges, what it reaches).  lensum, the loop entries of a regular fragment, equals its half-edges.
ROUTES = {
    "pyramid-512": (lambda: R.pyramid_over(R.regular(512)), 513, 2048, "pointer jumping in LDS, ear staging in LDS: H = FL_J"),
    "roof-512": (lambda: R.roof_over(R.regular(512), 256), 514, 2050, "LDS topology without jumps, loops from global memory: H = FL_J + 2"),
    "prisms-341": (lambda: _prisms(R.star(64), R.spiral(200), R.regular(77)), 682, 2046,
                   "as pyramid-512, with non-convex faces: the one-per-lane wave clipper reads 16-bit loops from LDS"),
    "prisms-342": (lambda: _prisms(R.star(64), R.spiral(200), R.regular(78)), 684, 2052,
                   "as roof-512, with non-convex faces: the one-per-lane wave clipper reads 32-bit loops from global memory"),
    "pyramid-1023-cut": (lambda: R.pyramid_over(R.regular(1023), diagonals=((0, 341), (341, 682))), 1024, 4096,
                         "LDS topology without jumps at both limits: n = FL_V, H = FL_H"),
    "bipyramid-683": (lambda: R.bipyramid_over(R.regular(683)), 685, 4098, "global route by half-edges: H = FL_H + 2, n <= FL_V"),
    "pyramid-1024": (lambda: R.pyramid_over(R.regular(1024)), 1025, 4096, "global route by vertices: n = FL_V + 1, H = FL_H"),
    "polytope-130": (lambda: R.tangent_polytope(130), 256, 768, "three ballots of faces, all staged in LDS"),
    "polytope-400": (lambda: R.tangent_polytope(400), 796, 2388, "seven ballots of faces on the LDS topology, loops from global memory"),
    "polytope-700": (lambda: R.tangent_polytope(700), 1396, 4188, "eleven ballots of faces on the global route"),
    "union": (lambda: R.union([R.prism_over(R.star(64)), R.prism_over(R.spiral(200)), R.tangent_polytope(700), R.prism_over(R.star(258))]),
              2440, 7320, "non-convex faces of every clipper on the global route"),
}
CONVEX = ("regular", "pyramid", "roof", "bipyramid", "polytope")
BATCH = [c for c in SHAPES if int(c.split("-")[1]) <= 70 and c.endswith("-r0")] + ["union"]


def family(name):
    return name.split("-")[0]


@functools.lru_cache(maxsize=None)
def build(name):
    if name in ROUTES:
        s = ROUTES[name][0]()
        assert (s["pos"].shape[0], s["nbr"].shape[0]) == ROUTES[name][1:3], (name, s["pos"].shape[0], s["nbr"].shape[0])
        return s
    fam, n, r = name.split("-")
    return R.prism_over(R.rotated(FAMILIES[fam](int(n)), int(r[1:])))


def twins_of(name, loop):
    """The pairs of vertices of this loop that carry one position (only the caps of a pinched prism have one)."""
    if family(name) != "pinched" or len(loop) != int(name.split("-")[1]):
        return ()
    lo = min(loop)
    return ((lo, lo + len(loop) // 2),)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Per designed face (as a loop started at its lowest vertex): its triangles, counters and margin; computed once per case."""
    s = build(name)
    out = {}
    for f in s["faces"]:
        loop = R.canonical(f)
        m = R._Margin()
        tris, info = R.ear_clip_f32(s["pos"], loop, m)
        out[loop] = {"tris": np.asarray(tris, np.uint32).reshape(-1), "info": info, "ratio": m.ratio, "zeros": m.zeros, "count": m.count}
    return out


def summary(name):
    """Counters of the case, over its faces."""
    ref = reference(name)
    key = ("ears", "refused_reflex", "refused_inside", "cleared", "same_position")
    tot = {k: sum(v["info"][k] for v in ref.values()) for k in key}
    tot["stalled"] = sum(v["info"]["stalled"] for v in ref.values())
    tot["ratio"] = min(v["ratio"] for v in ref.values())
    tot["zeros"] = sum(v["zeros"] for v in ref.values())
    return tot


def conditions(name):
    """What the case was designed to be, asserted from the reference alone."""
    ref, fam, tot = reference(name), family(name), summary(name)
    if fam in ("collinear", "pinched"):
        n = int(name.split("-")[1])
        caps = [v for k, v in ref.items() if len(k) == n]
        walls = [v for k, v in ref.items() if len(k) != n]
        assert len(caps) == 2 and len(walls) == n
        assert all(v["ratio"] >= 1 and v["zeros"] == 0 and not v["info"]["stalled"] for v in walls), name
        for v in caps:
            i = v["info"]
            if fam == "collinear":      # every value exactly 0, nothing is an ear: the face is given up after n + 1 candidates
                assert i["stalled"] and i["ears"] == 0 and i["refused_reflex"] == n + 1 and v["zeros"] == v["count"] and v["tris"].size == 0, name
            else:                       # the skip was taken, nothing stalled, and whatever is not exactly 0 is decided
                assert i["same_position"] >= 1 and not i["stalled"] and v["ratio"] >= 1 and v["tris"].size == 3 * (n - 2), name
        return
    assert tot["ratio"] >= 1 and tot["zeros"] == 0 and tot["stalled"] == 0, (name, tot)
    if fam in ("star", "spiral") or name in ("prisms-341", "prisms-342", "union"):
        assert tot["refused_inside"] >= 1 and tot["cleared"] >= 1, (name, tot)


def fan_of(loops):
    out = []
    for lp in loops:
        for v in range(1, len(lp) - 1):
            out += [lp[0], lp[v], lp[v + 1]]
    return np.asarray(out, np.uint32)


def expected(name, loops):
    """(per-face triangles, flat) for the loops as the engine returned them."""
    s, ref = build(name), reference(name)
    per = []
    for lp in loops:
        key = tuple(int(v) for v in lp)
        if key in ref:
            per.append(ref[key]["tris"])
        else:           # the same face started elsewhere: the rule depends on the start
            assert R.canonical(key) in ref, ("a loop that was not designed", name, key[:8])
            per.append(np.asarray(R.ear_clip_f32(s["pos"], key)[0], np.uint32).reshape(-1))
    return per


def check_solid(eng, oracle, name):
    conditions(name)
    s, ref = build(name), reference(name)
    # (a) the loops
    fo, fi = eng.extract_faces(s)
    ofo, ofi = oracle.extract_faces(s)
    assert np.array_equal(fo, ofo) and np.array_equal(fi, ofi), ("loops differ from the oracle's", name)
    loops = [tuple(int(v) for v in fi[fo[k]:fo[k + 1]]) for k in range(fo.shape[0] - 1)]
    assert sorted(R.canonical(lp) for lp in loops) == sorted(ref), ("loops differ from the designed ones", name)
    # (b) the indices, (d) stalled faces
    vnc, idx = eng.triangulate(s, is_convex=False, color=COLOUR)
    ovnc, oidx = oracle.render(s, convex=False, colour=COLOUR)
    per = expected(name, loops)
    at = 0
    for k, want in enumerate(per):
        got = idx[at:at + want.size]
        assert np.array_equal(got, want), ("face differs from ear_clip_f32", name, k, len(loops[k]), got[:12], want[:12])
        at += want.size
    assert at == idx.size, ("more indices than the faces account for", name, at, idx.size)
    assert np.array_equal(idx, oidx), ("indices differ from the oracle's", name)
    # (c) validity
    pos64 = s["pos"].astype(np.float64)
    whole = True
    for lp, tris in zip(loops, per):
        if tris.size == 0 and len(lp) > 2:
            assert ref[R.canonical(lp)]["info"]["stalled"], (name, "no triangles on a face that did not stall")
            whole = False
            continue
        R.replay_check(pos64, lp, tris.reshape(-1, 3), coincident=twins_of(name, lp))
    if whole and family(name) != "pinched":
        assert R.edges_paired(idx), ("triangle edges do not pair up over the solid", name)
    # (f) vnc
    assert vnc.shape == (s["pos"].shape[0], 9)
    assert np.array_equal(vnc[:, :3], s["pos"]) and not vnc[:, 3:6].any() and np.array_equal(vnc[:, 6:], np.tile(np.asarray(COLOUR, np.float32), (vnc.shape[0], 1))), name
    assert np.array_equal(vnc, ovnc), name
    # (e) the fan
    if family(name) in CONVEX:
        fv, fidx = eng.triangulate(s, is_convex=True, color=COLOUR)
        assert np.array_equal(fidx, fan_of(loops)), ("fan", name)
        assert np.array_equal(fidx, oracle.render(s, convex=True, colour=COLOUR)[1]), ("fan differs from the oracle's", name)
        assert np.array_equal(fv, vnc), name
    return idx, vnc


def run_cases(E, oracle, names):
    eng = E.Engine(0)
    try:
        for name in names:
            check_solid(eng, oracle, name)
    finally:
        eng.close()


def run_batch(E, oracle):
    """All small cases and the union as the fragments of one event: per fragment the single-solid answer, in place."""
    solids = [build(c) for c in BATCH]
    solo, eng = E.Engine(0), E.Engine(0)
    try:
        want = [solo.triangulate(s, is_convex=False) for s in solids]
        eng.load_fragments(solids, solids)
        eng.event_triangulate(False)
        ev = eng.download()
        c = eng.event_counts()
        assert c.status == 0 and c.n_frag == len(solids)
        assert c.n_idx == sum(w[1].size for w in want) == ev["idx"].size and ev["idx_off"][-1] == c.n_idx
        assert c.mesh_verts == sum(s["pos"].shape[0] for s in solids) == ev["vnc"].shape[0]
        sizes = []
        for k, (name, s) in enumerate(zip(BATCH, solids)):
            a, b = int(ev["idx_off"][k]), int(ev["idx_off"][k + 1])
            per = expected(name, [lp for lp in _loops_of(solo, s)])
            assert np.array_equal(ev["idx"][a:b], np.concatenate(per)), ("fragment differs from ear_clip_f32", name)
            assert np.array_equal(ev["idx"][a:b], want[k][1]), ("fragment differs from the single solid", name)
            va, vb = int(ev["mesh_vert_off"][k]), int(ev["mesh_vert_off"][k + 1])
            assert np.array_equal(ev["vnc"][va:vb, :3], s["pos"]) and np.array_equal(ev["vnc"][va:vb], want[k][0]), name
            sizes.append(b - a)
        assert min(sizes) == 30 and max(sizes) > 14000            # from ten triangles to thousands in one event
    finally:
        solo.close(); eng.close()


def _loops_of(eng, s):
    fo, fi = eng.extract_faces(s)
    return [tuple(int(v) for v in fi[fo[k]:fo[k + 1]]) for k in range(fo.shape[0] - 1)]


# ------------------------------------------------------------------ the designed inputs themselves (no engine)
def test_builders_make_what_they_promise():
    for n in (8, 64, 66, 258, 600):
        assert R.is_simple(R.star(n)) and R.is_simple(R.spiral(n)) and R.is_simple(R.regular(n))
    p = R.pinched(12)
    assert np.array_equal(p[0], p[6]) and np.unique(p, axis=0).shape[0] == 11
    assert np.array_equal(R.rotated(R.star(64), 63)[1], R.star(64)[0])
    for name, (_, n, h, _) in ROUTES.items():
        s = build(name)
        loops = [len(f) for f in s["faces"]]
        assert s["pos"].dtype == np.float32 and sum(loops) == h == s["nbr"].shape[0] and s["pos"].shape[0] == n
        islands = 4 if name == "union" else 3 if name.startswith("prisms") else 1
        assert s["pos"].shape[0] - h // 2 + len(loops) == 2 * islands, name      # Euler, per island
    # one solid on each side of each limit of k_faces
    side = {k: (v[1] <= FL_V, v[2] <= FL_J, v[2] <= FL_H) for k, v in ROUTES.items()}
    assert side["pyramid-512"] == (True, True, True) and ROUTES["pyramid-512"][2] == FL_J
    assert side["roof-512"] == (True, False, True) and ROUTES["roof-512"][2] == FL_J + 2
    assert side["pyramid-1023-cut"] == (True, False, True) and ROUTES["pyramid-1023-cut"][1:3] == (FL_V, FL_H)
    assert side["bipyramid-683"] == (True, False, False) and ROUTES["bipyramid-683"][2] == FL_H + 2
    assert side["pyramid-1024"] == (False, False, True) and ROUTES["pyramid-1024"][1] == FL_V + 1
    for name, faces in (("polytope-130", 130), ("polytope-400", 400), ("polytope-700", 700)):
        sizes = [len(f) for f in build(name)["faces"]]
        assert len(sizes) == faces and sum(5 <= k <= 7 for k in sizes) > 64 and max(sizes) <= 8, name


def test_replay_check_refuses_what_is_no_ear_clipping():
    """The definition has teeth: a fan over a star, a triangle left out, a triangle turned round are all refused."""
    s = build("star-64-r0")
    loop = R.canonical(s["faces"][1])
    pos64 = s["pos"].astype(np.float64)
    good = reference("star-64-r0")[loop]["tris"].reshape(-1, 3)
    R.replay_check(pos64, loop, good)
    for why, bad in (("a fan", fan_of([loop]).reshape(-1, 3)), ("one short", good[:-1]), ("turned round", np.concatenate([good[:5], good[5:6, ::-1], good[6:]])),
                     ("one twice", np.concatenate([good[:1], good[:-1]]))):
        with pytest.raises(AssertionError):
            R.replay_check(pos64, loop, bad)
            print("accepted:", why)
    # an ear that holds a vertex: corner 0 of a square with a dent that reaches into it
    dent = np.array([(0, 0, 0), (4, 0, 0), (4, 4, 0), (2, 0.5, 0), (0, 4, 0)], np.float64)
    R.replay_check(dent, range(5), [(3, 4, 0), (1, 2, 3), (0, 1, 3)])
    with pytest.raises(AssertionError, match="vertex inside"):
        R.replay_check(dent, range(5), [(4, 0, 1), (1, 2, 3), (4, 1, 3)])


def test_slot_coverage_of_the_four_per_lane_faces():
    """Together the faces of 65 .. 256 vertices hold a refusal decided by a reflex vertex of each of the four slots (loop index //
    64), and clipped ears whose prv and cur, and cur and nxt, lie in different slots."""
    infos = [v["info"] for c in SHAPES if family(c) in ("star", "spiral") and 65 <= int(c.split("-")[1]) <= 256 for v in reference(c).values()]
    slots, pc, cn = R.slot_coverage(infos)
    assert slots == {0, 1, 2, 3} and pc and cn, (slots, pc, cn)


# ------------------------------------------------------------------ CPU tier (emulation)
@pytest.mark.parametrize("group", list(SHAPE_GROUPS))
def test_shapes(emul_engine, oracle, group):
    run_cases(emul_engine, oracle, SHAPE_GROUPS[group])


@pytest.mark.parametrize("name", list(ROUTES))
def test_fragment_routes(emul_engine, oracle, name):
    run_cases(emul_engine, oracle, [name])


@pytest.mark.parametrize("tier", [None, 256])
def test_batch(emul_engine, oracle, monkeypatch, tier):
    """tier: every fragment above 256 half-edges goes to the second launch of k_faces, as in test_faces_second_tier_and_workgroup_budget."""
    if tier is not None:
        monkeypatch.setenv("SURTR_FACES_TIER_HE", str(tier))
    run_batch(emul_engine, oracle)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys, time
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    from surtr_amd import engine
    from oracle import oracle as O
    import test_faces_shapes as T
    case = sys.argv[1]
    O.lib()
    t0 = time.time()
    if case == "shapes":
        T.run_cases(engine, O, T.SHAPES)
    elif case == "routes":
        T.run_cases(engine, O, list(T.ROUTES))
    elif case == "batch":
        T.run_batch(engine, O)
    print("seconds %%.1f" %% (time.time() - t0))
    print("ok", case)
""")


@pytest.mark.gpu
def test_gpu_shapes():
    run_gpu_child(GPU_CHILD, "shapes", 240)


@pytest.mark.gpu
def test_gpu_fragment_routes():
    run_gpu_child(GPU_CHILD, "routes", 120)


@pytest.mark.gpu
def test_gpu_batch():
    run_gpu_child(GPU_CHILD, "batch", 120)
