"""The fan finish of the four ear clippers and the triangles written straight into the index arena (k_faces).

Once a face has no reflex corner left the clippers write the remaining triangles in closed form, (prv[cur], v, nxt[v]) along the
ring; the output must be the sequential rule's, bit for bit and in its order.  Prisms over designed polygons, numbered from corners
0, 1 and n - 1, and from 63 and 64 where n allows (rotations):

  convex     regular n-gons at the boundaries of the clippers and of the slots of the four-per-lane one: the fan is taken before
             the first iteration;
  dent       a regular n-gon with ONE corner c pulled inside the chord of its neighbours, but not inside the chord (c - 2, c + 1):
             the first ear clipped next to it makes it convex, and the rest of the face is the fan.  c = 0 (refused first, cleared by
             the ear at 1, the ring of the fan wraps round to 0), c = 1 (cleared by the first ear), c = 64 (cleared by the ear at 63,
             the fan starts at cur = 64, in the second slot) and c = n - 1 (cleared as prv of the first ear).  With one reflex corner
             on a regular polygon the ears are clipped in index order, so cur cannot come back to 0 or reach n - 1 before three
             corners are left: those two switches exist only as the positions of the dent.  (A fan that starts after cur has gone
             round, with alive corners of lower index that still get a triangle, takes corners that were refused in the same round for
             a reflex corner which was cleared in that round with many corners left.  No star or spiral here at 12 .. 260 corners in
             eight numberings does it, nor polygons with two dents or with spikes into the ears of large corners, which clear only
             when three or four corners are left: the designed cases do not reach that branch of the wave clippers.)
  star, spiral   reflex corners are cleared one by one until late in the face: the fan must not be taken while one is left;
  collinear  both caps stall (the first and the last face of the prism): no triangles, the other faces in place;
  pinched    two triangles of no area.

Every solid is checked against oracle.extract_faces / oracle.render bit for bit, face by face against faces_ref.ear_clip_f32, and
with faces_ref.replay_check.  One batch event of these solids checks idx_off, idx_n, n_idx and the packed arrays, with stalled
faces first, last, first and last, and between normal faces of a fragment, and a fragment of triangles and quads only; on the emulation also with
the second tier of k_faces forced.  The emulation runs ear_clip_small (3..8 corners) and ear_clip_face; the wave clippers run in the
GPU tier (5..64 one corner per lane, 65..256 four per lane)."""
import functools
import textwrap

import numpy as np
import pytest

import faces_ref as R
from helpers import run_gpu_child

COLOUR = (0.5, 0.25, 0.125)
CONVEX_N = (4, 5, 8, 9, 63, 64, 65, 66, 128, 129, 192, 256, 257)
DENT_N = (6, 9, 64, 65, 130, 257)
LATE_N = (8, 12, 66, 260)
DEGENERATE_N = (8, 70, 260)


def rotations(n):
    return tuple(sorted({r for r in (0, 1, n - 1, 63, 64) if r < n}))


def dent(n, c):
    """regular(n) with corner c on the ray of its angle, half way between the chord (c - 1, c + 1), at cos(2 pi / n), and the
    chord (c - 2, c + 1), at cos(3 pi / n) / cos(pi / n): reflex, and convex as soon as c - 1 or c + 1 has been clipped."""
    p = R.regular(n)
    t = 0.1 + 2.0 * np.pi * c / n
    r = 0.5 * (np.cos(2.0 * np.pi / n) + np.cos(3.0 * np.pi / n) / np.cos(np.pi / n))
    p[c] = (r * np.cos(t), r * np.sin(t))
    return p


def dent_corners(n):
    return tuple(sorted({c for c in (0, 1, 64, n - 1) if c < n}))


def _groups():
    g = {}
    for n in CONVEX_N:
        g["convex-%d" % n] = ["convex-%d-%d" % (n, r) for r in rotations(n)]
    for n in DENT_N:
        g["dent-%d" % n] = ["dent-%d-%d" % (n, c) for c in dent_corners(n)]
    for n in LATE_N:
        g["star-%d" % n] = ["star-%d-%d" % (n, r) for r in rotations(n)]
        g["spiral-%d" % n] = ["spiral-%d-%d" % (n, r) for r in rotations(n)]
    for n in DEGENERATE_N:
        g["collinear-%d" % n] = ["collinear-%d-%d" % (n, r) for r in rotations(n)]
        g["pinched-%d" % n] = ["pinched-%d-%d" % (n, r) for r in rotations(n)]
    return g


GROUPS = _groups()
FAMILIES = {"convex": R.regular, "star": R.star, "spiral": R.spiral, "collinear": R.collinear, "pinched": R.pinched}


@functools.lru_cache(maxsize=None)
def build(name):
    fam, n, r = name.split("-")
    if fam == "dent":
        return R.prism_over(dent(int(n), int(r)))
    return R.prism_over(R.rotated(FAMILIES[fam](int(n)), int(r)))


def clearings(pos, loop, trace):
    """The ears (places in the trace) after which a reflex flag was cleared, by replaying the trace with the rule's own predicate."""
    n = len(loop)
    F = R._Face(pos, list(loop), R._Margin())
    idx = np.arange(n)
    prv, nxt = (idx - 1) % n, (idx + 1) % n
    rfx = ~F.right(prv, idx, nxt)
    first = int(rfx.sum())
    at = []
    for k, (p, c, q) in enumerate(trace[:-1]):
        nxt[p] = q; prv[q] = p
        for v in (p, q):
            if rfx[v] and F.right(int(prv[v]), v, int(nxt[v])):
                rfx[v] = False
                at.append(k)
    return first, at


def conditions(name):
    """What the case was designed to be, from the reference alone."""
    s = build(name)
    fam, n, r = name.split("-")
    n, r = int(n), int(r)
    caps = [R.canonical(f) for f in s["faces"] if len(f) == n][:2] if n != 4 else []
    for loop in caps:
        m = R._Margin()
        tris, info = R.ear_clip_f32(s["pos"], loop, m)
        if fam == "collinear":
            assert info["stalled"] and info["ears"] == 0 and not tris, name
            continue
        # (a pinched polygon numbered from another corner takes its normal from corners next to the pinch: decisions that are exactly
        # 0 in float64 as well; the three implementations still have to agree on them)
        assert not info["stalled"] and len(tris) == n - 2 and (m.ratio >= 1 or (fam == "pinched" and r != 0)), (name, m.ratio)
        first, at = clearings(s["pos"], loop, info["ear_trace"])
        assert len(at) == info["cleared"], (name, at, info["cleared"])
        if fam == "convex":
            assert first == 0 and info["refused_reflex"] == 0 and info["refused_inside"] == 0 and m.zeros == 0, name
        elif fam == "dent":
            # one reflex corner, cleared by the first ear next to it, and ears follow: the switch is taken inside the loop
            assert first == 1 and info["cleared"] == 1 and info["refused_inside"] == 0 and m.zeros == 0, (name, first, info["cleared"])
            assert len(info["ear_trace"]) - 1 - at[0] >= 2, ("no ear follows the clearing", name, at)
        elif fam in ("star", "spiral"):
            # several reflex corners, cleared one at a time, the last of them after ears that were clipped with a reflex corner left
            assert first >= 2 and at[-1] >= 1 and at[-1] > at[0], (name, first, at)
        elif fam == "pinched":
            assert info["same_position"] >= 1, name


def loops_of(fo, fi):
    return [tuple(int(v) for v in fi[fo[k]:fo[k + 1]]) for k in range(fo.shape[0] - 1)]


def twins_of(s, loop):
    """The pairs of vertices of this loop that carry one position (only the caps of a pinched prism have one)."""
    seen, pairs = {}, []
    for v in loop:
        key = s["pos"][v].tobytes()
        if key in seen:
            pairs.append((min(seen[key], v), max(seen[key], v)))
        seen[key] = v
    return tuple(pairs)


def per_face(s, loops):
    return [np.asarray(R.ear_clip_f32(s["pos"], lp)[0], np.uint32).reshape(-1) for lp in loops]


def check_solid(eng, oracle, name):
    conditions(name)
    s = build(name)
    fo, fi = eng.extract_faces(s)
    ofo, ofi = oracle.extract_faces(s)
    assert np.array_equal(fo, ofo) and np.array_equal(fi, ofi), ("loops differ from the oracle's", name)
    loops = loops_of(fo, fi)
    vnc, idx = eng.triangulate(s, is_convex=False, color=COLOUR)
    ovnc, oidx = oracle.render(s, convex=False, colour=COLOUR)
    per = per_face(s, loops)
    at = 0
    for k, want in enumerate(per):
        got = idx[at:at + want.size]
        assert np.array_equal(got, want), ("face differs from ear_clip_f32", name, k, len(loops[k]), got[:12], want[:12])
        at += want.size
    assert at == idx.size, ("more indices than the faces account for", name, at, idx.size)
    assert np.array_equal(idx, oidx), ("indices differ from the oracle's", name)
    assert np.array_equal(vnc, ovnc), name
    pos64 = s["pos"].astype(np.float64)
    for lp, tris in zip(loops, per):
        if tris.size == 0:
            assert R.ear_clip_f32(s["pos"], lp)[1]["stalled"], (name, "no triangles on a face that did not stall")
            continue
        R.replay_check(pos64, lp, tris.reshape(-1, 3), coincident=twins_of(s, lp))


def run_cases(E, oracle, names):
    eng = E.Engine(0)
    try:
        for name in names:
            check_solid(eng, oracle, name)
    finally:
        eng.close()


# ------------------------------------------------------------------ the batch event
def _prisms(*polys):
    return R.union([R.prism_over(p) for p in polys])


def stall_last(n):
    """A prism over collinear(n) whose lower cap is replaced by the n triangles to a vertex below it: only the upper cap, the last
    face of the solid, stalls."""
    poly = R.collinear(n)
    pos = np.concatenate([R._lift(poly, 0.0), R._lift(poly, 1.0), [[0.5 * (n - 1), 0.0, -1.0]]])
    faces = [[n + i for i in range(n)]] + [[k, (k + 1) % n, n + (k + 1) % n, n + k] for k in range(n)] + [[(k + 1) % n, k, 2 * n] for k in range(n)]
    return R.solid(pos, faces)


# name -> builder.  What each is there for is asserted in batch_conditions.
BATCH = {
    "stall-between": lambda: _prisms(R.regular(5), R.collinear(8), R.regular(6)),
    "stall-first-last": lambda: R.prism_over(R.collinear(8)),
    "stall-first-only": lambda: R.pyramid_over(R.collinear(8)),
    "stall-last-only": lambda: stall_last(8),
    "stall-first-last-70": lambda: R.prism_over(R.collinear(70)),
    "tris-quads": lambda: R.union([R.prism_over(R.regular(4)), R.pyramid_over(R.regular(4)), R.pyramid_over(R.regular(3))]),
    "convex-5": lambda: build("convex-5-0"), "convex-9": lambda: build("convex-9-0"), "convex-64": lambda: build("convex-64-63"),
    "convex-65": lambda: build("convex-65-64"), "convex-257": lambda: build("convex-257-1"),
    "dent-6": lambda: build("dent-6-1"), "dent-9": lambda: build("dent-9-0"), "dent-64": lambda: build("dent-64-63"),
    "dent-130": lambda: build("dent-130-64"), "dent-257": lambda: build("dent-257-256"),
    "star-8": lambda: build("star-8-0"), "star-66": lambda: build("star-66-64"), "spiral-12": lambda: build("spiral-12-1"),
    "spiral-260": lambda: build("spiral-260-63"), "pinched-8": lambda: build("pinched-8-0"), "pinched-70": lambda: build("pinched-70-0"),
    "mixed": lambda: _prisms(R.star(12), R.collinear(9), dent(65, 64), R.spiral(66)),
}


@functools.lru_cache(maxsize=None)
def batch_solids():
    return [BATCH[k]() for k in BATCH]


def batch_conditions(oracle):
    names = list(BATCH)
    stalled = {}
    for name, s in zip(names, batch_solids()):
        loops = loops_of(*oracle.extract_faces(s))
        stalled[name] = ([k for k, lp in enumerate(loops) if R.ear_clip_f32(s["pos"], lp)[1]["stalled"]], [len(lp) for lp in loops])
    st, ln = stalled["stall-between"]
    assert st and 0 < st[0] and st[-1] < len(ln) - 1 and all(k - 1 not in st or k + 1 not in st for k in st), st
    st, ln = stalled["stall-first-last"]
    assert st == [0, len(ln) - 1], st
    st, ln = stalled["stall-first-only"]
    assert st == [0] and len(ln) > 2, st
    st, ln = stalled["stall-last-only"]
    assert st == [len(ln) - 1] and len(ln) > 2, st
    st, ln = stalled["tris-quads"]
    assert not st and set(ln) == {3, 4}, ln
    assert stalled["mixed"][0] and not stalled["star-66"][0]


def run_batch(E, oracle):
    batch_conditions(oracle)
    solids = batch_solids()
    want = [oracle.render(s, convex=False) for s in solids]
    eng = E.Engine(0)
    try:
        eng.load_fragments(solids, solids)
        eng.event_triangulate(False)
        ev = eng.download()
        c = eng.event_counts()
        assert c.status == 0 and c.n_frag == len(solids)
        sizes = [w[1].size for w in want]
        assert c.n_idx == sum(sizes) == ev["idx"].size, (c.n_idx, sum(sizes))
        assert np.array_equal(ev["idx_off"], np.concatenate([[0], np.cumsum(sizes)])), "idx_off / idx_n"
        assert np.array_equal(ev["idx"], np.concatenate([w[1] for w in want])), "idx"
        assert np.array_equal(ev["vnc"], np.concatenate([w[0] for w in want])), "vnc"
        for k, (name, s) in enumerate(zip(BATCH, solids)):
            a, b = int(ev["idx_off"][k]), int(ev["idx_off"][k + 1])
            per = per_face(s, loops_of(*oracle.extract_faces(s)))
            assert np.array_equal(ev["idx"][a:b], np.concatenate(per)), ("fragment differs from ear_clip_f32", name)
    finally:
        eng.close()


# ------------------------------------------------------------------ CPU tier (emulation)
@pytest.mark.parametrize("group", list(GROUPS))
def test_fan_shapes(emul_engine, oracle, group):
    run_cases(emul_engine, oracle, GROUPS[group])


@pytest.mark.parametrize("tier", [None, 256])
def test_fan_batch(emul_engine, oracle, monkeypatch, tier):
    """tier: every fragment above 256 half-edges goes to the second launch of k_faces, as in test_faces_shapes.test_batch."""
    if tier is not None:
        monkeypatch.setenv("SURTR_FACES_TIER_HE", str(tier))
    run_batch(emul_engine, oracle)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys, time
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    from surtr_amd import engine
    from oracle import oracle as O
    import test_faces_fan as T
    case = sys.argv[1]
    O.lib()
    t0 = time.time()
    if case == "batch":
        T.run_batch(engine, O)
    else:
        T.run_cases(engine, O, [c for g, cs in T.GROUPS.items() if g.split("-")[0] in case.split("+") for c in cs])
    print("seconds %%.1f" %% (time.time() - t0))
    print("ok", case)
""")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["convex+dent", "star+spiral", "collinear+pinched", "batch"])
def test_gpu_fan(case):
    run_gpu_child(GPU_CHILD, case, 180)
