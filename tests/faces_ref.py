"""Designed solids for k_faces (face extraction and ear clipping) and a plain statement of what their triangles must be.

numpy and scipy only, no ctypes, no code shared with oracle/ or the kernels.  Three things live here:

  builders          solids whose faces are known by construction (prisms, pyramids, roofs and bipyramids over designed polygons, the
                    tangent polytope of a Fibonacci sphere, unions of solids), positions rounded once from float64 to float32;
  ear_clip_f32      Poly::EarClipping restated from SURVEY.md and the comments of ear_clip_face, in np.float32 arithmetic, one
                    operation at a time, with counters of what it decided, and predicate_margin: how far every decision it took
                    was from zero, in units of the float32 rounding of that expression;
  replay_check      what a valid ear clipping IS, in float64, whichever ear was chosen: every triangle is (prv, cur, nxt) of the loop
                    that is left, turns the way the polygon does, holds no other remaining vertex, there are len - 2 of them and
                    their areas add up to the polygon's.

The rule (one face, vertices loop[0..N-1]).  n = (p1 - p0) x (p2 - p0), negated when (sum over v of (pv - p0) x (pv+1 - p0)) . n < 0.
right(a, b, c) = ((b - a) x (c - a)) . n > 0, the dot product summed as (x x' + y y') + z z'.  A vertex is reflex when its corner
(prv, v, nxt) is NOT right.  cur starts at 0.  While more than three vertices are left: cur is an ear when it is not flagged reflex
and no flagged vertex r (in index order; r other than prv and nxt, and not at the position of prv or of cur) is right of all three
edges prv->cur, cur->nxt, nxt->prv.  An ear is written as (prv, cur, nxt) and unlinked; prv and nxt are looked at again ONLY where
they were flagged reflex (a flag is never set again).  Anything else counts as skipped, and the face is dropped -- no triangles at
all -- once `++skipped > left`; an ear resets the count.  Then cur = nxt.  The last three vertices are written as (prv, cur, nxt)."""
import numpy as np

from regroup_ref import solid          # (rings from face loops: regroup_ref.rings_from_faces)

EPS32 = 2.0 ** -23
F32 = np.float32


# ------------------------------------------------------------------------------------------------------------------ polygon families
def regular(n, phase=0.1):
    t = phase + 2.0 * np.pi * np.arange(n) / n
    return np.stack([np.cos(t), np.sin(t)], 1)


def _cross2(u, v):
    return u[..., 0] * v[..., 1] - u[..., 1] * v[..., 0]


def is_simple(poly):
    """No two edges that share no corner meet (float64, all pairs)."""
    p = np.asarray(poly, np.float64)
    n = p.shape[0]
    a, b = p, np.roll(p, -1, 0)
    d = b - a
    i, j = np.triu_indices(n, 2)
    keep = ~((i == 0) & (j == n - 1))
    i, j = i[keep], j[keep]
    s1 = _cross2(d[i], a[j] - a[i]); s2 = _cross2(d[i], b[j] - a[i])
    s3 = _cross2(d[j], a[i] - a[j]); s4 = _cross2(d[j], b[i] - a[j])
    return not np.any((s1 * s2 <= 0) & (s3 * s4 <= 0))


def star(n, r_in=0.53, phase=0.1):
    """Alternating radii about 1 and about r_in (n even, n >= 8; each a few per cent off, by a fixed sequence, so that no three
    corners are in line by symmetry): even corners are tips, odd corners reflex.  A polygon whose corners go round a
    centre in order of angle can never refuse an ear for a vertex inside it (the ear lies in the wedge of its three corners, which
    holds no other corner), so ONE inner corner -- corner 3 -- is drawn through the centre into the tooth across: that tooth is a
    convex corner that is no ear until the slit's tip has been cut free.  Tooth and place in it are the first of a fixed list that leave
    the polygon simple."""
    assert n % 2 == 0 and n >= 8
    t = phase + 2.0 * np.pi * np.arange(n) / n
    k = np.arange(n)
    rad = np.where(k % 2 == 0, 1.0 + 0.04 * np.sin(2.3 * k + 1.0), r_in * (1.0 + 0.06 * np.sin(1.7 * k)))
    base = np.stack([rad * np.cos(t), rad * np.sin(t)], 1)
    across = [(3 + n // 2 + d) % n for d in (0, 1, -1)]
    for tip in [c for c in across if c % 2 == 0]:
        for wa, wb in ((0.3, 0.2), (0.4, 0.3), (0.45, 0.35), (0.5, 0.38)):      # (off the tooth's axis: no three corners in line)
            p = base.copy()
            p[3] = wa * base[tip - 1] + wb * base[(tip + 1) % n] + (1.0 - wa - wb) * base[tip]
            if is_simple(p):
                return p
    raise AssertionError("no slit for a star of %d corners" % n)


def spiral(n, turns=1.75, gap=1.0, width=0.5):
    """A thick spiral arm of min(turns, n / 24) turns: n // 2 corners outwards along its outer side, the others back along its inner
    side.  Ears of the outer side reach across the arm once it has been thinned out: candidate ears hold reflex corners of the inner
    side, which belong to a far part of the loop."""
    assert n >= 8
    turns = min(turns, n / 24.0)
    no = n // 2
    ni = n - no
    to = 2.0 * np.pi * turns * (np.arange(no) + 0.5) / no
    ti = 2.0 * np.pi * turns * (np.arange(ni) + 0.25) / ni
    ro = 1.0 + gap * to / (2.0 * np.pi) + width
    ri = 1.0 + gap * ti / (2.0 * np.pi)
    outer = np.stack([ro * np.cos(to), ro * np.sin(to)], 1)
    inner = np.stack([ri * np.cos(ti), ri * np.sin(ti)], 1)[::-1]
    return np.concatenate([outer, inner])


def collinear(n):
    """(k, 0), k = 0 .. n-1: every corner, the normal and the orientation sum are exactly 0 in any precision."""
    return np.stack([np.arange(n, dtype=np.float64), np.zeros(n)], 1)


def pinched(n):
    """Two round lobes that touch in the origin, which two different corners (0 and n // 2) carry: a loop that passes twice through
    one position.  Both carriers are reflex, and each is met as "a reflex vertex at the position of prv / cur" by the ears of the
    other lobe next to the pinch."""
    assert n >= 8 and n % 2 == 0
    k = n // 2 - 1
    j = np.arange(1, k + 1)
    ta = np.pi + 2.0 * np.pi * j / (k + 1)
    tb = 2.0 * np.pi * j / (k + 1)
    A = np.stack([1.0 + np.cos(ta), np.sin(ta)], 1)
    B = np.stack([-1.0 + np.cos(tb), np.sin(tb)], 1)
    z = np.zeros((1, 2))
    return np.concatenate([z, A, z, B])


def rotated(poly, r):
    """The same polygon numbered from corner r."""
    return np.roll(np.asarray(poly), -int(r) % len(poly), axis=0)


# ------------------------------------------------------------------------------------------------------------------ solids
def _lift(poly, z):
    poly = np.asarray(poly, np.float64)
    return np.concatenate([poly, np.full((poly.shape[0], 1), float(z))], 1)


def prism_over(poly2d):
    """2N vertices, 6N half-edges: the caps are N-gons (the lower one runs the other way round), the walls quads."""
    n = len(poly2d)
    faces = [[0] + list(range(n - 1, 0, -1)), list(range(n, 2 * n))]
    faces += [[k, (k + 1) % n, n + (k + 1) % n, n + k] for k in range(n)]
    return solid(np.concatenate([_lift(poly2d, 0.0), _lift(poly2d, 1.0)]), faces)


def _base_faces(n, diagonals):
    """The base N-gon seen from below, cut along the given diagonals (pairs of corners; they must not cross)."""
    loops = [[0] + list(range(n - 1, 0, -1))]
    for a, b in diagonals:
        for q, lp in enumerate(loops):
            if a in lp and b in lp:
                i, j = sorted((lp.index(a), lp.index(b)))
                loops[q:q + 1] = [lp[i:j + 1], lp[j:] + lp[:i + 1]]
                break
        else:
            raise AssertionError("diagonal crosses another")
    return loops


def pyramid_over(poly2d, apex=(0.0, 0.0, 1.0), diagonals=()):
    """N + 1 vertices, 4N half-edges (+ 2 per diagonal of the base): the base an N-gon, the walls triangles."""
    n = len(poly2d)
    faces = _base_faces(n, diagonals) + [[k, (k + 1) % n, n] for k in range(n)]
    return solid(np.concatenate([_lift(poly2d, 0.0), np.asarray([apex], np.float64)]), faces)


def roof_over(poly2d, split, ridge=((-0.25, 0.0, 1.0), (0.25, 0.0, 1.0))):
    """A pyramid whose apex is an edge: corners 0 .. split hang on ridge vertex N, the others on N + 1.  N + 2 vertices and
    4N + 2 half-edges: the even counts between two pyramids."""
    n = len(poly2d)
    faces = _base_faces(n, ())
    faces += [[k, k + 1, n] for k in range(split)] + [[split, split + 1, n + 1, n]]
    faces += [[k, k + 1, n + 1] for k in range(split + 1, n - 1)] + [[n - 1, 0, n, n + 1]]
    return solid(np.concatenate([_lift(poly2d, 0.0), np.asarray(ridge, np.float64)]), faces)


def bipyramid_over(poly2d):
    """N + 2 vertices, 6N half-edges, 2N triangles."""
    n = len(poly2d)
    faces = [[k, (k + 1) % n, n] for k in range(n)] + [[(k + 1) % n, k, n + 1] for k in range(n)]
    return solid(np.concatenate([_lift(poly2d, 0.0), np.asarray([(0, 0, 1.0), (0, 0, -1.0)], np.float64)]), faces)


def tangent_polytope(n_faces):
    """{x : p_i . x <= 1} over n_faces points p_i of a Fibonacci sphere: 2 n - 4 vertices, 6 n - 12 half-edges, every face a convex
    polygon of (mostly) 5 to 7 corners that touches the unit sphere in p_i."""
    from scipy.spatial import ConvexHull
    i = np.arange(n_faces) + 0.5
    z = 1.0 - 2.0 * i / n_faces
    t = np.pi * (1.0 + 5.0 ** 0.5) * i
    p = np.stack([np.sqrt(1.0 - z * z) * np.cos(t), np.sqrt(1.0 - z * z) * np.sin(t), z], 1)
    simp = ConvexHull(p).simplices
    verts = np.linalg.solve(p[simp], np.ones((simp.shape[0], 3, 1)))[:, :, 0]       # the point on all three tangent planes
    faces = []
    for f in range(n_faces):
        mine = np.nonzero((simp == f).any(1))[0]
        e1 = np.cross(p[f], [1.0, 0.0, 0.0] if abs(p[f, 0]) < 0.9 else [0.0, 1.0, 0.0])
        e2 = np.cross(p[f], e1)                                                       # e1 x e2 is along p_f: counter-clockwise from outside
        d = verts[mine] - p[f]
        faces.append(mine[np.argsort(np.arctan2(d @ e2, d @ e1))].tolist())
    return solid(verts, faces)


def union(solids):
    """Several solids as one disconnected solid."""
    pos, faces, base = [], [], 0
    for s in solids:
        pos.append(np.asarray(s["pos"], np.float32))
        faces += [[base + v for v in f] for f in s["faces"]]
        base += s["pos"].shape[0]
    return solid(np.concatenate(pos), faces)


def canonical(loop):
    """A loop up to rotation: started at its smallest vertex."""
    loop = [int(v) for v in loop]
    k = loop.index(min(loop))
    return tuple(loop[k:] + loop[:k])


# ------------------------------------------------------------------------------------------------------------------ ear clipping, float32
class _Margin:
    """Smallest |det64| / bound over the predicates evaluated, exact zeros apart."""

    def __init__(self):
        self.ratio, self.zeros, self.count = np.inf, 0, 0

    def take(self, det64, bound):
        det64 = np.abs(np.atleast_1d(det64)); bound = np.atleast_1d(bound)
        self.count += det64.size
        nz = det64 > 0
        self.zeros += int(det64.size - nz.sum())
        if nz.any():
            self.ratio = min(self.ratio, float((det64[nz] / np.maximum(bound[nz], 1e-300)).min()))


def _cross32(u, w):
    """float32, every product and difference rounded on its own."""
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


def _dot32(k, n):
    return (k[..., 0] * n[0] + k[..., 1] * n[1]) + k[..., 2] * n[2]


def _norm(v):
    v = np.asarray(v, np.float64)
    return np.sqrt(np.einsum("...i,...i->...", v, v))


def _cross64(u, w):
    """(np.cross spends its time on bookkeeping when the arrays are small)"""
    return np.stack([u[..., 1] * w[..., 2] - u[..., 2] * w[..., 1], u[..., 2] * w[..., 0] - u[..., 0] * w[..., 2],
                     u[..., 0] * w[..., 1] - u[..., 1] * w[..., 0]], -1)


class _Face:
    """Positions of one loop in float32 (P) and float64 (Q), its normal in both, and right() with every triple it is asked kept for
    the margin.

    THE BOUND.  u = eps32 / 2 is the unit roundoff.  Each coordinate difference carries (1 + d), |d| <= u.  A component of the cross
    product, fl(fl(a b) - fl(c d)), carries two differences, a product and a subtraction: an error of at most 4u (|a b| + |c d|) <=
    4u |U| |W| by Cauchy-Schwarz, so the computed cross product K of U and W is off by a vector e_K of at most 4 sqrt(3) u |U| |W|,
    and the normal n (from U0, W0, the first two edges; the flip only changes its sign) by e_n of at most 4 sqrt(3) u |U0| |W0|.  The
    dot product (x x' + y y') + z z' adds at most three roundings to each term: 3u |K| |n|.  So
        |computed - K.n| <= |e_K| |n| + |K| |e_n| + 3u |K| |n| <= u (4 sqrt 3 (|U| |W| |n| + |K| |U0| |W0|) + 3 |K| |n|)
    to first order; it is taken with 0.55 eps32 instead of u = 0.5 eps32 for the second-order terms.  (The middle term cannot turn a
    sign on a flat face, where K is along n; it is kept because a face need not be flat.)  The float64 value it is compared with is
    exact to 2^-50 of the same products.
    The orientation sum S = sum of N cross products: each term is off by 4 sqrt 3 u |U_v| |W_v|, each of the N additions rounds the
    partial sum S_v it produces by u |S_v|, so |e_S| <= u (4 sqrt 3 sum |U_v| |W_v| + sum |S_v|), and as above
        |computed - S.n| <= |e_S| |n| + u (4 sqrt 3 |S| |U0| |W0| + 3 |S| |n|)."""
    U_EFF = 0.55 * EPS32
    R3 = 4.0 * 3.0 ** 0.5

    def __init__(self, pos, loop, margin):
        self.P = np.asarray(pos, F32)[np.asarray(loop, np.int64)]
        self.Q = self.P.astype(np.float64)
        self.m = margin
        self.asked = []
        P, Q, N = self.P, self.Q, self.P.shape[0]
        n32 = _cross32(P[1] - P[0], P[2] - P[0])
        n64 = _cross64(Q[1] - Q[0], Q[2] - Q[0])
        self.n_mag = float(_norm(Q[1] - Q[0]) * _norm(Q[2] - Q[0]))
        self.n_len = float(_norm(n64))
        after = (np.arange(N) + 1) % N
        terms = _cross32(P - P[0], P[after] - P[0])
        s = np.zeros(3, F32)
        for v in range(N):                                  # in order: float addition is not associative
            s = s + terms[v]
        U, W = Q - Q[0], Q[after] - Q[0]
        t64 = _cross64(U, W)
        s64 = t64.sum(0)
        if margin is not None:
            e_s = self.R3 * float((_norm(U) * _norm(W)).sum()) + float(_norm(np.cumsum(t64, 0)).sum())
            s_len = float(_norm(s64))
            margin.take(s64 @ n64, self.U_EFF * (e_s * self.n_len + self.R3 * s_len * self.n_mag + 3.0 * s_len * self.n_len))
        self.flipped = bool(_dot32(s, n32) < 0)
        self.n32 = -n32 if self.flipped else n32
        self.n64 = -n64 if s64 @ n64 < 0 else n64
        self.X, self.Y, self.Z = (np.ascontiguousarray(P[:, k]) for k in range(3))
        self.twice = len({tuple(r) for r in P.tolist()}) < N          # some position is carried by two vertices

    def right(self, a, b, c):
        """a, b, c: loop indices, scalars or arrays that broadcast."""
        if self.m is not None:
            self.asked.append((a, b, c))
        X, Y, Z = self.X, self.Y, self.Z
        ux, uy, uz = X[b] - X[a], Y[b] - Y[a], Z[b] - Z[a]
        wx, wy, wz = X[c] - X[a], Y[c] - Y[a], Z[c] - Z[a]
        kx, ky, kz = uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx
        n = self.n32
        return ((kx * n[0] + ky * n[1]) + kz * n[2]) > 0

    def settle(self):
        """The margins of everything right() was asked, in one pass."""
        if self.m is None or not self.asked:
            return
        a, b, c = (np.concatenate([np.broadcast_to(q[k], np.broadcast(*q).shape).ravel() for q in self.asked]) for k in range(3))
        X, Y, Z = (self.Q[:, k].copy() for k in range(3))
        xa, ya, za = X[a], Y[a], Z[a]
        ux, uy, uz, wx, wy, wz = X[b] - xa, Y[b] - ya, Z[b] - za, X[c] - xa, Y[c] - ya, Z[c] - za
        kx, ky, kz = uy * wz - uz * wy, uz * wx - ux * wz, ux * wy - uy * wx
        n = self.n64
        uw = np.sqrt((ux * ux + uy * uy + uz * uz) * (wx * wx + wy * wy + wz * wz))
        k_len = np.sqrt(kx * kx + ky * ky + kz * kz)
        self.m.take(kx * n[0] + ky * n[1] + kz * n[2], self.U_EFF * (self.R3 * (uw * self.n_len + k_len * self.n_mag) + 3.0 * k_len * self.n_len))


def ear_clip_f32(pos, loop, margin=None):
    """-> (triangles as vertex ids [(a, b, c), ...], info).  info: ears, refused_reflex, refused_inside, cleared, same_position (reflex
    vertices passed over because they sit at the position of prv or cur), stalled, and the trace: `ear_trace` as (prv, cur, nxt) loop
    indices in order (the last three vertices included), `deciders` the loop index of the reflex vertex that refused each refused candidate."""
    loop = [int(v) for v in loop]
    N = len(loop)
    info = {"n": N, "ears": 0, "refused_reflex": 0, "refused_inside": 0, "cleared": 0, "same_position": 0, "stalled": False,
            "ear_trace": [], "deciders": []}
    if N <= 2:
        return [], info
    if N == 3:
        return [tuple(loop)], info
    key = np.asarray(pos, F32)[np.asarray(loop, np.int64)].tobytes()
    if key in _CLIPPED:         # (a pure function of the positions in loop order: the walls of a prism numbered from another corner)
        trace, counters, (ratio, zeros, count) = _CLIPPED[key]
        info.update(counters, ear_trace=list(trace), deciders=list(counters["deciders"]))
        if margin is not None:
            margin.ratio, margin.zeros, margin.count = min(margin.ratio, ratio), margin.zeros + zeros, margin.count + count
        return [(loop[p], loop[c], loop[n]) for p, c, n in trace] if not info["stalled"] else [], info
    own = _Margin()
    F = _Face(pos, loop, own)
    P = F.P

    def done(tris):
        F.settle()
        _CLIPPED[key] = (tuple(info["ear_trace"]), {k: v for k, v in info.items() if k != "ear_trace"}, (own.ratio, own.zeros, own.count))
        if margin is not None:
            margin.ratio, margin.zeros, margin.count = min(margin.ratio, own.ratio), margin.zeros + own.zeros, margin.count + own.count
        return tris, info
    idx = np.arange(N)
    prv, nxt = (idx - 1) % N, (idx + 1) % N
    rfx = ~F.right(prv, idx, nxt)
    n_rfx = int(rfx.sum())
    tris, skipped, left, cur = [], 0, N, 0
    while left > 3:
        p, n = int(prv[cur]), int(nxt[cur])
        ear = not rfx[cur]
        if not ear:
            info["refused_reflex"] += 1
        elif n_rfx:
            r = np.nonzero(rfx)[0]
            r = r[(r != p) & (r != n)]
            if F.twice:
                same = (P[r] == P[p]).all(1) | (P[r] == P[cur]).all(1)
                info["same_position"] += int(same.sum())
                r = r[~same]
            # (every lane of the wave clippers tests its own vertex, the serial ones stop at the first hit: all of them are taken
            # here, each through the three tests in order, so the margin covers either)
            for a, b in ((p, cur), (cur, n), (n, p)):
                if r.size:
                    r = r[F.right(a, b, r)]
            if r.size:
                ear = False
                info["refused_inside"] += 1
                info["deciders"].append(int(r[0]))
        if ear:
            tris.append((loop[p], loop[cur], loop[n]))
            info["ear_trace"].append((p, cur, n))
            nxt[p] = n; prv[n] = p
            for v in (p, n):
                if rfx[v] and F.right(int(prv[v]), v, int(nxt[v])):
                    rfx[v] = False
                    n_rfx -= 1
                    info["cleared"] += 1
            info["ears"] += 1
            left -= 1; skipped = 0
        else:
            skipped += 1
            if skipped > left:
                info["stalled"] = True
                return done([])
        cur = n
    tris.append((loop[int(prv[cur])], loop[cur], loop[int(nxt[cur])]))
    info["ear_trace"].append((int(prv[cur]), cur, int(nxt[cur])))
    return done(tris)


_CLIPPED = {}


def predicate_margin(pos, loop):
    """-> (smallest |det| / bound over every right() and the orientation sum the restatement evaluated on this face, how many of
    them were exactly 0, how many there were).  A ratio of 1 and more: float32 and float64 take the same decision."""
    m = _Margin()
    ear_clip_f32(pos, loop, m)
    return m.ratio, m.zeros, m.count


# ------------------------------------------------------------------------------------------------------------------ validity, float64
EPS64 = 2.0 ** -52


def replay_check(pos64, loop, tris, coincident=()):
    """Raises AssertionError unless `tris` (vertex ids) is an ear clipping of `loop`; -> relative error of the summed area.
    coincident: pairs of vertex ids that carry ONE position (pinched loops).  Each of the two lobes the pair closes is a polygon of
    one position less than it has vertices, so of its triangles one cannot have an area: for each pair exactly two triangles hold both
    carriers, and their area must be exactly 0 instead of positive.

    Areas are measured along the unit vector of the loop's float64 vector area A = 1/2 sum (p_v - p_0) x (p_v+1 - p_0).  "Strictly
    inside, with a margin": all three edge functions above 1e-9 of the product of the two lengths they are made of -- 10^6 float64
    roundings of that product, 10^-2 of a float32 one, so that a vertex ON an edge of the ear (which the rule allows) does not count
    and one that float32 could see inside does.  The area bound: each triangle's area is off by at most 4 sqrt 3 EPS64 |U| |W| / 2
    (as in _Face), the polygon's likewise per term, and each of the two sums adds one rounding per term of at most EPS64 times the
    running sum: 8 EPS64 sum |U| |W| over both sets of terms covers it."""
    Q = np.asarray(pos64, np.float64)
    loop = [int(v) for v in loop]
    N = len(loop)
    assert len(tris) == N - 2, ("triangles", len(tris), N - 2)
    at = {v: i for i, v in enumerate(loop)}
    assert len(at) == N
    for tri in tris:
        assert all(int(v) in at for v in tri), ("not of this face", tuple(tri))
    local = [tuple(at[int(v)] for v in tri) for tri in tris]
    twins = frozenset(frozenset(at[v] for v in pair) for pair in coincident)
    L = Q[loop]
    key = (L.tobytes(), tuple(local), twins)          # (a pure function: the walls of a prism numbered from another corner come again)
    if key in _REPLAYED:
        return _REPLAYED[key]
    U, W = L - L[0], L[(np.arange(N) + 1) % N] - L[0]
    A = 0.5 * _cross64(U, W).sum(0)
    area = float(_norm(A))
    assert area > 0
    nrm = A / area
    slack = 8.0 * EPS64 * float((_norm(U) * _norm(W)).sum())
    # along nrm an edge function (d x q) . nrm is the plane cross product of the two vectors' components across it
    e1 = _cross64(nrm, np.eye(3)[int(np.argmin(np.abs(nrm)))])
    e1 /= _norm(e1)
    e2 = _cross64(nrm, e1)
    X, Y = (L - L[0]) @ e1, (L - L[0]) @ e2           # (only the inside test, which has a margin of its own, works on the projection)
    xs, ys = X.tolist(), Y.tolist()
    l3, (n0, n1, n2) = L.tolist(), nrm.tolist()
    prv, nxt = [(i - 1) % N for i in range(N)], [(i + 1) % N for i in range(N)]
    alive = np.ones(N, bool)
    total, flat = 0.0, 0
    for a, b, c in local:
        assert alive[b] and prv[b] == a and nxt[b] == c, ("not (prv, cur, nxt) of what is left", (loop[a], loop[b], loop[c]))
        (ax, ay, az), (bx, by, bz), (cx, cy, cz) = l3[a], l3[b], l3[c]
        ux, uy, uz, wx, wy, wz = bx - ax, by - ay, bz - az, cx - ax, cy - ay, cz - az
        t = 0.5 * ((uy * wz - uz * wy) * n0 + (uz * wx - ux * wz) * n1 + (ux * wy - uy * wx) * n2)
        if any(pair <= {a, b, c} for pair in twins):
            assert t == 0.0, ("a triangle on both carriers of one position has no area", (loop[a], loop[b], loop[c]), t)
            flat += 1
        else:
            assert t > 0, ("area", (loop[a], loop[b], loop[c]), t)
        total += t
        slack += 8.0 * EPS64 * ((ux * ux + uy * uy + uz * uz) * (wx * wx + wy * wy + wz * wz)) ** 0.5
        alive[b] = False
        if N > 3:
            alive[a] = alive[c] = False
            rest = np.nonzero(alive)[0]
            alive[a] = alive[c] = True
            if rest.size:
                rx, ry = X[rest], Y[rest]
                inside = np.ones(rest.size, bool)
                for s_, e_ in ((a, b), (b, c), (c, a)):
                    dx, dy, qx, qy = xs[e_] - xs[s_], ys[e_] - ys[s_], rx - xs[s_], ry - ys[s_]
                    inside &= (dx * qy - dy * qx) > 1e-9 * np.sqrt((dx * dx + dy * dy) * (qx * qx + qy * qy))
                assert not inside.any(), ("vertex inside the ear", (loop[a], loop[b], loop[c]), [loop[i] for i in rest[inside]])
        nxt[a] = c; prv[c] = a
    assert flat == 2 * len(twins), ("two flat triangles for every doubled position", flat, len(twins))
    assert abs(total - area) <= slack, ("area", total, area, slack)
    _REPLAYED[key] = abs(total - area) / area
    return _REPLAYED[key]


_REPLAYED = {}


def edges_paired(tris):
    """Over a whole solid: every directed triangle edge occurs once and its opposite once."""
    t = np.asarray(tris, np.int64).reshape(-1, 3)
    e = np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])
    key = e[:, 0] * (int(e.max()) + 1) + e[:, 1]
    back = e[:, 1] * (int(e.max()) + 1) + e[:, 0]
    return np.unique(key).size == key.size and np.array_equal(np.sort(key), np.sort(back))


def slot_coverage(infos, slot=64):
    """For faces of 65 .. 256 vertices: the slots (loop index // 64) of the deciding reflex vertices, and whether some clipped ear has
    prv and cur, and cur and nxt, in different slots."""
    slots, pc, cn = set(), False, False
    for i in infos:
        if 64 < i["n"] <= 256:
            slots |= {d // slot for d in i["deciders"]}
            pc |= any(p // slot != c // slot for p, c, n in i["ear_trace"])
            cn |= any(c // slot != n // slot for p, c, n in i["ear_trace"])
    return slots, pc, cn
