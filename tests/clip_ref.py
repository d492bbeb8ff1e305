"""A float64 definition of what the fracture event's clip must deliver, and the checkers that hold an event against it.

THE DEFINITION.  The Mesh clip of a piece S (a closed oriented surface given as pos / off / nbr) against a cell C (the float32
planes the engine is given, read as exact float64 half-spaces n.x + d <= 0) is the set S n C.  Its integrals need no clipper
of S: for any fixed point O

    J(S n C) = sum over the triangles T = (a, b, c) of S of  sign(det[a-O, b-O, c-O]) . J(tet(O, a, b, c) n C)

and tet n C is an intersection of two convex bodies (convex_clip below: Sutherland-Hodgman on every face polygon, the cap from
the cut points sorted by angle, integrated by tetrahedra about the body's own vertex mean).  J is the ten integrals of
1, x, y, z, xx, yy, zz, xy, yz, zx about O.  No fragment, ring or island of an event enters reference_integrals().
Nothing here imports the oracle; plain numpy float64 and Python floats throughout.

THE CHECKS (check_event), per event, with eps = 2^-24, L the largest absolute coordinate of the scene, A_c the float64
surface area of the event's Mesh fragments of cell c, tau = K_V . eps . L:
  (a) integrals per (cell, piece): |J_event - J_ref| <= K . eps . L . A_c . L^k, k = 0, 1, 2 for the zeroth, first and second
      integrals (a cut vertex carries a few float32 roundings of size eps.L and moves the boundary by that much over an area
      of at most A_c; the integrand is at most L^k).  A pair without a fragment must have a reference volume below the same
      bound with A_c replaced by the area of the triangles of S that no single plane of C separates from it (the pair has no
      fragment to take an area from; where C misses S that area is 0 and only the float64 floor 2^-40 . L^3 of the sums is left).  Second-level pieces add A_c . p,
      p the piece's largest float64 planarity error (the clip cuts the polygon, the reference its fan).
  (b) old vertices: an input vertex with s < -tau on every plane appears bit-identically exactly once among the fragments of
      its pair; a fragment vertex that is bit-identical to an input vertex has s <= tau on every plane.
  (c) new vertices: every other fragment vertex is within tau of a plane and satisfies all of them within tau; on exactly one
      plane it is within tau of an input triangle; on two or more it is within tau of S or S winds once about it.
  (d) shape: symmetric links, every directed edge in exactly one face loop, Euler characteristic even and <= 2, positive
      volume, no vertex position shared between the islands of a pair, island numbers 0..n-1.
A cell is excused only through the engine's own flags, and the built scenes must raise none.
The Convex side (ConvexScene: Convex n C built by convex_clip as a polytope of its own):
  (e) without refit (check_convex_clip): volume and first integrals of the Convex fragment within K_E . eps . L . A . L^k of the
      polytope's, A the fragment's own area (the same derivation: its cut vertices move its own boundary); Hausdorff distance of
      the two vertex sets <= tau / sin(theta_min), theta_min the smallest angle between two planes that meet at a vertex of the
      polytope; the polytope must have no two vertices closer than 100 tau (a property of the scene, refused as 'e-scene').
  (f) with refit (check_refit): every Mesh vertex satisfies every face plane of the refitted Convex (Newell planes in float64 from
      its own loops); its vertices satisfy every plane of C and of the input Convex; every face is a plane of C, a plane of the
      input Convex, or touches a Mesh vertex: all within plain tau.  Two kinds of face have no plane beyond their vertices'
      rounding and are excused from the first and the last, and counted: narrower than K_W . tau, or a needle with D >= K_N . w
      (see check_refit).  Distances in (e) are Euclidean.

WHAT THE REFERENCE'S REPRESENTATION CANNOT SAY (see test_clip_definition.py, LAMINAE and NEGATIVE): a fragment whose rings list a
neighbour twice is walked as the reference walks it (face_loops(doubled=True)) and is exempt from (d)'s Euler and volume rules; an
island whose volume is within K . eps . L . (its own area) of zero is reported as flat, one below that as negative; in (c) a
vertex off S with winding number 0 passes only with a twin within tau, and the fragment it belongs to is reported.  check_event
returns the four lists (laminae, flat, negative, sheets) and the caller pins them.

THE CONSTANTS are set from the oracle's event (the restated reference, not the code under test) on every scene of
test_clip_definition.py: four times the largest ratio seen, rounded up to a power of two.  The measured ratios and the times of
the reference stand in test_clip_definition.py's docstring next to the scenes they were taken on.
"""
import math

import numpy as np

EPS = 2.0 ** -24
K = 2.0        # (a): bound = K . eps . L . A_c . L^k              (largest oracle ratio 0.33: cube, see test_clip_definition.py)
FLOOR = 2.0 ** -40     # of L^3 . L^k: the float64 rounding of the reference's own sums (signed volumes of size L^3, thousands of terms)
K_V = 16.0     # (b), (c), (e), (f): tau = K_V . eps . L          (largest oracle ratio 4.0: a refitted Convex vertex of cube on its cell plane)


class CheckFailed(AssertionError):
    """One check of check_event refused the event: .check names it ('a', 'b', 'c', 'd', 'flags')."""

    def __init__(self, check, msg):
        AssertionError.__init__(self, "check (%s): %s" % (check, msg))
        self.check = check


# ------------------------------------------------------------------ surface: face loops from the rings
def has_doubled_neighbour(solid):
    off, nbr = np.asarray(solid["off"], np.int64), np.asarray(solid["nbr"], np.int64)
    return any(len(set(nbr[off[v]:off[v + 1]].tolist())) < off[v + 1] - off[v] for v in range(off.shape[0] - 1))


def face_loops(solid, doubled=False):
    """The face loops of a solid from its neighbour rings: from the directed edge (prev, cur) the loop goes on to the neighbour
    that cur's ring lists just before prev.  Raises CheckFailed('d') when a ring names no vertex or lists one twice, a link has
    no way back, or a directed edge would lie in two loops.
    doubled=True: for a solid whose rings list a neighbour twice (the two sheets of a lamina, see check_event): the first
    listing counts, a walk ends where it meets an edge already walked, and a walk longer than the number of links is refused."""
    off = np.asarray(solid["off"], np.int64)
    nbr = np.asarray(solid["nbr"], np.int64)
    n = off.shape[0] - 1
    if nbr.size and (nbr.min() < 0 or nbr.max() >= n):
        raise CheckFailed("d", "a ring entry names no vertex")
    rings = [nbr[off[v]:off[v + 1]].tolist() for v in range(n)]
    where = [{u: k for k, u in reversed(list(enumerate(r)))} for r in rings]
    for v in range(n):
        if v in where[v] or (not doubled and len(where[v]) != len(rings[v])):
            raise CheckFailed("d", "vertex %d lists a neighbour twice or itself" % v)
        for u in rings[v]:
            if v not in where[u]:
                raise CheckFailed("d", "link %d -> %d has no way back" % (v, u))
    seen, loops = set(), []
    for v in range(n):
        for u in rings[v]:
            if (v, u) in seen:
                continue
            loop, prev, cur = [v], v, u
            while True:
                if (prev, cur) in seen and not doubled:
                    raise CheckFailed("d", "directed edge (%d, %d) lies in two face loops" % (prev, cur))
                if len(loop) > nbr.shape[0]:
                    raise CheckFailed("d", "a face walk from (%d, %d) does not end" % (v, u))
                seen.add((prev, cur))
                if cur == v:
                    break
                loop.append(cur)
                prev, cur = cur, rings[cur][where[cur][prev] - 1]
            loops.append(loop)
    return loops


def fan_triangles(solid, loops=None):
    """(T, 3) vertex indices: every loop fanned about its first corner.  The walk above gives loops that run counter-clockwise
    seen from outside: the unit box comes out with volume +1 (test_unit_box_has_volume_one)."""
    tris = [(l[0], l[j], l[j + 1]) for l in (face_loops(solid) if loops is None else loops) for j in range(1, len(l) - 1)]
    return np.asarray(tris, np.int64).reshape(-1, 3)


# ------------------------------------------------------------------ integrals
def tet_J(a, b, c, absolute=False):
    """(T, 10): integrals of 1, x, y, z, xx, yy, zz, xy, yz, zx over the tetrahedra (0, a, b, c), signed by det[a, b, c] (or by
    its absolute value)."""
    v6 = np.einsum("ij,ij->i", a, np.cross(b, c))
    if absolute:
        v6 = np.abs(v6)
    s = a + b + c
    J = np.empty((a.shape[0], 10))
    J[:, 0] = v6 / 6.0
    J[:, 1:4] = v6[:, None] * s / 24.0
    J[:, 4:7] = v6[:, None] * (a * a + b * b + c * c + s * s) / 120.0
    for k, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):
        J[:, 7 + k] = v6 * (a[:, i] * a[:, j] + b[:, i] * b[:, j] + c[:, i] * c[:, j] + s[:, i] * s[:, j]) / 120.0
    return J


def shift_J(J, m):
    """Integrals about a point P, of coordinates taken relative to P + m, restated relative to P.  J (T, 10), m (T, 3)."""
    out = J.copy()
    v = J[:, 0:1]
    out[:, 1:4] = J[:, 1:4] + m * v
    out[:, 4:7] = J[:, 4:7] + 2.0 * m * J[:, 1:4] + m * m * v
    for k, (i, j) in enumerate(((0, 1), (1, 2), (2, 0))):
        out[:, 7 + k] = J[:, 7 + k] + m[:, i] * J[:, 1 + j] + m[:, j] * J[:, 1 + i] + m[:, i] * m[:, j] * J[:, 0]
    return out


def surface_J(pos64, tris, origin):
    """J of the solid bounded by the triangles, about origin."""
    p = pos64 - origin
    return tet_J(p[tris[:, 0]], p[tris[:, 1]], p[tris[:, 2]]).sum(0)


def surface_area(pos64, tris):
    return float(np.linalg.norm(np.cross(pos64[tris[:, 1]] - pos64[tris[:, 0]], pos64[tris[:, 2]] - pos64[tris[:, 0]]), axis=1).sum() / 2.0)


def planarity_error(solid, loops=None, min_width=0.0):
    """The largest float64 distance of a face's corner from that face's Newell plane (0 for a triangle mesh).  A face narrower
    than min_width (area / diameter) has no plane to be off: its normal is rounding."""
    p = np.asarray(solid["pos"], np.float32).reshape(-1, 3).astype(np.float64)
    worst = 0.0
    for l in (face_loops(solid) if loops is None else loops):
        if len(l) < 4:
            continue
        q = p[l]
        c = q.mean(0)
        n = np.cross(q - c, np.roll(q, -1, 0) - c).sum(0)
        ln = np.linalg.norm(n)
        diam = np.sqrt(((q[:, None, :] - q[None, :, :]) ** 2).sum(2).max())
        if ln > 0 and ln / 2.0 > min_width * diam:
            worst = max(worst, float(np.abs((q - c) @ (n / ln)).max()))
    return worst


# ------------------------------------------------------------------ the convex clipper (Python floats: the polygons are tiny)
def _clip_body(faces, n, d):
    """A convex body as a list of face polygons (lists of 3-tuples), cut down to n.x + d <= 0.  A cut point is computed from
    the kept end of its edge towards the dropped one, so that the two faces that share the edge get the same point."""
    nx, ny, nz = n
    out, cuts = [], set()
    for poly in faces:
        s = [nx * p[0] + ny * p[1] + nz * p[2] + d for p in poly]
        if max(s) <= 0.0:
            out.append(poly)
            continue
        if min(s) > 0.0:
            continue
        new, k = [], len(poly)
        for i in range(k):
            a, sa = poly[i], s[i]
            b, sb = poly[(i + 1) % k], s[(i + 1) % k]
            if sa <= 0.0:
                new.append(a)
            if (sa <= 0.0) != (sb <= 0.0):
                if sa <= 0.0:
                    t = sa / (sa - sb)
                    c = (a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), a[2] + t * (b[2] - a[2]))
                else:
                    t = sb / (sb - sa)
                    c = (b[0] + t * (a[0] - b[0]), b[1] + t * (a[1] - b[1]), b[2] + t * (a[2] - b[2]))
                new.append(c)
                cuts.add(c)
        if len(new) >= 3:
            out.append(new)
    if len(cuts) >= 3:
        cs = list(cuts)
        k = len(cs)
        mx, my, mz = sum(c[0] for c in cs) / k, sum(c[1] for c in cs) / k, sum(c[2] for c in cs) / k
        # a basis of the plane: u from the axis least aligned with n, v = n x u
        ax = min(range(3), key=lambda i: abs(n[i]))
        e = [0.0, 0.0, 0.0]
        e[ax] = 1.0
        ux, uy, uz = ny * e[2] - nz * e[1], nz * e[0] - nx * e[2], nx * e[1] - ny * e[0]
        vx, vy, vz = ny * uz - nz * uy, nz * ux - nx * uz, nx * uy - ny * ux
        cs.sort(key=lambda c: math.atan2((c[0] - mx) * vx + (c[1] - my) * vy + (c[2] - mz) * vz,
                                         (c[0] - mx) * ux + (c[1] - my) * uy + (c[2] - mz) * uz))
        out.append(cs)
    return out


def convex_clip(faces, planes):
    """faces cut down by every plane (rows n, d: keeps n.x + d <= 0); [] when nothing with a volume is left."""
    for pl in planes:
        faces = _clip_body(faces, (float(pl[0]), float(pl[1]), float(pl[2])), float(pl[3]))
        if len(faces) < 4:
            return []
    return faces


def body_vertices(faces):
    return np.array(sorted({p for f in faces for p in f}), np.float64).reshape(-1, 3)


def body_triangles(faces):
    """(m, A, B, C): the body's vertex mean and its faces fanned into triangles."""
    m = body_vertices(faces).mean(0)
    tri = [(f[0], f[j], f[j + 1]) for f in faces for j in range(1, len(f) - 1)]
    t = np.asarray(tri, np.float64).reshape(-1, 3, 3)
    return m, t[:, 0], t[:, 1], t[:, 2]


def body_J(faces):
    """J of a convex body about the coordinate origin: by tetrahedra about its own vertex mean, every one of them counted
    positive (the mean lies inside), then shifted."""
    if len(faces) < 4:
        return np.zeros(10)
    m, a, b, c = body_triangles(faces)
    J = tet_J(a - m, b - m, c - m, absolute=True).sum(0)
    return shift_J(J[None], m[None])[0]


def box_faces(lo, hi):
    x0, y0, z0 = (float(v) for v in lo)
    x1, y1, z1 = (float(v) for v in hi)
    c = [(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)]
    return [[c[i] for i in q] for q in ((0, 3, 2, 1), (4, 5, 6, 7), (0, 1, 5, 4), (2, 3, 7, 6), (1, 2, 6, 5), (0, 4, 7, 3))]


def convex_faces(solid, origin):
    """A Convex (pos / off / nbr) as the face polygons of convex_clip, relative to origin."""
    p = np.asarray(solid["pos"], np.float64).reshape(-1, 3) - origin
    return [[tuple(p[v].tolist()) for v in l] for l in face_loops(solid)]


# ------------------------------------------------------------------ the reference: J(S n C) for every cell of a scene
def scene_origin(meshes):
    lo = np.min([np.asarray(m["pos"], np.float64).reshape(-1, 3).min(0) for m in meshes], 0)
    hi = np.max([np.asarray(m["pos"], np.float64).reshape(-1, 3).max(0) for m in meshes], 0)
    return (lo + hi) / 2.0


def scene_L(meshes):
    return float(max(np.abs(np.asarray(m["pos"], np.float64)).max() for m in meshes))


def reference_integrals(solid, plane_off, planes, origin, cells=None):
    """{cell: J(S n C_cell) about origin} for the cells asked for (default: all), from the piece's triangles alone."""
    pos = np.asarray(solid["pos"], np.float32).reshape(-1, 3).astype(np.float64) - origin
    tris = fan_triangles(solid, face_loops(solid, doubled=has_doubled_neighbour(solid)))
    a, b, c = pos[tris[:, 0]], pos[tris[:, 1]], pos[tris[:, 2]]
    det = np.einsum("ij,ij->i", a, np.cross(b, c))
    live = det != 0.0
    a, b, c, sign = a[live], b[live], c[live], np.sign(det[live])
    whole = tet_J(a, b, c, absolute=True)                   # tet(O, a, b, c), counted positive
    P4 = np.stack([np.zeros_like(a), a, b, c], 1)            # (T, 4, 3)
    # the three side planes of every tetrahedron through O and its base plane, normals pointing out of it
    cen = P4.mean(1)
    fn = np.stack([np.cross(a, b), np.cross(b, c), np.cross(c, a), np.cross(c - a, b - a)], 1)       # (T, 4, 3)
    fd = -np.einsum("tkj,tkj->tk", fn, np.stack([a, b, c, a], 1))
    flip = (np.einsum("tkj,tj->tk", fn, cen) + fd) > 0
    fn[flip] *= -1.0
    fd[flip] *= -1.0
    pl64 = np.asarray(planes, np.float32).reshape(-1, 4).astype(np.float64)
    pl64 = pl64.copy()
    pl64[:, 3] += pl64[:, :3] @ origin                       # the same half-spaces in coordinates relative to origin
    po = np.asarray(plane_off, np.int64)
    ext = 4.0 * float(np.abs(pos).max()) + 1.0
    out = {}
    for cell in (range(po.shape[0] - 1) if cells is None else cells):
        cp = pl64[po[cell]:po[cell + 1]]
        J = np.zeros(10)
        out[cell] = J
        hull = convex_clip(box_faces([-ext] * 3, [ext] * 3), cp)
        if not hull:
            continue
        s = P4 @ cp[:, :3].T + cp[:, 3]                       # (T, 4, planes)
        apart = (s > 0).all(1).any(1)                         # one cell plane has the whole tetrahedron on its far side
        inside = (s <= 0).all(1).all(1)
        J += (sign[inside, None] * whole[inside]).sum(0)
        cand = np.nonzero(~apart & ~inside)[0]
        if cand.size:
            hv = body_vertices(hull)
            sv = np.einsum("tkj,vj->tkv", fn[cand], hv) + fd[cand][:, :, None]
            cand = cand[~(sv > 0).all(2).any(1)]              # one plane of the tetrahedron has the whole cell on its far side
        acc_m, acc_a, acc_b, acc_c, acc_s = [], [], [], [], []
        for t in cand:
            pts = [tuple(P4[t, k].tolist()) for k in range(4)]
            cutting = cp[(s[t] > 0).any(0)]
            body = convex_clip([[pts[0], pts[1], pts[2]], [pts[0], pts[2], pts[3]], [pts[0], pts[3], pts[1]], [pts[1], pts[3], pts[2]]], cutting)
            if not body:
                continue
            m, ta, tb, tc = body_triangles(body)
            acc_m.append(np.broadcast_to(m, ta.shape)); acc_a.append(ta); acc_b.append(tb); acc_c.append(tc)
            acc_s.append(np.full(ta.shape[0], sign[t]))
        if acc_a:
            m, ta, tb, tc, sg = (np.concatenate(x) for x in (acc_m, acc_a, acc_b, acc_c, acc_s))
            # one body's tetrahedra about its own mean, shifted to O: the shift is linear, so it may be applied per tetrahedron
            J += (sg[:, None] * shift_J(tet_J(ta - m, tb - m, tc - m, absolute=True), m)).sum(0)
    return out


# ------------------------------------------------------------------ distances and winding numbers (float64, vectorised)
def dist_to_segments(q, a, b):
    """(Q,) distance of every point q to the nearest segment a[i] b[i]."""
    out = np.empty(q.shape[0])
    ab = b - a
    den = np.maximum(np.einsum("ij,ij->i", ab, ab), 1e-300)
    for i0 in range(0, q.shape[0], 256):
        x = q[i0:i0 + 256, None, :] - a[None]
        t = np.clip(np.einsum("qej,ej->qe", x, ab) / den, 0.0, 1.0)
        out[i0:i0 + 256] = np.sqrt(((x - t[..., None] * ab[None]) ** 2).sum(2).min(1))
    return out


def dist_to_triangles(q, a, b, c):
    """(Q,) distance of every point q to the nearest triangle: the distance to its plane where the foot falls inside, else to
    its border."""
    if q.shape[0] == 0:
        return np.zeros(0)
    edge = np.minimum(np.minimum(dist_to_segments(q, a, b), dist_to_segments(q, b, c)), dist_to_segments(q, c, a))
    n = np.cross(b - a, c - a)
    ln = np.linalg.norm(n, axis=1)
    ok = ln > 0
    a, b, c, n = a[ok], b[ok], c[ok], n[ok] / ln[ok, None]
    out = edge.copy()
    for i0 in range(0, q.shape[0], 256):
        x = q[i0:i0 + 256, None, :]
        h = np.einsum("qtj,tj->qt", x - a[None], n)
        f = x - h[..., None] * n[None]
        inside = (np.einsum("qtj,tj->qt", np.cross(b - a, f - a[None]), n) >= 0) & (np.einsum("qtj,tj->qt", np.cross(c - b, f - b[None]), n) >= 0) & \
                 (np.einsum("qtj,tj->qt", np.cross(a - c, f - c[None]), n) >= 0)
        hh = np.where(inside, np.abs(h), np.inf).min(1) if a.shape[0] else np.full(x.shape[0], np.inf)
        out[i0:i0 + 256] = np.minimum(out[i0:i0 + 256], hh)
    return out


def winding_number(q, a, b, c):
    """(Q,) solid-angle winding number of the triangles about every point q (van Oosterom and Strackee)."""
    out = np.empty(q.shape[0])
    for i, p in enumerate(q):
        x, y, z = a - p, b - p, c - p
        lx, ly, lz = np.linalg.norm(x, axis=1), np.linalg.norm(y, axis=1), np.linalg.norm(z, axis=1)
        num = np.einsum("ij,ij->i", x, np.cross(y, z))
        den = lx * ly * lz + np.einsum("ij,ij->i", x, y) * lz + np.einsum("ij,ij->i", y, z) * lx + np.einsum("ij,ij->i", z, x) * ly
        out[i] = 2.0 * np.arctan2(num, den).sum() / (4.0 * np.pi)
    return out


# ------------------------------------------------------------------ the scene's side of the checks, computed once
def _keys(pos32):
    p = np.ascontiguousarray(pos32, np.float32).reshape(-1, 3)
    return [r.tobytes() for r in p]


def fragment(ev, k, which="mesh"):
    vo, no = ev[which + "_vert_off"], ev[which + "_nbr_off"]
    a, b = int(vo[k]), int(vo[k + 1])
    return {"pos": ev[which + "_pos"][a:b], "off": (no[a:b + 1].astype(np.int64) - int(no[a])), "nbr": ev[which + "_nbr"][int(no[a]):int(no[b])]}


class Scene:
    """What check_event needs of the input, computed once per scene: the pieces' triangles, the reference integrals of every
    (cell, piece), L, the origin.  pairs: the (cell, piece) pairs of the event (default: every cell with every piece)."""

    def __init__(self, meshes, plane_off, planes, pairs=None, K=K, K_V=K_V):
        self.meshes = meshes
        self.plane_off = np.asarray(plane_off, np.int64)
        self.planes = np.asarray(planes, np.float32).reshape(-1, 4)
        self.planes64 = self.planes.astype(np.float64)
        n_cells = self.plane_off.shape[0] - 1
        self.pairs = [(c, p) for c in range(n_cells) for p in range(len(meshes))] if pairs is None else [(int(c), int(p)) for c, p in pairs]
        self.origin = scene_origin(meshes)
        self.L = scene_L(meshes)
        self.K, self.K_V = K, K_V
        self.tau = K_V * EPS * self.L
        self.pos64 = [np.asarray(m["pos"], np.float32).reshape(-1, 3).astype(np.float64) for m in meshes]
        self.loops = [face_loops(m, doubled=has_doubled_neighbour(m)) for m in meshes]
        self.tris = [fan_triangles(m, l) for m, l in zip(meshes, self.loops)]
        self.area = [surface_area(p, t) for p, t in zip(self.pos64, self.tris)]
        self.planarity = [planarity_error(m, l, self.tau) for m, l in zip(meshes, self.loops)]
        self.keys = [_keys(m["pos"]) for m in meshes]
        self.edges = []
        for m in meshes:
            off, nbr = np.asarray(m["off"], np.int64), np.asarray(m["nbr"], np.int64)
            src = np.repeat(np.arange(off.shape[0] - 1), np.diff(off))
            self.edges.append(np.stack([src, nbr], 1)[src < nbr])
        self.ref = {}
        by_piece = {}
        for c, p in self.pairs:
            by_piece.setdefault(p, []).append(c)
        for p, cells in by_piece.items():
            for c, J in reference_integrals(meshes[p], self.plane_off, self.planes, self.origin, cells).items():
                self.ref[(c, p)] = J

    def area_near(self, pair):
        """For a pair without a fragment, which has no A_c: the area of the triangles of S that no single plane of the cell has
        wholly on its far side (what of S can reach into C; 0 where the cell misses the piece)."""
        c, p = pair
        cp = self.cell_planes(c)
        P, T = self.pos64[p], self.tris[p]
        s = P @ cp[:, :3].T + cp[:, 3]
        near = ~((s[T[:, 0]] > 0) & (s[T[:, 1]] > 0) & (s[T[:, 2]] > 0)).any(1)
        return surface_area(P, T[near]) if near.any() else 0.0

    def cell_planes(self, c):
        return self.planes64[self.plane_off[c]:self.plane_off[c + 1]]

    def bound(self, area, piece=None):
        """The (a) bound for the ten integrals, given the area it acts on."""
        b = self.K * EPS * self.L * area
        if piece is not None:
            b += area * self.planarity[piece]
        return b * np.array([1.0] + [self.L] * 3 + [self.L ** 2] * 6)


# ------------------------------------------------------------------ the checks
def check_event(scene, ev, flagged_pairs=(), n_failed=0, allow_flags=False, measure=None, checks="abcd"):
    """Holds the Mesh fragments of an event (engine.download's or the oracle's arrays) against the scene's definition.  Raises
    CheckFailed naming the first check that refuses it.  measure: a dict that receives the largest ratios seen
    ('a0', 'a1', 'a2': |dJ| / (eps L A_c L^k); 'v': the largest vertex residual / (eps L))."""
    flagged = set(map(tuple, flagged_pairs))
    if not allow_flags and (flagged or n_failed):
        raise CheckFailed("flags", "the scene raised flags: %r, n_failed %d" % (sorted(flagged), n_failed))
    ids = np.asarray(ev["frag_ids"]).reshape(-1, 3)
    tau, L = scene.tau, scene.L
    by_pair = {}
    for k, (c, p, i) in enumerate(ids.tolist()):
        by_pair.setdefault((c, p), []).append((i, k))
    for pair in by_pair:
        if pair not in scene.ref:
            raise CheckFailed("d", "fragment of a pair that is not in the event: %r" % (pair,))
    frag_J, frag_area, frag_solid = {}, {}, {}
    cell_area, laminae, negative, flat, sheets = {}, [], [], [], set()
    # ---- (d) shape, and the fragments' own integrals
    for pair, lst in sorted(by_pair.items()):
        if "d" in checks and sorted(i for i, _ in lst) != list(range(len(lst))):
            raise CheckFailed("d", "island numbers of pair %r are %r" % (pair, sorted(i for i, _ in lst)))
        for i, k in lst:
            f = fragment(ev, k)
            lamina = has_doubled_neighbour(f)
            if lamina:
                laminae.append((pair[0], pair[1], i))
            loops = face_loops(f, doubled=lamina)
            p64 = np.asarray(f["pos"], np.float32).reshape(-1, 3).astype(np.float64)
            tris = fan_triangles(f, loops)
            J = surface_J(p64, tris, scene.origin)
            frag_J[k], frag_area[k], frag_solid[k] = J, surface_area(p64, tris), (f, p64)
            if "d" in checks and not lamina:
                chi = p64.shape[0] - len(f["nbr"]) // 2 + len(loops)
                if chi % 2 or chi > 2:
                    raise CheckFailed("d", "fragment %d of pair %r has Euler characteristic %d" % (i, pair, chi))
                # positive, or below what float32 vertices resolve over the island's own area (two sheets whose vertices differ
                # by a rounding: the sign of such a volume is rounding too)
                if abs(J[0]) <= scene.K * EPS * L * frag_area[k]:
                    flat.append((pair[0], pair[1], i))
                elif not J[0] > 0:
                    negative.append((pair[0], pair[1], i))
            cell_area[pair[0]] = cell_area.get(pair[0], 0.0) + frag_area[k]
        if "d" in checks and len(lst) > 1:
            seen = {}
            for i, k in lst:
                for key in set(_keys(frag_solid[k][0]["pos"])):
                    if key in seen:
                        raise CheckFailed("d", "islands %d and %d of pair %r share a vertex position" % (seen[key], i, pair))
                    seen[key] = i
    # ---- (a) integrals per (cell, piece)
    powers = np.array([1.0] + [L] * 3 + [L ** 2] * 6)
    for pair in scene.pairs:
        ref = scene.ref[pair]
        if pair in flagged:
            continue
        if pair in by_pair:
            J = sum(frag_J[k] for _, k in by_pair[pair])
            area = cell_area[pair[0]]
        else:
            J, area = np.zeros(10), scene.area_near(pair)
        ratio = np.abs(J - ref) / (EPS * L * area * powers) if area > 0 else np.zeros(10)      # (no area: only the floor below)
        if measure is not None:
            extra = scene.planarity[pair[1]] / (EPS * L)
            for name, r in (("a0", ratio[0]), ("a1", ratio[1:4].max()), ("a2", ratio[4:].max())):
                measure[name] = max(measure.get(name, 0.0), float(r))
                measure[name + "_less_planarity"] = max(measure.get(name + "_less_planarity", 0.0), float(r) - extra)
            measure["planarity_share"] = max(measure.get("planarity_share", 0.0), extra)
        if "a" in checks and np.any(np.abs(J - ref) > scene.bound(area, pair[1]) + FLOOR * L ** 3 * powers):
            raise CheckFailed("a", "pair %r: J %r, reference %r, ratio to eps.L.A.L^k %r" % (pair, J.tolist(), ref.tolist(), ratio.tolist()))
    # ---- (b), (c) vertices
    for pair in scene.pairs:
        if pair in flagged or not ("b" in checks or "c" in checks):
            continue
        c, p = pair
        cp = scene.cell_planes(c)
        s_in = scene.pos64[p] @ cp[:, :3].T + cp[:, 3]
        deep = np.nonzero((s_in < -tau).all(1))[0]
        lst = by_pair.get(pair, [])
        fkeys = [k for _, kk in lst for k in _keys(frag_solid[kk][0]["pos"])]
        fpos = np.concatenate([frag_solid[kk][1] for _, kk in lst]) if lst else np.zeros((0, 3))
        fisl = np.concatenate([np.full(frag_solid[kk][1].shape[0], isl) for isl, kk in lst]) if lst else np.zeros(0, int)
        count = {}
        for k in fkeys:
            count[k] = count.get(k, 0) + 1
        in_keys = scene.keys[p]
        mult = {}
        for v in deep:
            mult[in_keys[v]] = mult.get(in_keys[v], 0) + 1
        if "b" in checks:
            for k, m in mult.items():
                if count.get(k, 0) != m:
                    raise CheckFailed("b", "pair %r: an input vertex deep inside the cell appears %d times in its fragments, not %d" % (pair, count.get(k, 0), m))
        if not lst:
            continue
        s = fpos @ cp[:, :3].T + cp[:, 3]
        all_in = set(in_keys)
        old = np.array([k in all_in for k in fkeys], bool)
        if measure is not None:
            measure["v"] = max(measure.get("v", 0.0), float(s.max() / (EPS * L)))
        if "b" in checks and old.any() and s[old].max() > tau:
            raise CheckFailed("b", "pair %r: a kept input vertex is %g outside the cell (tau %g)" % (pair, s[old].max(), tau))
        if "c" not in checks or old.all():
            continue
        sn, qn = s[~old], fpos[~old]
        if measure is not None:
            measure["v"] = max(measure.get("v", 0.0), float(np.abs(sn).min(1).max() / (EPS * L)))
        if sn.max() > tau:
            raise CheckFailed("c", "pair %r: a new vertex is %g outside the cell (tau %g)" % (pair, sn.max(), tau))
        on = (np.abs(sn) <= tau).sum(1)
        if on.min() == 0:
            raise CheckFailed("c", "pair %r: a new vertex lies %g from the nearest cell plane (tau %g)" % (pair, np.abs(sn).min(1).max(), tau))
        P, T, E = scene.pos64[p], scene.tris[p], scene.edges[p]
        # (only what reaches into the box of these vertices can be within tau of one of them; beyond tau the distance is not used)
        qlo, qhi = qn.min(0) - tau, qn.max(0) + tau
        E = E[(np.maximum(P[E[:, 0]], P[E[:, 1]]) >= qlo).all(1) & (np.minimum(P[E[:, 0]], P[E[:, 1]]) <= qhi).all(1)]
        Tn = T[(P[T].max(1) >= qlo).all(1) & (P[T].min(1) <= qhi).all(1)]
        d = dist_to_segments(qn, P[E[:, 0]], P[E[:, 1]]) if E.shape[0] else np.full(qn.shape[0], np.inf)
        far = np.nonzero(d > tau)[0]
        if far.size and Tn.shape[0]:
            d[far] = np.minimum(d[far], dist_to_triangles(qn[far], P[Tn[:, 0]], P[Tn[:, 1]], P[Tn[:, 2]]))
        if measure is not None and (on == 1).any():
            measure["v"] = max(measure.get("v", 0.0), float(d[on == 1].max() / (EPS * L)))
        if (on == 1).any() and d[on == 1].max() > tau:
            raise CheckFailed("c", "pair %r: a vertex cut by one plane lies %g from the input surface (tau %g)" % (pair, d[on == 1].max(), tau))
        corner = np.nonzero((on >= 2) & (d > tau))[0]
        if corner.size:
            w = winding_number(qn[corner], P[T[:, 0]], P[T[:, 1]], P[T[:, 2]])
            # outside S only as one of the two sheets of a lamina: its twin of the other sheet lies within tau of it.  Every
            # fragment in which a vertex passes this way is reported ("sheets"), for the caller to pin
            gap = np.array([np.sort(np.sqrt(((qn - qn[j]) ** 2).sum(1)))[1] if qn.shape[0] > 1 else np.inf for j in corner])
            twin = (np.abs(w - 1.0) > 0.5) & (np.abs(w) <= 0.5) & (gap <= tau)
            sheets.update((c, p, int(isl)) for isl in fisl[~old][corner][twin])
            bad = (np.abs(w - 1.0) > 0.5) & ~twin
            if bad.any():
                raise CheckFailed("c", "pair %r: a vertex on a cell edge or corner is neither on the input surface nor inside it (winding %r, "
                                  "nearest other new vertex %r)" % (pair, w[bad].tolist(), gap[bad].tolist()))
    return {"laminae": sorted(laminae), "negative": sorted(negative), "flat": sorted(flat), "sheets": sorted(sheets)}


# ------------------------------------------------------------------ the Convex side
K_E = 4.0      # (e): the Convex's integrals within K_E . eps . L . A . L^k      (largest oracle ratio 0.59: the Convex of cube)
K_N = 64.0     # (f): a face with D >= K_N . w has no plane either            (least elongated oracle face that misses plain tau: D / w = 210)
K_W = 4.0      # (f): a face narrower than K_W . tau has no plane               (widest oracle face that misses plain tau: 0.8 tau)


def face_widths(pos64, loops):
    """Per face: area / diameter, the width its vertices' roundings have to be small against for its Newell normal to mean anything."""
    out = np.zeros(len(loops))
    for j, l in enumerate(loops):
        q = pos64[l]
        c = q.mean(0)
        area = np.linalg.norm(np.cross(q - c, np.roll(q, -1, 0) - c).sum(0)) / 2.0
        diam = np.sqrt(((q[:, None, :] - q[None, :, :]) ** 2).sum(2).max())
        out[j] = area / diam if diam > 0 else 0.0
    return out


def newell_planes(solid, loops=None):
    """(F, 4) float64 unit planes n.x + d <= 0 of a solid's faces (Newell normal of every loop, through the loop's mean), and
    the loops."""
    p = np.asarray(solid["pos"], np.float32).reshape(-1, 3).astype(np.float64)
    loops = face_loops(solid, doubled=has_doubled_neighbour(solid)) if loops is None else loops
    out = []
    for l in loops:
        q = p[l]
        c = q.mean(0)
        n = np.cross(q - c, np.roll(q, -1, 0) - c).sum(0)
        n /= max(np.linalg.norm(n), 1e-300)
        out.append([n[0], n[1], n[2], -float(n @ c)])
    return np.array(out).reshape(-1, 4), loops


class ConvexScene:
    """Convex n C of every pair as a polytope of its own (convex_clip of the input Convex's faces by the cell's planes).  The
    planes of an input Convex are its faces' Newell planes, but for the faces narrower than K_W . tau: those have no plane
    (n_narrow_in counts them; a box has none, the refitted Convexes of a first level have some)."""

    def __init__(self, scene, convexes):
        self.scene, self.convexes = scene, convexes
        self.in_planes, self.n_narrow_in = [], 0
        for c in convexes:
            pl, loops = newell_planes(c)
            wide = face_widths(np.asarray(c["pos"], np.float32).reshape(-1, 3).astype(np.float64), loops) >= K_W * scene.tau
            self.n_narrow_in += int((~wide).sum())
            self.in_planes.append(pl[wide])
        self._body = {}

    def body(self, pair):
        if pair not in self._body:
            S = self.scene
            c, p = pair
            cp = S.cell_planes(c).copy()
            cp[:, 3] += cp[:, :3] @ S.origin
            faces = convex_clip(convex_faces(self.convexes[p], S.origin), cp)
            self._body[pair] = faces
        return self._body[pair]

    def all_planes(self, pair):
        return np.concatenate([self.scene.cell_planes(pair[0]), self.in_planes[pair[1]]])


def check_convex_clip(cscene, ev, measure=None):
    """(e): the Convex fragments of an event without refit against Convex n C.  Distances are Euclidean."""
    S = cscene.scene
    tau, L = S.tau, S.L
    ids = np.asarray(ev["frag_ids"]).reshape(-1, 3)
    for k, (c, p, i) in enumerate(ids.tolist()):
        body = cscene.body((c, p))
        if not body:
            raise CheckFailed("e", "pair %r has a Convex fragment and no Convex n C" % ((c, p),))
        rv = body_vertices(body)                  # relative to the origin
        sep = min(np.sort(np.sqrt(((rv - v) ** 2).sum(1)))[1] for v in rv)
        if sep < 100 * tau:
            raise CheckFailed("e-scene", "pair %r: two vertices of Convex n C lie %g apart (100 tau = %g): not a scene for this check" % ((c, p), sep, 100 * tau))
        f = fragment(ev, k, "conv")
        p64 = np.asarray(f["pos"], np.float32).reshape(-1, 3).astype(np.float64)
        tris = fan_triangles(f)
        J, area = surface_J(p64, tris, S.origin), surface_area(p64, tris)
        ratio = np.abs(J - body_J(body))[:4] / (EPS * L * area * np.array([1.0, L, L, L]))
        if measure is not None:
            measure["e0"] = max(measure.get("e0", 0.0), float(ratio[0]))
            measure["e1"] = max(measure.get("e1", 0.0), float(ratio[1:].max()))
        if ratio.max() > K_E:
            raise CheckFailed("e", "Convex of fragment %r: integrals off by %r of eps.L.A.L^k" % ((c, p, i), ratio.tolist()))
        # conditioning: the smallest angle between two planes that meet at a vertex of Convex n C
        pl = cscene.all_planes((c, p))
        s = (rv + S.origin) @ pl[:, :3].T + pl[:, 3]
        sin_min = 1.0
        for row in s:
            act = pl[np.abs(row) <= 1e-9 * L, :3]
            cr = np.linalg.norm(np.cross(act[:, None, :], act[None, :, :]), axis=2)
            cr = cr[cr > 1e-9]
            if cr.size:
                sin_min = min(sin_min, float(cr.min()))
        q = p64 - S.origin
        d = np.sqrt(((q[:, None, :] - rv[None, :, :]) ** 2).sum(2))
        haus = max(d.min(1).max(), d.min(0).max())
        if measure is not None:
            measure["e_h"] = max(measure.get("e_h", 0.0), float(haus * sin_min / (EPS * L)))
        if haus > tau / sin_min:
            raise CheckFailed("e", "Convex of fragment %r: Hausdorff distance %g to Convex n C (tau / sin = %g)" % ((c, p, i), haus, tau / sin_min))


def check_refit(cscene, ev, only=("cover", "inside", "tight"), measure=None, fragments=None):
    """(f): the refitted Convex of every fragment covers its Mesh fragment, lies inside Convex n C, and every one of its face
    planes is a plane of C, a plane of the input Convex, or touches a Mesh vertex: all within plain tau.
    Two kinds of face are excused from cover and tight, as faces whose Newell plane is their vertices' rounding, and counted:
      narrow: width w = area / diameter below K_W . tau.  Where four planes meet at a vertex within rounding the clip leaves such
              a face; its corners differ by their own roundings.
      needle: D >= K_N . w, D the distance of the farthest Mesh vertex from the face's centre.  Roundings of eps . L tilt the
              normal by eps . L / w, which moves the plane by (D / w) . eps . L out there.  On the oracle's events (limits 4 and
              12) the least elongated face that misses plain tau has D / w = 210; K_N is a quarter of that as a power of two.
    Their vertices are still held to 'inside'.  Returns (narrow, needles); the caller pins both per scene.
    fragments: only these fragment indices."""
    S = cscene.scene
    tau, L = S.tau, S.L
    ids = np.asarray(ev["frag_ids"]).reshape(-1, 3)
    narrow = needles = 0
    for k, (c, p, i) in enumerate(ids.tolist()):
        if fragments is not None and k not in fragments:
            continue
        f, m = fragment(ev, k, "conv"), fragment(ev, k, "mesh")
        fp, loops = newell_planes(f)
        if len(loops) < 4:
            raise CheckFailed("f-cover", "fragment %r has no Convex (%d vertices)" % ((c, p, i), len(f["pos"])))
        cpos = np.asarray(f["pos"], np.float32).reshape(-1, 3).astype(np.float64)
        mpos = np.asarray(m["pos"], np.float32).reshape(-1, 3).astype(np.float64)
        w = face_widths(cpos, loops)
        wide = w >= K_W * tau
        narrow += int((~wide).sum())
        sm = (mpos @ fp[:, :3].T + fp[:, 3]).max(0)            # per face: how far the farthest Mesh vertex is outside it
        D = np.array([np.sqrt(((mpos - cpos[l].mean(0)) ** 2).sum(1).max()) for l in loops])
        covered = wide & (D < K_N * w)                         # the faces held to cover and tight
        needles += int((wide & ~covered).sum())
        if measure is not None and (wide & (sm > tau)).any():
            measure["f_needle"] = min(measure.get("f_needle", np.inf), float((D / w)[wide & (sm > tau)].min()))
        if measure is not None:
            measure["f_cover"] = max(measure.get("f_cover", 0.0), float(sm[covered].max() / (EPS * L)))
            if (sm > tau)[D < K_N * w].any():
                measure["f_width"] = max(measure.get("f_width", 0.0), float(w[(sm > tau) & (D < K_N * w)].max() / tau))
        if "cover" in only and (sm[covered] > tau).any():
            j = int(np.argmax(np.where(covered, sm, -np.inf)))
            raise CheckFailed("f-cover", "fragment %r: a Mesh vertex lies %g outside face %d of its refitted Convex (tau %g)" % ((c, p, i), sm[j], j, tau))
        pl = cscene.all_planes((c, p))
        sc = cpos @ pl[:, :3].T + pl[:, 3]                     # (Convex vertices, planes of C and of the input Convex)
        if measure is not None:
            measure["f_inside"] = max(measure.get("f_inside", 0.0), float(sc.max() / (EPS * L)))
        if "inside" in only and sc.max() > tau:
            raise CheckFailed("f-inside", "fragment %r: a vertex of the refitted Convex lies %g outside Convex n C (tau %g)" % ((c, p, i), sc.max(), tau))
        if "tight" in only:
            for j, l in enumerate(loops):
                if not covered[j] or (np.abs(sc[l]).max(0) <= tau).any():      # no plane, or the whole face lies in one given plane
                    continue
                if measure is not None:
                    measure["f_tight"] = max(measure.get("f_tight", 0.0), float(-sm[j] / (EPS * L)))
                if -sm[j] > tau:
                    raise CheckFailed("f-tight", "fragment %r: face %d of the refitted Convex is no given plane and stays %g off the Mesh (tau %g)" % ((c, p, i), j, -sm[j], tau))
    return narrow, needles
