"""A float64 checker for surtr_scene_contacts that runs no GJK (include/surtr_hip.h carries the definition).

Inputs: the world vertices of every piece come from a second engine after scene_apply_poses + download_piece (the method of
test_scene_upkeep.reference_boxes), so they are the floats the definition names.  The predicates of the broad and mid phases run in
numpy on those boxes: the same exact comparisons on the same floats, so candidate counts and pair sets must be EQUAL.

Overlap is decided by a separating-axis test over face normals and edge x edge axes (faces from scipy.spatial.ConvexHull); the
reference distance of a separated pair is the minimum over vertex-triangle (both ways) and edge-edge feature pairs.  A reported record
is checked by a CERTIFICATE that proves its distance without computing it: with tol = 16 * 2^-24 * (S + margin) -- three float roundings
of a coordinate and of a unit normal inside a dot product, with room; derived, not measured --
    point_a satisfies every Qhull half-space of A within tol, point_b those of B;
    |point_b - point_a - distance * normal| <= tol per coordinate;    | |normal| - 1 | <= 4 * 2^-24;
    normal . (v - point_a) <= tol for every vertex v of A;            normal . (w - point_b) >= -tol for every vertex w of B.
Which pairs must appear: every pair with reference distance <= margin - k must, no pair with distance >= margin + k may, k = 1e-3 L
with L the scene's extent.  The band between is a condition with cap zero, asserted on the reference before the engine is asked
(Reference.classes), and so is a depth or distance within k of the OVERLAP threshold -- but for the pairs a test names as touching,
where either status is accepted."""
import numpy as np
from scipy.spatial import ConvexHull

from surtr_amd import engine

EPS = 2.0 ** -24


class Solid:
    def __init__(self, pos):
        self.pos = np.asarray(pos, np.float32).reshape(-1, 3).astype(np.float64)
        h = ConvexHull(self.pos)
        self.eq = h.equations                      # n . x + d <= 0 inside, |n| = 1
        self.tri = h.simplices
        e = np.concatenate([self.tri[:, [0, 1]], self.tri[:, [1, 2]], self.tri[:, [2, 0]]])
        self.edge = np.unique(np.sort(e, 1), axis=0)
        self.S = np.abs(self.pos).max()


def boxes_near(lo_a, hi_a, lo_b, hi_b, margin):
    """The broad / mid phase predicate: float records, compared in double."""
    m = np.float64(np.float32(margin))
    la, ha, lb, hb = (np.asarray(x, np.float32).astype(np.float64) for x in (lo_a, hi_a, lo_b, hi_b))
    return bool(((la - hb <= m) & (lb - ha <= m)).all())


def sat_gap(A, B):
    """max over the axes (face normals of both, edge x edge) of the gap between the projections: > 0 separated by at least that,
    < 0 overlapping with that depth along the best axis."""
    da = A.pos[A.edge[:, 1]] - A.pos[A.edge[:, 0]]
    db = B.pos[B.edge[:, 1]] - B.pos[B.edge[:, 0]]
    cr = np.cross(da[:, None, :], db[None, :, :]).reshape(-1, 3)
    ln = np.linalg.norm(cr, axis=1)
    scale = max(np.linalg.norm(da, axis=1).max() * np.linalg.norm(db, axis=1).max(), 1e-300)
    cr = cr[ln > 1e-9 * scale] / ln[ln > 1e-9 * scale][:, None]
    ax = np.concatenate([A.eq[:, :3], B.eq[:, :3], cr])
    pa, pb = A.pos @ ax.T, B.pos @ ax.T
    return float(np.maximum(pb.min(0) - pa.max(0), pa.min(0) - pb.max(0)).max())


def _seg_seg(p1, q1, p2, q2):
    """Distances of every segment of the first set to every one of the second (closest points of two segments, clamped)."""
    d1, d2 = (q1 - p1)[:, None, :], (q2 - p2)[None, :, :]
    r = p1[:, None, :] - p2[None, :, :]
    a, e, f = (d1 * d1).sum(-1), (d2 * d2).sum(-1), (d2 * r).sum(-1)
    b, c = (d1 * d2).sum(-1), (d1 * r).sum(-1)
    den = a * e - b * b
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(den > 0, np.clip((b * f - c * e) / np.where(den > 0, den, 1), 0, 1), 0.0)
        t = (b * s + f) / e
        s = np.where(t < 0, np.clip(-c / a, 0, 1), np.where(t > 1, np.clip((b - c) / a, 0, 1), s))
        t = np.clip(t, 0, 1)
    x = r + d1 * s[..., None] - d2 * t[..., None]
    return np.sqrt((x * x).sum(-1))


def _vert_tri(P, T):
    """Distances of the points P to the triangles T (k, 3, 3) where the foot of the perpendicular lies inside; inf elsewhere (the
    edges are covered by the edge-edge pairs)."""
    a, b, c = T[:, 0], T[:, 1], T[:, 2]
    n = np.cross(b - a, c - a)
    ln = np.linalg.norm(n, axis=1)
    ok = ln > 0
    n = n[ok] / ln[ok][:, None]
    a, b, c = a[ok], b[ok], c[ok]
    h = ((P[:, None, :] - a[None]) * n[None]).sum(-1)
    foot = P[:, None, :] - h[..., None] * n[None]
    inside = np.ones(h.shape, bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross((v - u)[None], foot - u[None]) * n[None]).sum(-1) >= 0
    return np.where(inside, np.abs(h), np.inf)


def feature_distance(A, B):
    d = _seg_seg(A.pos[A.edge[:, 0]], A.pos[A.edge[:, 1]], B.pos[B.edge[:, 0]], B.pos[B.edge[:, 1]]).min()
    d = min(d, _vert_tri(A.pos, B.pos[B.tri]).min(), _vert_tri(B.pos, A.pos[A.tri]).min())
    return float(d)


class Reference:
    """The reference side of one scene at one margin, computed once and left unchanged."""

    def __init__(self, positions, table, margin, nonfinite=()):
        """positions: the world float positions of every piece's Convex; table: the compound table."""
        self.margin = float(np.float32(margin))
        self.table = np.asarray(table, np.int64)
        self.n, self.nc = len(positions), len(table) - 1
        self.comp = np.repeat(np.arange(self.nc), np.diff(self.table))
        pos = [np.asarray(p, np.float32).reshape(-1, 3) for p in positions]
        fin = [np.where(np.isfinite(p), p, np.nan) for p in pos]
        self.plo = np.array([np.nanmin(p, 0) for p in fin], np.float32)
        self.phi = np.array([np.nanmax(p, 0) for p in fin], np.float32)
        bad = np.array([not np.isfinite(p).all() for p in pos])
        self.blo = np.array([self.plo[self.table[c]:self.table[c + 1]].min(0) for c in range(self.nc)])
        self.bhi = np.array([self.phi[self.table[c]:self.table[c + 1]].max(0) for c in range(self.nc)])
        self.bbad = np.array([bad[self.table[c]:self.table[c + 1]].any() for c in range(self.nc)])
        assert sorted(np.flatnonzero(self.bbad)) == sorted(nonfinite)
        # the broad phase in bulk (the same comparisons, vectorised), the mid phase pair by pair
        m = np.float64(np.float32(margin))
        lo, hi = self.blo.astype(np.float64), self.bhi.astype(np.float64)
        near = ((lo[:, None, :] - hi[None, :, :] <= m) & (lo[None, :, :] - hi[:, None, :] <= m)).all(-1)
        near &= ~self.bbad[:, None] & ~self.bbad[None, :]
        self.body_pairs = [(a, b) for a in range(self.nc) for b in range(a + 1, self.nc) if near[a, b]]
        pp = []
        for a, b in self.body_pairs:
            for p in range(self.table[a], self.table[a + 1]):
                for q in range(self.table[b], self.table[b + 1]):
                    if boxes_near(self.plo[p], self.phi[p], self.plo[q], self.phi[q], margin):
                        pp.append((p, q))
        self.piece_pairs = sorted(pp)
        used = sorted({p for pq in self.piece_pairs for p in pq})
        self.solid = {p: Solid(pos[p]) for p in used}
        ext = [pos[p] for p in range(self.n) if not bad[p]]
        self.L = float((np.max([p.max(0) for p in ext], 0) - np.min([p.min(0) for p in ext], 0)).max())
        self.k = 1e-3 * self.L
        self.gap = {}          # per candidate piece pair: > 0 the distance of a separated pair, < 0 minus the depth of an overlapping one
        for p, q in self.piece_pairs:
            g = sat_gap(self.solid[p], self.solid[q])
            self.gap[(p, q)] = feature_distance(self.solid[p], self.solid[q]) if g > 0 else g

    def threshold(self, p, q):
        return EPS * max(self.solid[p].S, self.solid[q].S)

    def tol(self, p, q):
        return 16 * EPS * (max(self.solid[p].S, self.solid[q].S) + self.margin)

    def classes(self, touching=()):
        """-> {pair: 'overlap' | 'near' | 'far' | 'touching'}.  Asserts the cap-zero conditions: no pair in the band about the margin,
        none within k of the OVERLAP threshold but the named touching ones."""
        out = {}
        for pq, g in self.gap.items():
            if pq in touching:
                assert abs(g) <= self.tol(*pq), (pq, g)
                out[pq] = "touching"
                continue
            assert abs(g - self.threshold(*pq)) >= self.k, ("a pair within k of the OVERLAP threshold", pq, g)
            assert abs(g - self.margin) >= self.k, ("a pair in the band about the margin", pq, g, self.margin)
            out[pq] = "overlap" if g < 0 else ("near" if g <= self.margin - self.k else "far")
        return out


def check_certificate(ref, r):
    """One reported record proves itself."""
    p, q = int(r["piece_a"]), int(r["piece_b"])
    A, B = ref.solid[p], ref.solid[q]
    tol = ref.tol(p, q)
    pa, pb, n, d = (np.asarray(r[k], np.float64) for k in ("point_a", "point_b", "normal", "distance"))
    assert (A.eq[:, :3] @ pa + A.eq[:, 3] <= tol).all(), ("point_a off its hull", p, q)
    assert (B.eq[:, :3] @ pb + B.eq[:, 3] <= tol).all(), ("point_b off its hull", p, q)
    if r["status"] & engine.CONTACT_OVERLAP:
        assert d == 0 and (n == 0).all() and (pa == pb).all(), (p, q)
        return
    assert d > 0
    assert (np.abs(pb - pa - d * n) <= tol).all(), ("witnesses, distance and normal disagree", p, q)
    assert abs(np.linalg.norm(n) - 1) <= 4 * EPS, ("normal not unit", p, q)
    assert ((A.pos - pa) @ n <= tol).all(), ("normal does not support A", p, q)
    assert ((B.pos - pb) @ n >= -tol).all(), ("normal does not support B", p, q)


def check_records(ref, rec, touching=()):
    """Everything about the records of one call: fields, order, the must / must-not sets, every certificate."""
    cls = ref.classes(touching)
    rec = np.asarray(rec)
    assert rec.dtype == engine.CONTACT_DTYPE
    keys = [(int(r["piece_a"]), int(r["piece_b"])) for r in rec]
    assert keys == sorted(set(keys)), "records ascend by (piece_a, piece_b), each pair once"
    for r, pq in zip(rec, keys):
        assert pq in cls, ("not a candidate of the mid phase", pq)
        assert int(r["body_a"]) == ref.comp[pq[0]] and int(r["body_b"]) == ref.comp[pq[1]] and r["body_a"] < r["body_b"], pq
        assert r["reserved"] == 0 and r["distance"] >= 0 and not (r["status"] & ~np.uint32(engine.CONTACT_OVERLAP | engine.CONTACT_ITER)), pq
        assert not (r["status"] & engine.CONTACT_ITER), ("iteration cap reached", pq)
        assert cls[pq] != "far", ("reported although the reference distance is beyond the margin", pq, ref.gap[pq])
        if cls[pq] == "overlap":
            assert r["status"] & engine.CONTACT_OVERLAP, pq
        elif cls[pq] == "near":
            assert not (r["status"] & engine.CONTACT_OVERLAP), pq
            assert abs(float(r["distance"]) - ref.gap[pq]) <= ref.tol(*pq), (pq, r["distance"], ref.gap[pq])
        else:
            assert (r["status"] & engine.CONTACT_OVERLAP) or r["distance"] <= ref.tol(*pq), pq
        check_certificate(ref, r)
    missing = [pq for pq, c in cls.items() if c != "far" and pq not in set(keys)]
    assert not missing, ("pairs within the margin that were not reported", missing)


def check_totals(ref, h):
    assert int(h["n_bodies"]) == ref.nc and int(h["n_pieces"]) == ref.n
    assert int(h["n_body_pairs"]) == len(ref.body_pairs) and int(h["n_piece_pairs"]) == len(ref.piece_pairs), \
        (int(h["n_body_pairs"]), len(ref.body_pairs), int(h["n_piece_pairs"]), len(ref.piece_pairs))
    assert int(h["lists"]) == 0 and not np.asarray(h["reserved"]).any()
