"""A plain statement of the compound regrouping rule (Surtr::ApplyFracture's bind sets, MergeOutOfImpact,
ConvexOutOfSphere and HandleConvexIsland of the reference), for scenes whose faces are known by construction.

numpy, float64, no ctypes.  Solids come as explicit face loops (outward normals, counter-clockwise seen from outside): no ring
walk, no ExtractFaces.  Every pair of faces of a compound is compared (no sort, no window to break out of), and pieces are
joined by a union-find.  Next to the answer it returns how close every decision was to its threshold, so that a test can
require an input on which float32 and float64 cannot disagree.

The rule, per compound of two pieces or more.  Face = its points p0..pk-1, plane through p0, p1, p2: n = unit((p1-p0) x (p2-p0)),
d = -n.p0.  Faces i and j of two pieces touch when
    | |d_i| - |d_j| | <= 1e-3      (distance from the ORIGIN, not from each other)
    | 1 + n_i.n_j |  <  1e-4       (opposite normals)
    some point of i is strictly to the left of every edge of j, or (only then tried) some point of j of every edge of i:
    ((b - a) x (c - a)).n > 0 for every edge a->b of the polygon, n its own normal (VMACH::OnYourRight).
Pieces joined through touching faces stay together; a compound that falls apart keeps the group of its lowest piece, the other
groups are appended after all compounds in the order they were found (compound by compound, each by its lowest piece).
With `partial`, a fragment is first moved to compound 0 when no vertex of it is nearer than `radius` to `origin` (strictly) and
no point of the cloud lies in it (n.q + d <= 0 for every face); compounds emptied that way disappear."""
import numpy as np

EPS32 = 2.0 ** -23
WINDOW, OPPOSITE = 1e-3, 1e-4


class Margins:
    """Per kind of decision: the smallest distance to its threshold, the smallest ratio of that distance to the float32 rounding
    of the quantity (over the decisions that are not exactly on the threshold), and how many are exactly on it."""
    KINDS = ("window", "normal", "right", "vertex", "cloud")

    def __init__(self):
        self.margin = {k: np.inf for k in self.KINDS}
        self.ratio = {k: np.inf for k in self.KINDS}
        self.zeros = {k: 0 for k in self.KINDS}
        self.count = {k: 0 for k in self.KINDS}

    def take(self, kind, margin, rounding):
        m = np.abs(np.asarray(margin, np.float64)).ravel()
        if not m.size:
            return
        u = np.broadcast_to(np.asarray(rounding, np.float64), np.asarray(margin).shape).ravel()
        self.count[kind] += m.size
        self.margin[kind] = min(self.margin[kind], float(m.min()))
        nz = m > 0
        self.zeros[kind] += int(m.size - nz.sum())
        if nz.any():
            self.ratio[kind] = min(self.ratio[kind], float((m[nz] / np.maximum(u[nz], 1e-300)).min()))

    def smallest_ratio(self):
        return min(self.ratio.values())


def _unit(v):
    l = np.sqrt((v * v).sum(-1, keepdims=True))
    return np.where(l > 0, v / np.where(l > 0, l, 1.0), 0.0)


def _faces_of(piece):
    """[(points f64[k,3], n f64[3], d)] of the faces of three points or more; positions as float32 holds them."""
    pos = np.asarray(piece["pos"], np.float32).astype(np.float64)
    out = []
    for loop in piece["faces"]:
        if len(loop) < 3:
            continue
        P = pos[np.asarray(loop, np.int64)]
        n = _unit(np.cross(P[1] - P[0], P[2] - P[0]))
        out.append((P, n, float(-(n * P[0]).sum())))
    return pos, out


def out_of_sphere(piece, cloud, origin, radius, margins):
    pos, faces = _faces_of(piece)
    dist = np.sqrt(((origin[None, :] - pos) ** 2).sum(1))
    margins.take("vertex", dist - radius, EPS32 * np.maximum(dist, abs(radius)))
    if (dist < radius).any():
        return False
    if cloud.shape[0] == 0:
        return True
    inside = np.ones(cloud.shape[0], bool)
    for P, n, d in faces:
        s = cloud @ n + d
        margins.take("cloud", s, EPS32 * (np.abs(cloud).sum(1) + np.abs(P[0]).sum()))
        inside &= ~(s > 0)
    return not inside.any()


def _touch(A, nA, B, nB, margins):
    """A: one face f64[na,3]; B: k faces of nb points f64[k,nb,3] -> bool[k]."""
    eB = np.roll(B, -1, axis=1) - B                                   # k, nb, 3
    w = A[None, :, None, :] - B[:, None, :, :]                        # k, na, nb, 3
    v1 = (np.cross(eB[:, None, :, :], w) * nB[:, None, None, :]).sum(-1)
    margins.take("right", v1, EPS32 * np.sqrt((eB ** 2).sum(-1))[:, None, :] * np.sqrt((w ** 2).sum(-1)))
    eA = np.roll(A, -1, axis=0) - A                                   # na, 3
    w2 = B[:, :, None, :] - A[None, None, :, :]                       # k, nb, na, 3
    v2 = (np.cross(eA[None, None, :, :], w2) * nA[None, None, None, :]).sum(-1)
    margins.take("right", v2, EPS32 * np.sqrt((eA ** 2).sum(-1))[None, None, :] * np.sqrt((w2 ** 2).sum(-1)))
    return (v1 > 0).all(2).any(1) | (v2 > 0).all(2).any(1)


def _islands(local, solids, margins):
    """Groups of the pieces of one compound (each ascending, ordered by lowest piece) and its touching pairs of faces."""
    pc, ad, nm, l1, pts = [], [], [], [], []
    for p in local:
        for P, n, d in solids[p][1]:
            pc.append(p); ad.append(abs(d)); nm.append(_unit(n)); l1.append(np.abs(P[0]).sum()); pts.append(P)
    m = len(pc)
    pc, ad, nm, l1 = np.asarray(pc), np.asarray(ad), np.asarray(nm).reshape(m, 3), np.asarray(l1)
    cnt = np.asarray([P.shape[0] for P in pts])
    dense = {k: np.stack([pts[f] for f in np.nonzero(cnt == k)[0]]) for k in np.unique(cnt)}
    row = np.zeros(m, np.int64)
    for k in np.unique(cnt):
        row[cnt == k] = np.arange((cnt == k).sum())
    parent = {p: p for p in local}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    n_touch = 0
    for a in range(m - 1):
        js = np.arange(a + 1, m)
        js = js[pc[js] != pc[a]]            # (two faces of one piece: whatever the rule says of them joins nothing)
        diff = np.abs(ad[a] - ad[js])
        margins.take("window", diff - WINDOW, EPS32 * np.maximum(l1[a], l1[js]))
        js = js[~(diff > WINDOW)]
        val = np.abs(1.0 + nm[js] @ nm[a])
        margins.take("normal", val - OPPOSITE, EPS32)
        js = js[val < OPPOSITE]
        for k in np.unique(cnt[js]):
            jk = js[cnt[js] == k]
            hit = _touch(pts[a], nm[a], dense[k][row[jk]], nm[jk], margins)
            for j in jk[hit]:
                n_touch += 1
                ra, rb = find(pc[a]), find(pc[j])
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
    groups = {}
    for p in sorted(local):
        groups.setdefault(find(p), []).append(p)
    return [groups[r] for r in sorted(groups)], n_touch


def regroup(pieces, cells, n_outside=0, partial=False, cloud=None, origin=(0, 0, 0), radius=1.0):
    """pieces: [{'pos': f32[n,3], 'faces': [loop, ...]}], the first n_outside of them kept out of the event; cells: cell of every
    piece (those of the first n_outside are not read).  -> (compound_off u32, compound_piece i32, info) with info = {'margins':
    Margins, 'touching_face_pairs': n, 'out_of_sphere': n, 'out_pieces': [...]}."""
    n = len(pieces)
    margins = Margins()
    solids = [_faces_of(p) for p in pieces]
    bind = [list(range(n_outside))]
    for p in range(n_outside, n):
        if p == n_outside or cells[p] != cells[p - 1]:
            bind.append([])
        bind[-1].append(p)
    moved_out = []
    if partial:
        cl = np.zeros((0, 3)) if cloud is None else np.asarray(cloud, np.float32).astype(np.float64).reshape(-1, 3)
        org = np.asarray(origin, np.float32).astype(np.float64)
        rad = float(np.float32(radius))
        for i in range(1, len(bind)):
            out = [c for c in bind[i] if out_of_sphere(pieces[c], cl, org, rad, margins)]
            moved_out += out
            bind[i] = [c for c in bind[i] if c not in out]
            bind[0] = sorted(bind[0] + out)
        bind = bind[:1] + [b for b in bind[1:] if b]
    extra, n_touch = [], 0
    for i, local in enumerate(bind):
        if len(local) <= 1:
            continue
        groups, t = _islands(local, solids, margins)
        n_touch += t
        bind[i] = groups[0]
        extra += groups[1:]
    bind += extra
    off = np.cumsum([0] + [len(b) for b in bind]).astype(np.uint32)
    flat = np.asarray([p for b in bind for p in b], np.int32)
    return off, flat, {"margins": margins, "touching_face_pairs": n_touch, "out_of_sphere": len(moved_out), "out_pieces": moved_out}


# ---- solids from face loops ----------------------------------------------------------------------------------------------------
def rings_from_faces(n_vertices, faces):
    """Neighbour rings (off, nbr) from which a walk `next = the ring entry before the one we came from` returns the loops."""
    succ = [dict() for _ in range(n_vertices)]      # per vertex: face -> the vertex after it in that face
    pred = [dict() for _ in range(n_vertices)]
    for f, loop in enumerate(faces):
        k = len(loop)
        for q, v in enumerate(loop):
            succ[v][f] = loop[(q + 1) % k]
            pred[v][f] = loop[q - 1]
    off, nbr = [0], []
    for v in range(n_vertices):
        by_succ = {s: f for f, s in succ[v].items()}
        f = next(iter(succ[v]))
        for _ in succ[v]:
            nbr.append(succ[v][f])
            f = by_succ[pred[v][f]]
        off.append(len(nbr))
    return np.asarray(off, np.uint32), np.asarray(nbr, np.int32)


def solid(pos, faces):
    pos = np.asarray(pos, np.float32).reshape(-1, 3)
    off, nbr = rings_from_faces(pos.shape[0], faces)
    return {"pos": pos, "off": off, "nbr": nbr, "faces": [list(f) for f in faces]}


BOX_FACES = [[0, 3, 2, 1], [4, 5, 6, 7], [0, 1, 5, 4], [2, 3, 7, 6], [1, 2, 6, 5], [0, 4, 7, 3]]
_BOX_RINGS = rings_from_faces(8, BOX_FACES)


def box(lo, hi):
    (x0, y0, z0), (x1, y1, z1) = lo, hi
    pos = np.asarray([(x0, y0, z0), (x1, y0, z0), (x1, y1, z0), (x0, y1, z0), (x0, y0, z1), (x1, y0, z1), (x1, y1, z1), (x0, y1, z1)], np.float32)
    return {"pos": pos, "off": _BOX_RINGS[0], "nbr": _BOX_RINGS[1], "faces": BOX_FACES}


def moved(s, matrix=None, shift=(0, 0, 0)):
    """The solid rotated (proper rotation: loops keep their sense) and shifted, in float64, rounded once to float32."""
    p = np.asarray(s["pos"], np.float64)
    if matrix is not None:
        p = p @ np.asarray(matrix, np.float64).T
    return dict(s, pos=(p + np.asarray(shift, np.float64)).astype(np.float32))


def prism(n, radius=1.0, z0=0.0, z1=1.0):
    """Regular n-gon prism about the z axis: 2n vertices of degree 3 (6n half-edges), two n-gon caps and n quads."""
    t = 2.0 * np.pi * np.arange(n) / n
    ring = np.stack([radius * np.cos(t), radius * np.sin(t)], 1)
    pos = np.concatenate([np.concatenate([ring, np.full((n, 1), z0)], 1), np.concatenate([ring, np.full((n, 1), z1)], 1)])
    faces = [[0] + list(range(n - 1, 0, -1)), list(range(n, 2 * n))]
    faces += [[k, (k + 1) % n, n + (k + 1) % n, n + k] for k in range(n)]
    return solid(pos, faces)


def is_dyadic(arrays, squares=False, finest=20):
    """Every coordinate is, axis by axis, a small integer times one power of two (down to 2^-finest), small enough that a sum of
    three products of two differences along different axes (with `squares`: along any axes) is exact in float32.  With
    axis-aligned planes every quantity of the rule but the square root of the sphere test is then exact."""
    a = np.concatenate([np.asarray(x, np.float64).reshape(-1, 3) for x in arrays])
    size = []
    for c in range(3):
        for q in range(finest + 1):
            s = a[:, c] * 2.0 ** q
            if np.array_equal(s, np.round(s)):
                size.append(float(np.abs(s).max()))
                break
        else:
            return False
    pairs = [(x, y) for x in range(3) for y in range(3) if squares or x != y]
    return all(3 * (2 * size[x]) * (2 * size[y]) <= 2 ** 24 for x, y in pairs)
