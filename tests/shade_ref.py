"""The definition of the lit render buffers (include/surtr_hip.h, "lit render buffers") restated in plain Python.  Nothing here runs the
code under test: the faces come from a sequential walk of the rings (which is what Poly::ExtractFaces does), the Newell sum of a loop is
math.fsum over float64 terms, and the common-face rule and the fallback are written out.

shade_solid(pos, off, nbr, idx) -> dict
    whole       the fragment takes the fallback as a whole (its successor is no permutation of its half-edges)
    n_faces     loops (0 when whole)
    loops       [[vertex, ...], ...] in face order, each from its smallest vertex (its leading half-edge)
    normal64    float64[n_faces, 3]: N / sqrt(N.N), or zero (N.N zero or not finite, k < 3)
    bound       float64[n_faces]: e = k * max_c(sum_i |T_i|_c) / max_c |N_c| * 2^-52, the room a float64 sum in ANY order has around
                the exact sum, relative to the normal's largest component.  Where every term is exactly zero (a loop on one line, a
                triangle with two corners in one place) the absolute room k * sum |T_i| * 2^-52 is zero and e = 0; where N is zero by
                cancellation of terms that are not, e = inf
    flat        the faces whose N is exactly zero
    tri_face    uint32[n_tri]: the face of every triangle of idx, NO_FACE on the fallback
    tri_normal  float64[n_tri, 3]: the normal every vertex of the triangle carries
    per_triangle  some triangle (or the whole fragment) took the fallback
"""
import math

import numpy as np

NO_FACE = 0xFFFFFFFF
PER_TRIANGLE = 1


def _cross(a, b):
    return (a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0])


def _sub(a, b):
    return (a[0] - b[0], a[1] - b[1], a[2] - b[2])


def _unit(N):
    nn = (N[0] * N[0] + N[1] * N[1]) + N[2] * N[2]
    if not (nn > 0.0) or not math.isfinite(nn):
        return (0.0, 0.0, 0.0)
    ln = math.sqrt(nn)
    return (N[0] / ln, N[1] / ln, N[2] / ln)


def successor(off, nbr, nv):
    """Half-edge id = position in the packed rings; next(a -> b) = the slot before a in ring(b).  -> (org, nxt) or None when the
    successor is no permutation: an entry names no vertex, a link lacks its way back, a ring lists a neighbour twice."""
    off = [int(x) for x in off]
    nbr = [int(x) for x in nbr]
    H = off[nv]
    if any(off[v + 1] < off[v] for v in range(nv)) or H != len(nbr) or off[0] != 0:
        return None
    org = [0] * H
    for v in range(nv):
        for e in range(off[v], off[v + 1]):
            org[e] = v
    nxt, seen = [0] * H, [0] * H
    for e in range(H):
        a, b = org[e], nbr[e]
        if not 0 <= b < nv:
            return None
        ring = nbr[off[b]:off[b + 1]]
        if a not in ring:
            return None
        k = ring.index(a)
        nxt[e] = off[b] + (len(ring) - 1 if k == 0 else k - 1)
        seen[nxt[e]] += 1
    if any(c != 1 for c in seen):
        return None
    return org, nxt


def walk_faces(org, nxt):
    """The sequential walk: half-edges in id order, each unvisited one leads a new loop.  -> (loops of half-edge ids, face of every
    half-edge)."""
    H = len(nxt)
    face = [-1] * H
    loops = []
    for e in range(H):
        if face[e] >= 0:
            continue
        loop, x = [], e
        while face[x] < 0:
            face[x] = len(loops)
            loop.append(x)
            x = nxt[x]
        assert x == e
        loops.append(loop)
    return loops, face


def loop_normal(q):
    """q: the loop's positions as float64 triples -> (unit normal or zero, the bound e)."""
    k = len(q)
    T = [_cross(_sub(q[i], q[0]), _sub(q[i + 1], q[0])) for i in range(1, k - 1)]
    N = tuple(math.fsum(t[c] for t in T) for c in range(3))
    top = max(abs(c) for c in N)
    mass = max(math.fsum(abs(t[c]) for t in T) for c in range(3)) if T else 0.0
    # (every term exactly zero: the sum is exactly zero in any order, and the quotient 0 / 0 stands for "no error at all")
    bound = 0.0 if mass == 0.0 else (k * mass / top * 2.0 ** -52 if top > 0.0 and math.isfinite(top) else math.inf)
    return (_unit(N) if k >= 3 else (0.0, 0.0, 0.0)), bound


_CACHE = {}


def shade_solid(pos, off, nbr, idx):
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    off, nbr, idx = np.ascontiguousarray(off, np.uint32), np.ascontiguousarray(nbr, np.int32), np.ascontiguousarray(idx, np.uint32)
    key = (pos.tobytes(), off.tobytes(), nbr.tobytes(), idx.tobytes())
    if key not in _CACHE:
        _CACHE[key] = _shade_solid(pos, off, nbr, idx)
    return _CACHE[key]


def _shade_solid(pos, off, nbr, idx):
    nv = pos.shape[0]
    P = [tuple(float(c) for c in p) for p in pos]
    tris = [tuple(int(x) for x in idx[3 * t:3 * t + 3]) for t in range(idx.shape[0] // 3)]
    out = dict(whole=True, n_faces=0, loops=[], normal64=np.zeros((0, 3)), bound=np.zeros(0), per_triangle=False, flat=[])
    faces_at = None
    topo = successor(off, nbr, nv)
    if topo is not None:
        org, nxt = topo
        loops, face = walk_faces(org, nxt)
        normals, bounds = [], []
        for lp in loops:
            n, b = loop_normal([P[org[e]] for e in lp])
            normals.append(n); bounds.append(b)
        faces_at = [set() for _ in range(nv)]
        for e, f in enumerate(face):
            faces_at[org[e]].add(f)
        out.update(whole=False, n_faces=len(loops), loops=[[org[e] for e in lp] for lp in loops],
                   normal64=np.asarray(normals, np.float64).reshape(-1, 3), bound=np.asarray(bounds, np.float64),
                   flat=[f for f, n in enumerate(normals) if n == (0.0, 0.0, 0.0)])
    tf = np.full(len(tris), NO_FACE, np.uint32)
    tn = np.zeros((len(tris), 3))
    for t, (a, b, c) in enumerate(tris):
        common = (faces_at[a] & faces_at[b] & faces_at[c]) if faces_at is not None else set()
        if common:
            tf[t] = min(common)
            tn[t] = out["normal64"][tf[t]]
        else:
            tn[t] = _unit(_cross(_sub(P[b], P[a]), _sub(P[c], P[a])))
            out["per_triangle"] = True
    if out["whole"]:
        out["per_triangle"] = True
    out.update(tri_face=tf, tri_normal=tn)
    return out
