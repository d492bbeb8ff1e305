"""The checker of the cooked hulls (cook_dev.hip): float64 numpy and Python floats, written from the definition in include/surtr_hip.h;
it shares no code with the kernels and builds no hull of its own.  check_solid takes the input points of one solid and the engine's
answer for it and raises Refused(reason) at the first property that does not hold; the reasons, in the order they are checked:

  src           src is not strictly ascending, names no input point, or a point is no bit copy of the input point it names
  weld          the greedy weld of the definition, restated here: a hull vertex that the weld drops, or another n_welded
  loop          a loop names no vertex or has fewer than three entries
  loop-start    a loop does not start at its smallest vertex
  loop-repeat   a loop names a vertex twice
  edge-twice    a directed edge occurs twice
  edge-open     a directed edge without its reverse
  degree        a vertex on fewer than three faces
  euler         V - E + F != 2
  order         the faces are not ordered by (smallest vertex, second vertex)
  plane-normal  a plane's normal is not the Newell normal of its loop (float64, the stated order), rounded to float32: byte for byte
  plane-offset  ... or its offset is not the mid-range offset           (exact) or within one float32 ulp per component (GPU)
  planarity     a loop's own vertex farther than plane_tol + s_f from its plane
  outside       an INPUT point more than 2 plane_tol + weld_dist + s_f in front of a plane
  record        a field of the record is not what the returned arrays give

s_f = 2^-24 ((|n_x| + |n_y| + |n_z|) R + |d|), R the largest coordinate magnitude of the input, is the rounding of the written plane:
derived, not measured.  The factor 2 is one tolerance for the stopping rule of the hull and one for the merge.  weld_dist enters because a
welded point lies within weld_dist of a kept one and a unit normal moves its distance by no more than that; at weld_dist 0 the bound
is 2 plane_tol + s_f."""
import math

import numpy as np

F32 = np.float32
SKIPPED, FEW, DEGENERATE, NONFINITE, LARGE, FAILED, OVER_255 = 1, 2, 4, 8, 16, 32, 64
WITHHELD = SKIPPED | FEW | DEGENERATE | NONFINITE | LARGE | FAILED


class Refused(AssertionError):
    def __init__(self, reason, detail=""):
        AssertionError.__init__(self, "%s: %s" % (reason, detail))
        self.reason = reason


def need(cond, reason, detail=""):
    if not cond:
        raise Refused(reason, detail)


def solid_of(got, k):
    """Solid k of an answer of event_cook / pieces_cook / cook_points -> dict(record, points, src, loops, planes), copies."""
    r = got["records"][k]
    p0, f0, i0 = int(r["pt_off"]), int(r["face_off"]), int(r["idx_off"])
    polys = got["polygons"][f0:f0 + int(r["n_faces"])]
    idx = got["idx"][i0:i0 + int(r["n_idx"])]
    loops = [[int(v) for v in idx[int(p["index_base"]):int(p["index_base"]) + int(p["n_verts"])]] for p in polys]
    return dict(record=r.copy(), points=got["points"][p0:p0 + int(r["nv"])].copy(), src=got["src"][p0:p0 + int(r["nv"])].copy(),
                loops=loops, planes=polys["plane"].copy(), index_base=[int(p["index_base"]) for p in polys])


def solid_bytes(got, k):
    """What must not depend on the batch: everything of solid k but its three offsets."""
    s = solid_of(got, k)
    r = s["record"].copy()
    r["pt_off"] = r["face_off"] = r["idx_off"] = 0
    return r.tobytes() + s["points"].tobytes() + s["src"].tobytes() + s["planes"].tobytes() + repr((s["loops"], s["index_base"])).encode()


def weld(points, weld_dist):
    """The kept indices of the greedy weld, ascending (float64, ((dx dx + dy dy) + dz dz) <= weld_dist^2)."""
    p = np.asarray(points, np.float64)
    w2 = float(F32(weld_dist)) * float(F32(weld_dist))
    kept = []
    for i in range(p.shape[0]):
        if kept:
            d = p[i] - p[kept]
            if ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2] <= w2).any():
                continue
        kept.append(i)
    return kept


def newell(q):
    """Newell normal and mid-range offset of a loop of float64 positions, from q[0] -> four Python floats, or None (N zero)."""
    nx = ny = nz = 0.0
    for i in range(1, len(q) - 1):
        ax, ay, az = q[i][0] - q[0][0], q[i][1] - q[0][1], q[i][2] - q[0][2]
        bx, by, bz = q[i + 1][0] - q[0][0], q[i + 1][1] - q[0][1], q[i + 1][2] - q[0][2]
        nx, ny, nz = nx + (ay * bz - az * by), ny + (az * bx - ax * bz), nz + (ax * by - ay * bx)
    if nx == 0.0 and ny == 0.0 and nz == 0.0:
        return None
    ln = math.sqrt((nx * nx + ny * ny) + nz * nz)
    nx, ny, nz = nx / ln, ny / ln, nz / ln
    t = [(nx * p[0] + ny * p[1]) + nz * p[2] for p in q]
    return nx, ny, nz, -(max(t) + min(t)) / 2.0


def dist(planes, pts):
    """float64 distances [F, N] of points from float32 planes, ((n.x x + n.y y) + n.z z) + d."""
    pl, p = np.asarray(planes, np.float64), np.asarray(pts, np.float64)
    return ((pl[:, 0:1] * p[:, 0] + pl[:, 1:2] * p[:, 1]) + pl[:, 2:3] * p[:, 2]) + pl[:, 3:4]


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, F32)).astype(F32)).astype(np.float64)


def check_solid(inp, ans, weld_dist, plane_tol, exact):
    """Every property of the module's list on one solid that was not withheld.  exact: the emulation (bytes); else the MI355X."""
    inp = np.ascontiguousarray(inp, F32).reshape(-1, 3)
    r, pts, src, loops, planes = ans["record"], ans["points"], ans["src"].astype(np.int64), ans["loops"], np.asarray(ans["planes"], F32)
    nv, nf = pts.shape[0], len(loops)
    need(not int(r["status"]) & WITHHELD, "record", "status %d" % int(r["status"]))
    # src, copies
    need(src.shape[0] == nv and (np.diff(src) > 0).all() and (nv == 0 or (src[0] >= 0 and src[-1] < inp.shape[0])), "src", src)
    need(pts.dtype == F32 and pts.tobytes() == inp[src].tobytes(), "src", "a point is no bit copy")
    # weld
    kept = weld(inp, weld_dist)
    need(set(src.tolist()) <= set(kept), "weld", "a hull vertex the weld drops")
    need(int(r["n_welded"]) == inp.shape[0] - len(kept), "weld", (int(r["n_welded"]), inp.shape[0] - len(kept)))
    # loops
    for lp in loops:
        need(len(lp) >= 3 and all(0 <= v < nv for v in lp), "loop", lp)
        need(lp[0] == min(lp), "loop-start", lp)
        need(len(set(lp)) == len(lp), "loop-repeat", lp)
    edges = {}
    for lp in loops:
        for a, b in zip(lp, lp[1:] + lp[:1]):
            need((a, b) not in edges, "edge-twice", (a, b))
            edges[(a, b)] = 1
    for a, b in edges:
        need((b, a) in edges, "edge-open", (a, b))
    deg = np.bincount(np.asarray([v for lp in loops for v in lp], np.int64), minlength=nv)
    need((deg >= 3).all(), "degree", deg)
    need(nv - len(edges) // 2 + nf == 2, "euler", (nv, len(edges) // 2, nf))
    keys = [(lp[0], lp[1]) for lp in loops]
    need(keys == sorted(keys), "order", keys)
    base = np.concatenate([[0], np.cumsum([len(lp) for lp in loops])])[:-1]
    need(list(base) == list(ans["index_base"]), "record", "index_base")
    # planes: the definition restated, then the tolerances
    p64 = [[float(c) for c in p] for p in pts]
    want = np.zeros((nf, 4), F32)
    for f, lp in enumerate(loops):
        pl = newell([p64[v] for v in lp])
        need(pl is not None, "plane-normal", "a loop without area")
        want[f] = [F32(c) for c in pl]
    if exact:
        need(planes[:, :3].tobytes() == want[:, :3].tobytes(), "plane-normal", np.abs(planes - want).max())
        need(planes[:, 3].tobytes() == want[:, 3].tobytes(), "plane-offset", np.abs(planes - want).max())
    else:
        d = np.abs(planes.astype(np.float64) - want.astype(np.float64))
        tol = np.maximum(ulp32(planes), ulp32(want))
        print("planes off by at most %.3g ulp" % float((d / tol).max()))
        need((d[:, :3] <= tol[:, :3]).all(), "plane-normal", float((d / tol).max()))
        need((d[:, 3] <= tol[:, 3]).all(), "plane-offset", float((d / tol).max()))
    R = float(np.abs(inp).max())
    pl = planes.astype(np.float64)
    s_f = 2.0 ** -24 * ((np.abs(pl[:, 0]) + np.abs(pl[:, 1]) + np.abs(pl[:, 2])) * R + np.abs(pl[:, 3]))
    own = dist(planes, pts)
    plan = 0.0
    for f, lp in enumerate(loops):
        e = float(np.abs(own[f, lp]).max())
        plan = max(plan, e)
        need(e <= float(F32(plane_tol)) + s_f[f], "planarity", (f, e, s_f[f]))
    front = dist(planes, inp)
    room = 2.0 * float(F32(plane_tol)) + float(F32(weld_dist)) + s_f
    worst = (front - room[:, None]).max()
    print("nv_in %d nv %d faces %d: planarity %.3g, largest distance of an input point %.3g (room %.3g)"
          % (inp.shape[0], nv, nf, plan, float(front.max()), float(room.min())))
    need(worst <= 0.0, "outside", float(front.max()))
    # the record from the returned arrays
    conv = float(front.max())
    ext = (inp.max(0) - inp.min(0)).astype(F32).max()
    fields = dict(nv_in=inp.shape[0], nv=nv, n_faces=nf, n_idx=sum(map(len, loops)), max_loop=max(map(len, loops)))
    for k, v in fields.items():
        need(int(r[k]) == v, "record", (k, int(r[k]), v))
    need(int(r["status"]) == (OVER_255 if nv > 255 or nf > 255 else 0), "record", "status")
    need(r["extent"].tobytes() == F32(ext).tobytes() and r["reach"].tobytes() == F32(R).tobytes() and not r["reserved"].any(), "record", "extent / reach")
    for name, val in (("convexity", conv), ("planarity", plan)):
        if exact:
            need(r[name].tobytes() == F32(val).tobytes(), "record", (name, float(r[name]), val))
        else:
            need(abs(float(r[name]) - val) <= float(ulp32(val)) + 2.0 ** -40 * float(ext), "record", (name, float(r[name]), val))


def check_withheld(rec, n_in):
    """A withheld or skipped solid hands nothing out."""
    assert int(rec["status"]) & WITHHELD and int(rec["nv_in"]) == n_in
    for k in ("nv", "n_faces", "n_idx", "max_loop", "convexity", "planarity", "extent", "reach"):
        assert rec[k] == 0, (k, rec)


def check_flat(inp, plane_tol):
    """A DEGENERATE verdict on finite points is right only for a flat set.  The cooker gives it when no kept point stands more than
    plane_tol off the plane of its three start points: the whole set then lies in a slab of thickness 2 plane_tol, so its width
    along SOME direction is at most 2 plane_tol.  Checked here along the direction of least variance (numpy's SVD), which is that
    direction up to the noise of a nearly flat set.  -> the width."""
    p = np.asarray(inp, np.float64).reshape(-1, 3)
    c = p - p.mean(0)
    w = c @ np.linalg.svd(c)[2][2]
    width = float(w.max() - w.min())
    need(width <= 2.0 * float(F32(plane_tol)), "flat", width)
    return width


# ------------------------------------------------------------------ seven wrong answers made from a right one
def _copy(ans):
    return dict(record=ans["record"].copy(), points=ans["points"].copy(), src=ans["src"].copy(), loops=[list(lp) for lp in ans["loops"]],
                planes=ans["planes"].copy(), index_base=list(ans["index_base"]))


def _refresh(m, replane=()):
    """Keep the record's counts and index_base in step with the arrays, so that a mutation is refused for what it is."""
    for f in replane:
        pl = newell([[float(c) for c in m["points"][v]] for v in m["loops"][f]])
        m["planes"][f] = [F32(c) for c in pl]
    m["index_base"] = [int(x) for x in np.concatenate([[0], np.cumsum([len(lp) for lp in m["loops"]])])[:-1]]
    r = m["record"]
    r["nv"], r["n_faces"], r["n_idx"], r["max_loop"] = m["points"].shape[0], len(m["loops"]), sum(map(len, m["loops"])), max(map(len, m["loops"]))
    return m


def mutations(inp, ans, plane_tol):
    """-> [(name, wrong answer, the reason it must be refused for), ...].  ans: a right answer with an interior input point, a face of
    four or more vertices and a vertex on exactly three faces (the cube with its extra points)."""
    inp = np.ascontiguousarray(inp, F32).reshape(-1, 3)
    out = []
    m = _copy(ans); del m["loops"][1]; m["planes"] = np.delete(m["planes"], 1, 0)
    out.append(("a face dropped", _refresh(m), "edge-open"))
    m = _copy(ans); m["loops"][0] = [m["loops"][0][0]] + m["loops"][0][:0:-1]
    out.append(("a loop reversed", _refresh(m), "edge-twice"))
    # a hull vertex replaced by an interior input point (src stays ascending): the planes of its faces are no longer their loops'
    src = ans["src"].astype(np.int64)
    inside = [j for j in range(inp.shape[0]) if j not in set(src.tolist()) and j < src[-1] and (np.abs(inp[j]) < 0.5 * np.abs(inp).max()).all()]
    j = inside[0]
    k = int(np.searchsorted(src, j))
    m = _copy(ans); m["src"][k] = j; m["points"][k] = inp[j]
    out.append(("a hull vertex replaced by an interior point", _refresh(m), "plane-normal"))
    m = _copy(ans)
    pl = m["planes"][0].astype(np.float64)
    s_f = 2.0 ** -24 * ((abs(pl[0]) + abs(pl[1]) + abs(pl[2])) * float(np.abs(inp).max()) + abs(pl[3]))
    m["planes"][0][3] = F32(pl[3] - (3.0 * plane_tol + 3.0 * s_f))
    out.append(("d shifted", _refresh(m), "plane-offset"))
    m = _copy(ans); m["loops"][0].insert(2, m["loops"][0][1])
    out.append(("a vertex duplicated", _refresh(m), "loop-repeat"))
    # an extreme vertex (on exactly three faces) removed from the points and the loops, the hole closed by a triangle, planes anew
    deg = np.bincount(np.asarray([v for lp in ans["loops"] for v in lp]), minlength=src.shape[0])
    v = int(np.nonzero(deg == 3)[0][-1])
    m = _copy(ans)
    ring, touched = [], []
    for f, lp in enumerate(m["loops"]):
        if v in lp:
            i = lp.index(v)
            ring.append((lp[i - 1], lp[(i + 1) % len(lp)]))      # (before v, after v) on this face
            lp.remove(v); touched.append(f)
    nxt = {after: before for before, after in ring}              # a face now runs before -> after: the lid takes every such edge the other way
    a0 = ring[0][0]
    lid = [a0, nxt[a0], nxt[nxt[a0]]]
    assert all(len(m["loops"][f]) >= 3 for f in touched) and len(set(lid)) == 3
    ren = lambda x: x - 1 if x > v else x
    m["loops"] = [[ren(x) for x in lp] for lp in m["loops"]] + [[ren(x) for x in lid]]
    m["loops"] = [lp[lp.index(min(lp)):] + lp[:lp.index(min(lp))] for lp in m["loops"]]
    m["points"], m["src"] = np.delete(m["points"], v, 0), np.delete(m["src"], v)
    m["planes"] = np.concatenate([m["planes"], np.zeros((1, 4), F32)])
    order = sorted(range(len(m["loops"])), key=lambda f: (m["loops"][f][0], m["loops"][f][1]))
    m["loops"], m["planes"] = [m["loops"][f] for f in order], m["planes"][order]
    out.append(("an extreme vertex removed", _refresh(m, range(len(m["loops"]))), "outside"))
    m = _copy(ans); lp = m["loops"][0]; lp[0], lp[1] = lp[1], lp[0]
    out.append(("two entries of a loop swapped", _refresh(m), "loop-start"))
    return out
