"""Runs cases through the compiled reference (oracle/_ref/ref_driver, `make -C oracle ref`) and through the oracle, and compares.

TEST INFRASTRUCTURE ONLY, like oracle.py.  A case is a dict {"name", "op", inputs...}; a result is a dict of arrays, or
{"aborted": True} where the reference indexed outside a vector (-D_GLIBCXX_ASSERTIONS), {"threw": True} where it threw,
{"failed": reason} for anything else (a signal, the time limit).  The driver runs as a child process under a time limit;
an abort ends that child and the cases after it go to a fresh one.

  ops:  clip(solid, planes) -> solid        faces(solid) -> fo, fi            render(solid, convex, colour) -> vnc, idx
        neighbours(pos, tris) -> off, nbr   moments(solid) -> vol, centre     transform(solid, world) -> pos
        kdop(points, normals, ach, max_axis_scale, gap_inv) -> planes         refit(convex, mesh, limit) -> solid
        hull(points, limit) -> normals

TOPOLOGY holds, per op, the result keys compared with array_equal; COORDS the float keys.  compare() checks topology exactly
and returns the largest difference of the coordinates from the reference's (0.0: equal as numbers, every one of them)."""
import os
import signal
import struct
import subprocess
import tempfile

import numpy as np

from . import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
REFERENCE = os.environ.get("SURTR_REFERENCE", "/root/reference")
DRIVER = os.path.join(HERE, "_ref", "ref_driver")
OPS = {"clip": 1, "faces": 2, "render": 3, "neighbours": 4, "moments": 5, "transform": 6, "kdop": 7, "refit": 8, "hull": 9}
TOPOLOGY = {"clip": ("off", "nbr"), "faces": ("fo", "fi"), "render": ("idx",), "neighbours": ("off", "nbr"), "moments": (),
            "transform": (), "kdop": (), "refit": ("off", "nbr"), "hull": ()}
COORDS = {"clip": ("pos",), "faces": (), "render": ("vnc",), "neighbours": (), "moments": ("vol", "centre"), "transform": ("pos",),
          "kdop": ("planes",), "refit": ("pos",), "hull": ("normals",)}


def reference_present():
    return os.path.isdir(os.path.join(REFERENCE, "Src"))


def build():
    subprocess.check_call(["make", "-s", "-C", HERE, "ref", "REFERENCE=" + REFERENCE])
    return DRIVER


# ------------------------------------------------------------------------------------------------------------------ the batch file
def _f32(a):
    return np.ascontiguousarray(a, np.float32).tobytes()


def _solid_bytes(s):
    pos = np.ascontiguousarray(s["pos"], np.float32).reshape(-1, 3)
    off = np.ascontiguousarray(s["off"], np.uint32)
    nbr = np.ascontiguousarray(s["nbr"], np.int32)
    assert off.shape[0] == pos.shape[0] + 1 and off[-1] == nbr.shape[0]
    return struct.pack("<I", pos.shape[0]) + pos.tobytes() + off.tobytes() + nbr.tobytes()


def _points_bytes(p):
    p = np.ascontiguousarray(p, np.float32).reshape(-1, 3)
    return struct.pack("<I", p.shape[0]) + p.tobytes()


def _case_bytes(c):
    op = c["op"]
    b = struct.pack("<i", OPS[op])
    if op == "clip":
        pl = np.ascontiguousarray(c["planes"], np.float32).reshape(-1, 4)
        return b + _solid_bytes(c["solid"]) + struct.pack("<I", pl.shape[0]) + pl.tobytes()
    if op in ("faces", "moments"):
        return b + _solid_bytes(c["solid"])
    if op == "render":
        return b + _solid_bytes(c["solid"]) + struct.pack("<i", int(c["convex"])) + _f32(c["colour"])
    if op == "neighbours":
        t = np.ascontiguousarray(c["tris"], np.int32).reshape(-1)
        return b + _points_bytes(c["pos"]) + struct.pack("<I", t.shape[0]) + t.tobytes()
    if op == "transform":
        return b + _solid_bytes(c["solid"]) + _f32(np.asarray(c["world"], np.float32).reshape(16))
    if op == "kdop":
        return (b + _points_bytes(c["points"]) + _points_bytes(c["normals"]) + struct.pack("<i", int(c["ach"]))
                + struct.pack("<d", float(c["max_axis_scale"])) + struct.pack("<f", float(c["gap_inv"])))
    if op == "refit":
        return b + _solid_bytes(c["convex"]) + _solid_bytes(c["mesh"]) + struct.pack("<i", int(c["limit"]))
    if op == "hull":
        return b + _points_bytes(c["points"]) + struct.pack("<i", int(c["limit"]))
    raise KeyError(op)


class _Reader:
    def __init__(self, raw):
        self.raw, self.at = raw, 0

    def take(self, dtype, n=1):
        nb = np.dtype(dtype).itemsize * n
        if self.at + nb > len(self.raw):
            raise EOFError
        a = np.frombuffer(self.raw, dtype, n, self.at).copy()
        self.at += nb
        return a

    def solid(self):
        nv = int(self.take(np.uint32)[0])
        pos = self.take(np.float32, 3 * nv).reshape(-1, 3)
        off = self.take(np.uint32, nv + 1)
        return {"pos": pos, "off": off, "nbr": self.take(np.int32, int(off[-1]))}

    def lists(self):
        n = int(self.take(np.uint32)[0])
        sizes = self.take(np.uint32, n)
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        return off, self.take(np.int32, int(off[-1]))


def _read_result(r, op):
    got_op, status = (int(v) for v in r.take(np.int32, 2))
    assert got_op == OPS[op], (got_op, op)
    if status == 2:
        return {"threw": True}
    if op in ("clip", "refit"):
        return r.solid()
    if op == "faces":
        fo, fi = r.lists()
        return {"fo": fo, "fi": fi}
    if op == "render":
        nv = int(r.take(np.uint32)[0])
        vnc = r.take(np.float32, 9 * nv).reshape(-1, 9)
        ni = int(r.take(np.uint32)[0])
        return {"vnc": vnc, "idx": r.take(np.uint32, ni)}
    if op == "neighbours":
        off, nbr = r.lists()
        return {"off": off, "nbr": nbr}
    if op == "moments":
        vol = r.take(np.float64)
        return {"vol": vol, "centre": r.take(np.float32, 3).astype(np.float64)}
    if op == "transform":
        return {"pos": r.solid()["pos"]}
    if op == "kdop":
        k = int(r.take(np.uint32)[0])
        return {"planes": r.take(np.float32, 8 * k).reshape(-1, 4)}
    if op == "hull":
        k = int(r.take(np.uint32)[0])
        return {"normals": r.take(np.float32, 3 * k).reshape(-1, 3)}
    raise KeyError(op)


def run(cases, seconds=60, driver=None):
    """The compiled reference's result for every case, in order."""
    driver = driver or DRIVER
    results = [None] * len(cases)
    left = list(range(len(cases)))
    with tempfile.TemporaryDirectory() as tmp:
        while left:
            fin, fout = os.path.join(tmp, "batch"), os.path.join(tmp, "result")
            with open(fin, "wb") as f:
                f.write(struct.pack("<I", len(left)) + b"".join(_case_bytes(cases[i]) for i in left))
            if os.path.exists(fout):
                os.remove(fout)
            try:
                rc = subprocess.run([driver, fin, fout], capture_output=True, timeout=seconds).returncode
            except subprocess.TimeoutExpired:
                rc = "time limit"
            raw = open(fout, "rb").read() if os.path.exists(fout) else b""
            r, done = _Reader(raw), 0
            try:
                for i in left:
                    at = r.at
                    results[i] = _read_result(r, cases[i]["op"])
                    done += 1
            except EOFError:
                r.at = at
            if rc == 0 and done == len(left):
                break
            assert done < len(left), ("the driver failed after its last case", rc)
            bad = left[done]
            results[bad] = {"aborted": True} if rc == -signal.SIGABRT else {"failed": "exit status %s" % (rc,)}
            left = left[done + 1:]
    return results


# ------------------------------------------------------------------------------------------------------------------ the oracle's side
def oracle_result(c):
    """The same case on the oracle; "links" is oracle.links_off_the_array() for it (non-zero: the reference leaves its arrays),
    "inner_point_undefined" oracle.inner_point_undefined() (non-zero: its limited hull used an inner point that it never set)."""
    op = c["op"]
    O.links_off_the_array(reset=True)
    O.inner_point_undefined(reset=True)
    if op == "clip":
        out = dict(O.clip(c["solid"], c["planes"]))
    elif op == "faces":
        fo, fi = O.extract_faces(c["solid"])
        out = {"fo": fo, "fi": fi}
    elif op == "render":
        vnc, idx = O.render(c["solid"], convex=c["convex"], colour=c["colour"])
        out = {"vnc": vnc, "idx": idx}
    elif op == "neighbours":
        try:
            s = O.neighbours_from_mesh(c["pos"], c["tris"])
            out = {"off": s["off"], "nbr": s["nbr"]}
        except ValueError:
            out = {"threw": True}
    elif op == "moments":
        vol, cen = O.moments(c["solid"])
        out = {"vol": np.asarray([vol]), "centre": np.asarray(cen, np.float64)}
    elif op == "transform":
        out = {"pos": O.transform(c["solid"], c["world"])["pos"]}
    elif op == "kdop":
        out = {"planes": O.kdop_planes(c["points"], c["normals"], ach=c["ach"], max_axis_scale=c["max_axis_scale"], gap_inv=c["gap_inv"])}
    elif op == "refit":
        out = dict(O.refit(c["convex"], c["mesh"], c["limit"]))
    elif op == "hull":
        out = {"normals": O.hull_normals(c["points"], c["limit"])}
    else:
        raise KeyError(op)
    out["links"] = O.links_off_the_array(reset=True)
    out["inner_point_undefined"] = O.inner_point_undefined(reset=True)
    return out


# ------------------------------------------------------------------------------------------------------------------ the comparison
class Differs(AssertionError):
    pass


def relative_difference(got, ref):
    """Largest |got - ref| over the array, relative to the larger of each reference value's size and one hundredth of the array's
    largest (helpers.assert_event_equal's rtol / atol pair as one figure); 0.0 when the arrays are equal as numbers."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    if got.size == 0:
        return 0.0
    same = (got == ref) | (np.isnan(got) & np.isnan(ref))
    if same.all():
        return 0.0
    if not np.isfinite(ref[~same]).all() or not np.isfinite(got[~same]).all():
        return float("inf")
    scale = max(1.0, float(np.abs(ref[np.isfinite(ref)]).max()))
    return float((np.abs(got - ref)[~same] / np.maximum(np.abs(ref[~same]), 1e-2 * scale)).max())


def compare(op, got, ref, name="", exact=True, rtol=0.0):
    """`got` (the oracle's, the engine's, a mutation) against `ref` (the compiled reference's).  Topology: array_equal, no
    exceptions.  Coordinates: equal as numbers where exact, else within rtol.  Returns the largest relative difference."""
    if ref.get("threw") or got.get("threw"):
        if not (ref.get("threw") and got.get("threw")):
            raise Differs("%s: one side threw" % name)
        return 0.0
    for k in TOPOLOGY[op]:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if a.shape != b.shape or not np.array_equal(a, b):
            raise Differs("%s: %s differs (%s against %s)" % (name, k, a.shape, b.shape))
    worst = 0.0
    for k in COORDS[op]:
        a, b = np.asarray(got[k]), np.asarray(ref[k])
        if a.shape != b.shape:
            raise Differs("%s: %s has shape %s against %s" % (name, k, a.shape, b.shape))
        d = relative_difference(a, b)
        if (exact and d != 0.0) or (not exact and d > rtol):
            raise Differs("%s: %s differs by %.3g relative" % (name, k, d))
        worst = max(worst, d)
    return worst


# ------------------------------------------------------------------------------------------------------------------ the fixture
# tests/golden/reference_compiled.npz: cases and the compiled reference's results for them, so that the pin holds where the
# reference is absent.  Three blobs (float32, int32, float64) and an index in JSON; arrays with the same bytes are stored once.
_KIND = {"float32": "f", "int32": "i", "uint32": "u", "float64": "d"}
_DTYPE = {v: k for k, v in _KIND.items()}
_BLOB = {"f": "f32", "i": "i32", "u": "i32", "d": "f64"}


def record(path, cases, results):
    import json
    blobs, seen, index = {"f32": [], "i32": [], "f64": []}, {}, []
    fill = {"f32": 0, "i32": 0, "f64": 0}

    def put(v):
        if isinstance(v, (bool, int, float, str)):
            return v
        a = np.ascontiguousarray(v)
        if a.dtype not in (np.float32, np.int32, np.uint32, np.float64):
            raise TypeError(a.dtype)
        kind = _KIND[a.dtype.name]
        key = (kind, a.tobytes())
        if key not in seen:
            b = _BLOB[kind]
            seen[key] = fill[b]
            blobs[b].append(a.reshape(-1).view(np.int32) if kind == "u" else a.reshape(-1))
            fill[b] += a.size
        return [kind, seen[key], list(a.shape)]

    for c, r in zip(cases, results):
        assert "aborted" not in r and "failed" not in r, c["name"]
        index.append({"name": c["name"], "op": c["op"],
                      "in": {k: ({kk: put(vv) for kk, vv in v.items()} if isinstance(v, dict) else put(v))
                             for k, v in c.items() if k not in ("name", "op")},
                      "out": {k: put(v) for k, v in r.items()}})
    cat = {b: (np.concatenate(v) if v else np.zeros(0, {"f32": np.float32, "i32": np.int32, "f64": np.float64}[b])) for b, v in blobs.items()}
    np.savez_compressed(path, index=np.frombuffer(json.dumps(index, separators=(",", ":")).encode(), np.uint8), **cat)


def load(path):
    """-> (cases, results) as record() was given them."""
    import json
    z = np.load(path)
    blobs = {b: z[b] for b in ("f32", "i32", "f64")}

    def get(v):
        if isinstance(v, dict):
            return {k: get(w) for k, w in v.items()}
        if not isinstance(v, list):
            return v
        kind, start, shape = v
        n = int(np.prod(shape)) if shape else 1
        a = blobs[_BLOB[kind]][start:start + n]
        return (a.view(np.uint32) if kind == "u" else a).reshape(shape).copy()

    cases, results = [], []
    for e in json.loads(z["index"].tobytes().decode()):
        cases.append(dict({"name": e["name"], "op": e["op"]}, **{k: get(v) for k, v in e["in"].items()}))
        results.append({k: get(v) for k, v in e["out"].items()})
    return cases, results
