"""ctypes binding of libsurtr_hip.so (include/surtr_hip.h) for tests and bench.

This is plumbing only: numpy arrays in, numpy arrays out, every call goes
through the C ABI.  There is no CPU fallback -- if the shared library or a HIP
device is missing the calls raise.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

OK, E_INVALID, E_TOPOLOGY, E_CAPACITY, E_HIP, E_STATE, E_NOGPU = range(7)
EVT_REFIT, EVT_RENDER = 1, 2
CELLS_ALL = 0xFFFFFFFF      # SURTR_CELLS_ALL: every cell of every instance of place_cells_patterns


class SurtrError(RuntimeError):
    def __init__(self, code, msg=""):
        self.code = code
        RuntimeError.__init__(self, "surtr error %d: %s %s" % (code, _strerror(code), msg))


class Counts(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint32) for n in
                ("n_frag", "mesh_verts", "mesh_nbrs", "conv_verts", "conv_nbrs", "n_idx", "n_pairs", "status", "n_failed")]


class Mass(ctypes.Structure):
    """surtr_mass (include/surtr_hip.h), 96 bytes."""
    _fields_ = [("volume", ctypes.c_double), ("mass", ctypes.c_double), ("com", ctypes.c_double * 3),
                ("inertia", ctypes.c_double * 6), ("nv", ctypes.c_uint32), ("status", ctypes.c_uint32)]


# the same record as a numpy structured array: inertia = Ixx Iyy Izz Ixy Iyz Izx (tensor entries, about com)
MASS_DTYPE = np.dtype([("volume", "<f8"), ("mass", "<f8"), ("com", "<f8", (3,)), ("inertia", "<f8", (6,)),
                       ("nv", "<u4"), ("status", "<u4")])
assert MASS_DTYPE.itemsize == ctypes.sizeof(Mass) == 96

# surtr_hull / surtr_hull_polygon (include/surtr_hip.h): one record per solid, one polygon per face (PxHullPolygon's layout)
HULL_DTYPE = np.dtype([("nv", "<u4"), ("n_faces", "<u4"), ("n_idx", "<u4"), ("status", "<u4"), ("face_off", "<u4"), ("idx_off", "<u4"),
                       ("max_loop", "<u4"), ("reserved0", "<u4"), ("convexity", "<f4"), ("planarity", "<f4"), ("extent", "<f4"),
                       ("reserved1", "<u4")])
POLY_DTYPE = np.dtype([("plane", "<f4", (4,)), ("n_verts", "<u2"), ("index_base", "<u2")])
assert HULL_DTYPE.itemsize == 48 and POLY_DTYPE.itemsize == 20
HULL_FEW, HULL_OPEN, HULL_FLAT, HULL_IRREGULAR, HULL_LARGE, HULL_OVER_255 = 1, 2, 4, 8, 16, 32
HULL_WITHHELD = HULL_FEW | HULL_OPEN | HULL_IRREGULAR | HULL_LARGE


def hull_usable(record, rel_tol=1e-5):
    """surtr::HullUsable: no withholding bit, no flat face, and both errors within rel_tol of the solid's extent; a hull that fails
    falls back to ConvexPoints (a quickhull of the points)."""
    if int(record["status"]) & (HULL_WITHHELD | HULL_FLAT):
        return False
    tol = np.float32(rel_tol) * np.float32(record["extent"])
    return bool(record["convexity"] <= tol and record["planarity"] <= tol)


# surtr_shaded (include/surtr_hip.h), 16 bytes: one record per fragment of event_shaded
SHADED_DTYPE = np.dtype([("first_vertex", "<u4"), ("n_vertices", "<u4"), ("n_faces", "<u4"), ("status", "<u4")])
assert SHADED_DTYPE.itemsize == 16
SHADE_PER_TRIANGLE = 1
SHADE_NO_FACE = 0xFFFFFFFF


# surtr_cooked (include/surtr_hip.h), 64 bytes: one record per solid of event_cook / pieces_cook / cook_points
COOK_DTYPE = np.dtype([("nv_in", "<u4"), ("nv", "<u4"), ("n_faces", "<u4"), ("n_idx", "<u4"), ("status", "<u4"), ("pt_off", "<u4"),
                       ("face_off", "<u4"), ("idx_off", "<u4"), ("max_loop", "<u4"), ("n_welded", "<u4"), ("convexity", "<f4"),
                       ("planarity", "<f4"), ("extent", "<f4"), ("reach", "<f4"), ("reserved", "<u4", (2,))])
assert COOK_DTYPE.itemsize == 64
COOK_SKIPPED, COOK_FEW, COOK_DEGENERATE, COOK_NONFINITE, COOK_LARGE, COOK_FAILED, COOK_OVER_255 = 1, 2, 4, 8, 16, 32, 64
COOK_WITHHELD = COOK_SKIPPED | COOK_FEW | COOK_DEGENERATE | COOK_NONFINITE | COOK_LARGE | COOK_FAILED


def cooked_usable(record, plane_tol=7e-6, weld_dist=0.0):
    """surtr::CookedUsable: no withholding bit, planarity <= plane_tol + s and convexity <= 2 plane_tol + weld_dist + s, where
    s = 2^-24 * 3.5 * reach bounds the rounding of a written plane: |n_x| + |n_y| + |n_z| <= sqrt(3) and |d| <= sqrt(3) reach for a
    unit normal and a plane that passes among points of coordinates within reach."""
    if int(record["status"]) & COOK_WITHHELD:
        return False
    s = 2.0 ** -24 * 3.5 * float(record["reach"])
    return bool(record["planarity"] <= plane_tol + s and record["convexity"] <= 2.0 * plane_tol + weld_dist + s)


def cook_max_vertices():
    """surtr_cook_max_vertices: the most kept points the cooker takes per solid."""
    f = lib().surtr_cook_max_vertices
    f.restype = ctypes.c_uint32
    return int(f())


# surtr_ray_hit (include/surtr_hip.h), 48 bytes; status bits and the per-piece status bits of a query
RAY_HIT_DTYPE = np.dtype([("piece", "<i4"), ("status", "<u4"), ("t", "<f4"), ("pos", "<f4", (3,)), ("normal", "<f4", (3,)),
                          ("reserved", "<u4", (3,))])
assert RAY_HIT_DTYPE.itemsize == 48
# surtr_scene_ray_hit: the same record with the body of the piece hit
SCENE_RAY_HIT_DTYPE = np.dtype([("piece", "<i4"), ("status", "<u4"), ("t", "<f4"), ("pos", "<f4", (3,)), ("normal", "<f4", (3,)),
                                ("compound", "<i4"), ("reserved", "<u4", (2,))])
assert SCENE_RAY_HIT_DTYPE.itemsize == 48
RAY_STARTS_INSIDE, RAY_INVALID = 1, 2
QUERY_FEW, QUERY_OPEN, QUERY_FLAT, QUERY_LONG = 1, 2, 4, 8
# surtr_bounds (include/surtr_hip.h), 32 bytes: the world-space box of a body or a piece; the reason bits of scene_cull
BOUNDS_DTYPE = np.dtype([("lo", "<f4", (3,)), ("hi", "<f4", (3,)), ("n_vertices", "<u4"), ("status", "<u4")])
assert BOUNDS_DTYPE.itemsize == 32
BOUNDS_NONFINITE = 1
CULL_LIGHT, CULL_OUTSIDE = 1, 2
# surtr_contact and surtr_contact_header (include/surtr_hip.h), 64 bytes each: a reported pair of pieces of two bodies; the totals of a run
CONTACT_DTYPE = np.dtype([("body_a", "<u4"), ("body_b", "<u4"), ("piece_a", "<u4"), ("piece_b", "<u4"), ("distance", "<f4"), ("status", "<u4"),
                          ("point_a", "<f4", (3,)), ("point_b", "<f4", (3,)), ("normal", "<f4", (3,)), ("reserved", "<u4")])
CONTACT_HEADER_DTYPE = np.dtype([("status", "<u4"), ("n_records", "<u4"), ("n_body_pairs", "<u4"), ("n_piece_pairs", "<u4"), ("n_bodies", "<u4"),
                                 ("n_pieces", "<u4"), ("lists", "<u4"), ("reserved", "<u4", (9,))])
assert CONTACT_DTYPE.itemsize == 64 and CONTACT_HEADER_DTYPE.itemsize == 64
CONTACT_OVERLAP, CONTACT_ITER = 1, 2


# the arrays of surtr_pieces_derived, in the order of the SURTR_DERIVED_* enumeration (include/surtr_hip.h)
_DERIVED = (("llen", np.uint32), ("tri", np.uint8), ("rad", np.float32), ("box", np.float32), ("perm", np.uint32),
            ("posr_s", np.float32), ("bsph", np.float32), ("bsph2", np.float32), ("bsph3", np.float32), ("iperm", np.uint32),
            ("row_s", np.uint16), ("dup", np.uint8), ("bo", np.uint32), ("bo2", np.uint32), ("bo3", np.uint32), ("build", np.uint32))


class Fragments(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in
                ("frag_ids", "mesh_vert_off", "mesh_pos", "mesh_nbr_off", "mesh_nbr", "conv_vert_off", "conv_pos",
                 "conv_nbr_off", "conv_nbr", "vnc", "idx_off", "idx", "frag_status")]


def lib_path():
    return os.path.join(_HERE, "libsurtr_hip.so")


def _configure(L):
    L.surtr_strerror.restype = ctypes.c_char_p
    L.surtr_last_error.restype = ctypes.c_char_p
    L.surtr_last_error.argtypes = [ctypes.c_void_p]
    L.surtr_event_blob_bytes.restype = ctypes.c_size_t
    L.surtr_destroy.argtypes = [ctypes.c_void_p]
    L.surtr_destroy.restype = None
    return L


def _use_library_for_tests(path):
    """tests/ only: bind the single-lane CPU emulation of the kernels (tests/emul/libsurtr_emul.so)
    so kernel logic can be checked without a GPU.  Never called by product code."""
    global _LIB
    _LIB = _configure(ctypes.CDLL(path)) if path else None


def _share_hip_runtime_with_torch():
    """PyTorch wheels bundle their own libamdhip64 / libhsa-runtime64.  If libsurtr_hip.so is loaded first it brings in
    /opt/rocm's runtime, a later `import torch` brings in the bundled one, and the second ROCr runtime of a process cannot open
    the GPU ("No HIP GPUs are available").  A process that may use both (tests, bench.py, multigpu.py hand torch buffers to the
    engine) therefore loads the runtime torch would load, first: libsurtr_hip.so's libamdhip64.so.N then resolves to it by
    soname, which is what happens anyway when torch is imported before the engine.  Without torch installed this does nothing."""
    import sys, importlib.util
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            ctypes.CDLL(cand, mode=ctypes.RTLD_GLOBAL)
        except OSError:
            pass


def lib():
    global _LIB
    if _LIB is None:
        if not os.path.exists(lib_path()):
            raise ImportError("libsurtr_hip.so is not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        _share_hip_runtime_with_torch()
        L = _configure(ctypes.CDLL(lib_path()))
        _LIB = L
    return _LIB


def _strerror(code):
    try:
        return lib().surtr_strerror(ctypes.c_int(code)).decode()
    except Exception:
        return "?"


def _p(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _solid_arrays(s):
    return (np.ascontiguousarray(s["pos"], np.float32).reshape(-1, 3), np.ascontiguousarray(s["off"], np.uint32),
            np.ascontiguousarray(s["nbr"], np.int32))


def pack_solids(solids):
    """list of {'pos','off','nbr'} -> (vert_off, pos, nbr_off (global), nbr)"""
    vo = [0]
    pos, off, nbr = [], [np.zeros(1, np.int64)], []
    base = 0
    for s in solids:
        p = np.ascontiguousarray(s["pos"], np.float32).reshape(-1, 3)
        o = np.asarray(s["off"], np.int64)
        pos.append(p)
        off.append(o[1:] + base)
        base += int(o[-1])
        nbr.append(np.asarray(s["nbr"], np.int32))
        vo.append(vo[-1] + p.shape[0])
    return (np.asarray(vo, np.uint32), np.ascontiguousarray(np.concatenate(pos), np.float32),
            np.concatenate(off).astype(np.uint32), np.ascontiguousarray(np.concatenate(nbr), np.int32))


def _impact_targets(targets):
    """One list of compounds per impact -> (target_off uint32[K + 1], compounds uint32[n])."""
    lists = [np.ascontiguousarray(t, np.uint32).reshape(-1) for t in targets]
    to = np.zeros(len(lists) + 1, np.uint32)
    to[1:] = np.cumsum([x.shape[0] for x in lists])
    return to, (np.concatenate(lists) if lists else np.zeros(0, np.uint32)).astype(np.uint32)


def _impact_spheres(sphere_points, origins, radii, k=None):
    """One cloud, origin and radius per impact -> (K, sphere_off uint32[K + 1], points f32[n,3], origins f32[K,3], radii f32[K])."""
    if origins is not None:
        k = np.ascontiguousarray(origins, np.float32).reshape(-1, 3).shape[0]
    k = int(k or 0)
    org = np.zeros((k, 3), np.float32) if origins is None else np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
    rad = np.zeros(k, np.float32) if radii is None else np.ascontiguousarray(radii, np.float32).reshape(-1)
    clouds = [np.zeros((0, 3), np.float32)] * k if sphere_points is None else \
        [np.zeros((0, 3), np.float32) if c is None else np.ascontiguousarray(c, np.float32).reshape(-1, 3) for c in sphere_points]
    if not len(clouds) == org.shape[0] == rad.shape[0] == k:
        raise SurtrError(E_INVALID, "one cloud, origin and radius per impact")
    so = np.zeros(k + 1, np.uint32)
    so[1:] = np.cumsum([c.shape[0] for c in clouds])
    sp = np.ascontiguousarray(np.concatenate(clouds) if clouds else np.zeros((0, 3), np.float32), np.float32)
    if sp.shape[0] == 0:
        sp = np.zeros((1, 3), np.float32)      # (a pointer the library may check, never read)
    return k, so, sp, org, rad


class Engine:
    """One context per GPU (surtr_create / surtr_destroy)."""

    def __init__(self, device=0, stream=None):
        self._h = ctypes.c_void_p()
        rc = lib().surtr_create(ctypes.c_int(device), ctypes.byref(self._h))
        if rc:
            raise SurtrError(rc)
        if stream is not None:
            self.set_stream(stream)

    def close(self):
        if self._h:
            lib().surtr_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        if rc:
            raise SurtrError(rc, lib().surtr_last_error(self._h).decode())

    def set_stream(self, stream_ptr):
        self._ck(lib().surtr_set_stream(self._h, ctypes.c_void_p(stream_ptr)))

    def set_scratch(self, max_verts, max_nbrs):
        self._ck(lib().surtr_set_scratch(self._h, ctypes.c_uint32(max_verts), ctypes.c_uint32(max_nbrs)))

    def set_arena(self, verts, nbrs, idx):
        self._ck(lib().surtr_set_arena(self._h, ctypes.c_uint64(verts), ctypes.c_uint64(nbrs), ctypes.c_uint64(idx)))

    def set_profiling(self, on=True):
        self._ck(lib().surtr_set_profiling(self._h, ctypes.c_int(int(on))))

    def kernel_times(self):
        ms = (ctypes.c_float * 16)()
        self._ck(lib().surtr_kernel_times(self._h, ms))
        names = ("clip_pairs", "frag_table", "refit", "faces", "out_scan", "pack", "clip_convex", "prep_pairs", "clip_pairs_big", "clip_pairs_half", "clip_pairs_retry", "clip_pairs_wave", None, "clip_pairs_catch")
        return {n: float(ms[i]) for i, n in enumerate(names) if n}      # (slot 12 is unused)

    def set_events_in_flight(self, n):
        """Tells the context how many contexts the host keeps busy on this GPU (include/surtr_hip.h: surtr_set_events_in_flight)."""
        self._ck(lib().surtr_set_events_in_flight(self._h, ctypes.c_uint32(int(n))))

    PLAN_FIELDS = ("n_pairs", "events_in_flight", "bits", "prep_kind", "n_wg", "n_wg_cvx", "n_wg_lean", "n_wg_cvx2", "n_wg_prep", "n_wg_big",
                   "n_wg_half", "n_wg_retry", "n_catch", "n_wg_sweep", "n_poll", "g_refit", "g_faces", "g_faces2", "t_faces", "frag_tasks",
                   "prep_threads")
    PLAN_BITS = {"wave": 1, "split": 2, "half": 4, "front_par": 8, "both": 16, "cvx_lean": 32, "many_grids": 64, "cell_order": 128}

    def event_plan(self, n_pairs, flags=3, pair_list=False):
        """The plan an event of n_pairs pairs gets from this context now (include/surtr_hip.h: surtr_event_plan): a dict of
        PLAN_FIELDS, the bits of PLAN_BITS spelled out as booleans."""
        out = (ctypes.c_uint32 * 32)()
        self._ck(lib().surtr_event_plan(self._h, ctypes.c_uint32(int(n_pairs)), ctypes.c_int(int(bool(pair_list))), ctypes.c_uint32(int(flags)), out))
        plan = {n: int(out[i]) for i, n in enumerate(self.PLAN_FIELDS)}
        for n, b in self.PLAN_BITS.items():
            plan[n] = bool(plan["bits"] & b)
        return plan

    def kernel_history(self):
        """Durations (ms) of the Mesh clip kernel over the last events, oldest first (surtr_kernel_history)."""
        ms = (ctypes.c_float * 16)(); slot = (ctypes.c_int * 16)(); n = ctypes.c_uint32(0)
        self._ck(lib().surtr_kernel_history(self._h, ms, slot, ctypes.byref(n)))
        return [float(ms[i]) for i in range(n.value)]

    def pair_status(self, n_pairs):
        """Status per pair of the last event (include/surtr_hip.h: surtr_pair_status)."""
        out = np.zeros(n_pairs, dtype=np.uint32)
        self._ck(lib().surtr_pair_status(self._h, ctypes.c_uint32(n_pairs), _p(out)))
        return out

    def pair_costs(self, n_pairs):
        """Cost estimate per pair of the last event (include/surtr_hip.h: surtr_event_pair_costs)."""
        out = np.zeros(n_pairs, dtype=np.uint32)
        self._ck(lib().surtr_event_pair_costs(self._h, ctypes.c_uint32(n_pairs), _p(out)))
        return out

    def queue_stats(self):
        """Device-side counters of the last event (include/surtr_hip.h: surtr_queue_stats)."""
        out = (ctypes.c_uint32 * 128)()
        self._ck(lib().surtr_queue_stats(self._h, out))
        return np.frombuffer(out, dtype=np.uint32).copy()

    def handover_stats(self):
        """Hand-over words of the last event's split Mesh clip (include/surtr_hip.h: surtr_handover_stats): pushed, main workgroups
        started, signed off, poll slots claimed, the catcher's own-class cursor, the sweep's cursor, clip workgroups, list capacity."""
        out = (ctypes.c_uint32 * 8)()
        self._ck(lib().surtr_handover_stats(self._h, out))
        # (the first six in the order of the hand-over block CUR_HO_PUSHED .. CUR_Q_SWEEP of the slot enumeration in csrc/surtr_ctx.h)
        names = ("pushed", "main_started", "main_signed_off", "poll_claimed", "catch_own", "sweep_cursor", "max_wg", "hcap")
        return {n: int(out[i]) for i, n in enumerate(names)}

    def pair_order(self):
        """The order k_clip_convex took the last event's pairs in (include/surtr_hip.h: surtr_pair_order)."""
        n = ctypes.c_uint32()
        self._ck(lib().surtr_pair_order(self._h, ctypes.c_uint32(0), ctypes.byref(n), None))
        out = np.zeros(n.value, np.uint32)
        self._ck(lib().surtr_pair_order(self._h, ctypes.c_uint32(n.value), ctypes.byref(n), _p(out)))
        return out

    def upload_pieces(self, meshes, convexes):
        assert len(meshes) == len(convexes)
        m = pack_solids(meshes)
        c = pack_solids(convexes)
        self._ck(lib().surtr_upload_pieces(self._h, ctypes.c_uint32(len(meshes)), _p(m[0]), _p(m[1]), _p(m[2]), _p(m[3]),
                                           _p(c[0]), _p(c[1]), _p(c[2]), _p(c[3])))

    def build_cells(self, seeds, group_seed_off=None):
        """surtr_build_cells: Voronoi cells of the seeds on the device, installed as the pattern.  Returns (n_faces, n_face_verts)."""
        s = np.ascontiguousarray(seeds, np.float64).reshape(-1, 3)
        go = np.array([0, s.shape[0]], np.uint32) if group_seed_off is None else np.ascontiguousarray(group_seed_off, np.uint32)
        nf, nfv = ctypes.c_uint32(), ctypes.c_uint32()
        self._ck(lib().surtr_build_cells(self._h, ctypes.c_uint32(go.shape[0] - 1), _p(go), _p(s), ctypes.byref(nf), ctypes.byref(nfv)))
        self._cells_n = (s.shape[0], nf.value, nfv.value)
        return nf.value, nfv.value

    def download_cells(self):
        """The cells of the last build_cells in the layout of engine.voronoi_cells (+ 'v012')."""
        n, nf, nfv = self._cells_n
        cfo = np.zeros(n + 1, np.uint32); gen = np.zeros(nf, np.int32); fvo = np.zeros(nf + 1, np.uint32)
        verts = np.zeros((nfv, 3), np.float64); v012 = np.zeros((nf, 9), np.float32)
        self._ck(lib().surtr_download_cells(self._h, _p(cfo), _p(gen), _p(fvo), _p(verts), _p(v012)))
        return {"cell_face_off": cfo, "face_gen": gen, "face_vert_off": fvo, "verts": verts, "v012": v012}

    def neighbors_from_mesh(self, pos, tris):
        """Poly::ExtractNeighborFromMesh on the device (surtr_neighbors_from_mesh_dev) -> (solid, kernel milliseconds)."""
        pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
        tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
        off = np.zeros(pos.shape[0] + 1, np.uint32)
        nbr = np.zeros(3 * tris.shape[0] + 4, np.int32)
        ms = ctypes.c_float()
        self._ck(lib().surtr_neighbors_from_mesh_dev(self._h, ctypes.c_uint32(pos.shape[0]), ctypes.c_uint32(tris.shape[0]), _p(tris), _p(off), _p(nbr),
                                                     ctypes.byref(ms)))
        return {"pos": pos, "off": off, "nbr": nbr[:off[-1]].copy()}, float(ms.value)

    def upload_pattern(self, face_off, v012):
        fo = np.ascontiguousarray(face_off, np.uint32)
        v = np.ascontiguousarray(v012, np.float32).reshape(-1, 9)
        assert v.shape[0] == fo[-1]
        self._ck(lib().surtr_upload_pattern(self._h, ctypes.c_uint32(fo.shape[0] - 1), _p(fo), _p(v)))

    def place_cells(self, scale, translate):
        s = np.ascontiguousarray(scale, np.float32)
        t = np.ascontiguousarray(translate, np.float32)
        self._ck(lib().surtr_place_cells(self._h, _p(s), _p(t)))

    def place_cells_impacts(self, scales, translates):
        """surtr_place_cells_impacts: one instance of the pattern per impact, in one launch; instance i's cell c is cell
        i * n_cells + c.  scales / translates: f32[K,3]."""
        s = np.ascontiguousarray(scales, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(translates, np.float32).reshape(-1, 3)
        if s.shape[0] != t.shape[0]:
            raise SurtrError(E_INVALID, "%d scales, %d translates" % (s.shape[0], t.shape[0]))
        self._ck(lib().surtr_place_cells_impacts(self._h, ctypes.c_uint32(s.shape[0]), _p(s), _p(t)))

    # ---- the pattern library (include/surtr_hip.h): several patterns resident on the device
    def pattern_store(self):
        """surtr_pattern_store: the installed pattern into the library, device to device -> its id (0, 1, ... in order of storing)."""
        i = ctypes.c_uint32()
        self._ck(lib().surtr_pattern_store(self._h, ctypes.byref(i)))
        return i.value

    def pattern_count(self):
        n = ctypes.c_uint32()
        self._ck(lib().surtr_pattern_count(self._h, ctypes.byref(n)))
        return n.value

    def pattern_info(self, id):
        """surtr_pattern_info -> (n_cells, n_faces) of stored pattern id."""
        nc, nf = ctypes.c_uint32(), ctypes.c_uint32()
        self._ck(lib().surtr_pattern_info(self._h, ctypes.c_uint32(int(id)), ctypes.byref(nc), ctypes.byref(nf)))
        return nc.value, nf.value

    def pattern_select(self, id):
        """surtr_pattern_select: stored pattern id becomes the installed pattern, as upload_pattern of the same arrays leaves it."""
        self._ck(lib().surtr_pattern_select(self._h, ctypes.c_uint32(int(id))))

    def pattern_clear(self):
        self._ck(lib().surtr_pattern_clear(self._h))

    def place_cells_patterns(self, pattern_ids, scales, translates):
        """surtr_place_cells_patterns: one instance per impact, instance i being stored pattern pattern_ids[i] under scales[i] /
        translates[i]; its cells are [b[i], b[i + 1]) of placed_cells().  The event over them: scene_fracture_impacts(targets, 0,
        CELLS_ALL)."""
        ids = np.ascontiguousarray(pattern_ids, np.uint32).reshape(-1)
        s = np.ascontiguousarray(scales, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(translates, np.float32).reshape(-1, 3)
        if not ids.shape[0] == s.shape[0] == t.shape[0]:
            raise SurtrError(E_INVALID, "%d ids, %d scales, %d translates" % (ids.shape[0], s.shape[0], t.shape[0]))
        self._ck(lib().surtr_place_cells_patterns(self._h, ctypes.c_uint32(ids.shape[0]), _p(ids), _p(s), _p(t)))

    def placed_cells(self):
        """surtr_placed_cells: cell_base of the placed instances (uint32[K + 1]) after place_cells_impacts or place_cells_patterns."""
        n = ctypes.c_uint32()
        self._ck(lib().surtr_placed_cells(self._h, ctypes.c_uint32(0), ctypes.byref(n), None))
        out = np.zeros(n.value, np.uint32)
        self._ck(lib().surtr_placed_cells(self._h, ctypes.c_uint32(n.value), ctypes.byref(n), _p(out)))
        return out

    def event_regroup_impacts_partial(self, partial, sphere_points=None, origins=None, radii=None):
        """surtr_event_regroup_impacts_partial: event_regroup_impacts with a flag per impact (a sequence): the bodies of an impact
        whose flag is 0 are tested against no sphere (its cloud may be None or empty).  -> as event_regroup_impacts."""
        flags = np.ascontiguousarray([1 if f else 0 for f in partial], np.uint8)
        k, so, sp, org, rad = _impact_spheres(sphere_points, origins, radii, flags.shape[0])
        if k != flags.shape[0]:
            raise SurtrError(E_INVALID, "%d spheres for %d flags" % (k, flags.shape[0]))
        return self._regroup("surtr_event_regroup_impacts_partial", [self._h, _p(flags), ctypes.c_uint32(k), _p(so), _p(sp), _p(org), _p(rad)], True)

    def download_planes(self, impacts=False):
        """surtr_download_planes (diagnostic): the placed planes as f32[n,4]; impacts: those of place_cells_impacts, instance-major."""
        n = ctypes.c_uint32()
        self._ck(lib().surtr_download_planes(self._h, ctypes.c_int(int(impacts)), ctypes.c_uint32(0), ctypes.byref(n), None))
        out = np.zeros((max(n.value, 1), 4), np.float32)
        self._ck(lib().surtr_download_planes(self._h, ctypes.c_int(int(impacts)), ctypes.c_uint32(n.value), ctypes.byref(n), _p(out)))
        return out[:n.value].copy()

    def upload_planes(self, plane_off, planes):
        po = np.ascontiguousarray(plane_off, np.uint32)
        pl = np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
        self._ck(lib().surtr_upload_planes(self._h, ctypes.c_uint32(po.shape[0] - 1), _p(po), _p(pl)))

    def fracture_event(self, cell_begin, cell_end, outside=None, flags=EVT_REFIT | EVT_RENDER):
        c = Counts()
        om = None if outside is None else np.ascontiguousarray(outside, np.uint8)
        self._ck(lib().surtr_fracture_event(self._h, ctypes.c_uint32(cell_begin), ctypes.c_uint32(cell_end), _p(om),
                                            ctypes.c_uint32(flags), ctypes.byref(c)))
        return c

    def fracture_event_async(self, cell_begin, cell_end, outside=None, flags=EVT_REFIT | EVT_RENDER):
        om = None if outside is None else np.ascontiguousarray(outside, np.uint8)
        self._ck(lib().surtr_fracture_event_async(self._h, ctypes.c_uint32(cell_begin), ctypes.c_uint32(cell_end), _p(om),
                                                  ctypes.c_uint32(flags)))

    def place_cells_groups(self, group_cell_off, scales, translates):
        go = np.ascontiguousarray(group_cell_off, np.uint32)
        s = np.ascontiguousarray(scales, np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(translates, np.float32).reshape(-1, 3)
        assert s.shape[0] == go.shape[0] - 1 == t.shape[0]
        self._ck(lib().surtr_place_cells_groups(self._h, ctypes.c_uint32(s.shape[0]), _p(go), _p(s), _p(t)))

    def place_cells_in_pieces(self, group_cell_off):
        go = np.ascontiguousarray(group_cell_off, np.uint32)
        self._ck(lib().surtr_place_cells_in_pieces(self._h, ctypes.c_uint32(go.shape[0] - 1), _p(go)))

    def fracture_pairs(self, pair_cell, pair_piece, flags=EVT_REFIT | EVT_RENDER):
        pc = np.ascontiguousarray(pair_cell, np.uint32)
        pp = np.ascontiguousarray(pair_piece, np.uint32)
        assert pc.shape == pp.shape
        self._ck(lib().surtr_fracture_pairs_async(self._h, ctypes.c_uint32(pc.shape[0]), _p(pc), _p(pp), ctypes.c_uint32(flags)))
        return self.event_counts()

    def fracture_pairs_async(self, pair_cell, pair_piece, flags=EVT_REFIT | EVT_RENDER):
        """fracture_pairs without reading the counts back: nothing waits for the event (surtr_fracture_pairs_async)."""
        pc = np.ascontiguousarray(pair_cell, np.uint32)
        pp = np.ascontiguousarray(pair_piece, np.uint32)
        assert pc.shape == pp.shape
        self._ck(lib().surtr_fracture_pairs_async(self._h, ctypes.c_uint32(pc.shape[0]), _p(pc), _p(pp), ctypes.c_uint32(flags)))

    def _regroup(self, symbol, args, with_bodies):
        """The regroup calls: sizes first, then the fill through `symbol` -> (compound_off, compound_piece[, body_compound_off])."""
        n, nc, nb = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        sizes = lib().surtr_event_regroup_bodies if symbol == "surtr_event_regroup" else getattr(lib(), symbol)
        # (the sizes: after scene_fracture_bodies every body has a bind 0 of its own, so n_pieces + n_bodies + 1 offsets)
        self._ck(sizes(*args, ctypes.byref(n), ctypes.byref(nc), None, None, ctypes.byref(nb), None))
        co = np.zeros(n.value + nb.value + 1, np.uint32); cp = np.zeros(max(n.value, 1), np.int32); bo = np.zeros(nb.value + 1, np.uint32)
        tail = (ctypes.byref(nb), _p(bo)) if with_bodies else ()
        self._ck(getattr(lib(), symbol)(*args, ctypes.byref(n), ctypes.byref(nc), _p(co), _p(cp), *tail))
        out = (co[:nc.value + 1].copy(), cp[:co[nc.value]].copy())
        return out + (bo,) if with_bodies else out

    def _sphere_args(self, partial, sphere_points, origin, radius):
        sp = np.zeros((0, 3), np.float32) if sphere_points is None else np.ascontiguousarray(sphere_points, np.float32).reshape(-1, 3)
        org = np.ascontiguousarray(origin, np.float32)
        return [self._h, ctypes.c_int(int(partial)), ctypes.c_uint32(sp.shape[0]), _p(sp), _p(org), ctypes.c_float(radius)]

    def event_regroup(self, partial=False, sphere_points=None, origin=(0, 0, 0), radius=1.0):
        """surtr_event_regroup: bind sets + MergeOutOfImpact + HandleConvexIsland of the last event, on the device."""
        return self._regroup("surtr_event_regroup", self._sphere_args(partial, sphere_points, origin, radius), False)

    def event_regroup_bodies(self, partial=False, sphere_points=None, origin=(0, 0, 0), radius=1.0):
        """surtr_event_regroup_bodies: event_regroup with the compounds of every body of the event -> (compound_off, compound_piece,
        body_compound_off): body b (target b of scene_fracture_bodies) owns compounds [body_off[b], body_off[b + 1])."""
        return self._regroup("surtr_event_regroup_bodies", self._sphere_args(partial, sphere_points, origin, radius), True)

    def event_regroup_impacts(self, partial=False, sphere_points=None, origins=None, radii=None, n_impacts=None):
        """surtr_event_regroup_impacts: event_regroup_bodies after scene_fracture_impacts, every body against the sphere of its own
        impact.  sphere_points: one f32[n_i,3] cloud per impact; origins f32[K,3]; radii f32[K].  -> (compound_off, compound_piece,
        body_compound_off), a body being a target in the order given."""
        k, so, sp, org, rad = _impact_spheres(sphere_points, origins, radii, n_impacts)
        return self._regroup("surtr_event_regroup_impacts", [self._h, ctypes.c_int(int(partial)), ctypes.c_uint32(k), _p(so), _p(sp), _p(org), _p(rad)], True)

    def regroup_stats(self):
        """What the last event_regroup counted (include/surtr_hip.h: surtr_regroup_stats); no synchronisation."""
        out = (ctypes.c_uint32 * 8)()
        self._ck(lib().surtr_regroup_stats(self._h, out))
        names = ("pieces", "faces", "face_points", "edges", "cap_edges", "rounds", "out_of_sphere")
        return {n: int(out[i]) for i, n in enumerate(names)}

    def _mass(self, fn, set, density):
        n = ctypes.c_uint32()
        args = [self._h, ctypes.c_int(int(set)), ctypes.c_float(density)]
        self._ck(fn(*args, ctypes.byref(n), None))
        out = np.zeros(n.value, MASS_DTYPE)
        if n.value:
            self._ck(fn(*args, ctypes.byref(n), _p(out)))
        return out

    def event_mass(self, set=1, density=10.0):
        """surtr_event_mass: mass, centre of mass and inertia of every fragment of the last event (set 0 = Mesh, 1 = Convex)
        as a MASS_DTYPE array, computed on the device."""
        return self._mass(lib().surtr_event_mass, set, density)

    def pieces_mass(self, set=1, density=10.0):
        """surtr_pieces_mass: the same for the resident pieces."""
        return self._mass(lib().surtr_pieces_mass, set, density)

    def event_mass_dev(self, dev_ptr, capacity, set=1, density=10.0):
        """surtr_event_mass_dev: the records into a device buffer, on the context's stream, without a synchronisation."""
        self._ck(lib().surtr_event_mass_dev(self._h, ctypes.c_int(int(set)), ctypes.c_float(density), ctypes.c_void_p(dev_ptr),
                                            ctypes.c_size_t(capacity)))

    def pieces_mass_dev(self, dev_ptr, capacity, set=1, density=10.0):
        self._ck(lib().surtr_pieces_mass_dev(self._h, ctypes.c_int(int(set)), ctypes.c_float(density), ctypes.c_void_p(dev_ptr),
                                             ctypes.c_size_t(capacity)))

    def _hulls(self, fn):
        n, nf, ni = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._ck(fn(self._h, ctypes.byref(n), None, ctypes.byref(nf), None, ctypes.byref(ni), None))
        rec, poly, idx = np.zeros(n.value, HULL_DTYPE), np.zeros(nf.value, POLY_DTYPE), np.zeros(ni.value, np.uint16)
        # (zero-length arrays still pass as non-NULL: numpy gives them an address)
        self._ck(fn(self._h, ctypes.byref(n), _p(rec), ctypes.byref(nf), _p(poly), ctypes.byref(ni), _p(idx)))
        return {"records": rec, "polygons": poly, "idx": idx}

    def event_hulls(self):
        """surtr_event_hulls: face loops and planes of the Convex of every current fragment, computed on the device ->
        {records (HULL_DTYPE), polygons (POLY_DTYPE), idx (uint16, solid-local)}."""
        return self._hulls(lib().surtr_event_hulls)

    def pieces_hulls(self):
        """surtr_pieces_hulls: the same for the Convex solids of the resident pieces."""
        return self._hulls(lib().surtr_pieces_hulls)

    def event_hulls_dev(self, dev_records, records_bytes, dev_polys, polys_cap, dev_idx, idx_cap):
        """surtr_event_hulls_dev: header + records, polygons and indices into device buffers, on the context's stream, without a
        synchronisation (capacities in bytes, polygons, indices)."""
        self._ck(lib().surtr_event_hulls_dev(self._h, ctypes.c_void_p(dev_records), ctypes.c_size_t(records_bytes), ctypes.c_void_p(dev_polys),
                                             ctypes.c_size_t(polys_cap), ctypes.c_void_p(dev_idx), ctypes.c_size_t(idx_cap)))

    def pieces_hulls_dev(self, dev_records, records_bytes, dev_polys, polys_cap, dev_idx, idx_cap):
        self._ck(lib().surtr_pieces_hulls_dev(self._h, ctypes.c_void_p(dev_records), ctypes.c_size_t(records_bytes), ctypes.c_void_p(dev_polys),
                                              ctypes.c_size_t(polys_cap), ctypes.c_void_p(dev_idx), ctypes.c_size_t(idx_cap)))

    def event_shaded(self, color=None, tri_face=False):
        """surtr_event_shaded: the lit render buffers of the current (triangulated) fragments, computed on the device ->
        (records (SHADED_DTYPE), vnc f32[n, 9]: position, face normal, colour of every index of the packed idx, tri_face u32[n / 3] or
        None).  color: three floats (None: 0.25 grey)."""
        col = None if color is None else (ctypes.c_float * 3)(*[float(x) for x in color])
        fn = lib().surtr_event_shaded
        n, nv, nf = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        self._ck(fn(self._h, col, ctypes.byref(n), None, ctypes.byref(nv), None, None, ctypes.byref(nf)))
        rec, vnc = np.zeros(n.value, SHADED_DTYPE), np.zeros((nv.value, 9), np.float32)
        tri = np.zeros(nv.value // 3, np.uint32) if tri_face else None
        # (zero-length arrays still pass as non-NULL: numpy gives them an address)
        self._ck(fn(self._h, col, ctypes.byref(n), _p(rec), ctypes.byref(nv), _p(vnc), _p(tri), ctypes.byref(nf)))
        return rec, vnc, tri

    def event_shaded_dev(self, dev_records, records_bytes, dev_vnc, vnc_cap, dev_tri_face=0, tri_cap=0, color=None):
        """surtr_event_shaded_dev: header + records, vertices and (optionally) face numbers into device buffers, on the context's stream,
        without a synchronisation (capacities in bytes, vertices, triangles)."""
        col = None if color is None else (ctypes.c_float * 3)(*[float(x) for x in color])
        self._ck(lib().surtr_event_shaded_dev(self._h, col, ctypes.c_void_p(dev_records or None), ctypes.c_size_t(records_bytes),
                                              ctypes.c_void_p(dev_vnc or None), ctypes.c_size_t(vnc_cap), ctypes.c_void_p(dev_tri_face or None),
                                              ctypes.c_size_t(tri_cap)))

    def set_shade_tier(self, half_edges):
        """surtr_set_shade_tier (diagnostic): fragments above this many half-edges take event_shaded's global-scratch tier; 0: built-in."""
        self._ck(lib().surtr_set_shade_tier(self._h, ctypes.c_uint32(int(half_edges))))

    def _cook(self, call):
        c = [ctypes.c_uint32() for _ in range(4)]
        self._ck(call(ctypes.byref(c[0]), None, ctypes.byref(c[1]), None, None, ctypes.byref(c[2]), None, ctypes.byref(c[3]), None))
        rec, pts, src = np.zeros(c[0].value, COOK_DTYPE), np.zeros((c[1].value, 3), np.float32), np.zeros(c[1].value, np.uint32)
        poly, idx = np.zeros(c[2].value, POLY_DTYPE), np.zeros(c[3].value, np.uint16)
        self._ck(call(ctypes.byref(c[0]), _p(rec), ctypes.byref(c[1]), _p(pts), _p(src), ctypes.byref(c[2]), _p(poly), ctypes.byref(c[3]), _p(idx)))
        return {"records": rec, "points": pts, "src": src, "polygons": poly, "idx": idx}

    def _cook_sel(self, fn, hulls, rel_tol, weld_dist, plane_tol):
        h = None if hulls is None else np.ascontiguousarray(hulls, HULL_DTYPE)
        return self._cook(lambda *a: fn(self._h, None if h is None else _p(h), ctypes.c_uint32(0 if h is None else h.shape[0]),
                                        ctypes.c_float(rel_tol), ctypes.c_float(weld_dist), ctypes.c_float(plane_tol), *a))

    def event_cook(self, hulls=None, rel_tol=1e-5, weld_dist=0.0, plane_tol=7e-6):
        """surtr_event_cook: weld, convex hull and coplanar merge of the points of the Convex of every current fragment, on the
        device -> {records (COOK_DTYPE), points f32[n, 3], src (the input point of each), polygons (POLY_DTYPE), idx (uint16)}.
        hulls: the records of event_hulls; only the solids hull_usable refuses at rel_tol are cooked.  None: every solid."""
        return self._cook_sel(lib().surtr_event_cook, hulls, rel_tol, weld_dist, plane_tol)

    def pieces_cook(self, hulls=None, rel_tol=1e-5, weld_dist=0.0, plane_tol=7e-6):
        """surtr_pieces_cook: the same for the Convex solids of the resident pieces (hulls: the records of pieces_hulls)."""
        return self._cook_sel(lib().surtr_pieces_cook, hulls, rel_tol, weld_dist, plane_tol)

    def cook_points(self, solids, weld_dist=0.0, plane_tol=7e-6):
        """surtr_cook_points: the same kernels on point sets of the host (a list of f32[n, 3] arrays), every one cooked."""
        arrs = [np.ascontiguousarray(a, np.float32).reshape(-1, 3) for a in solids]
        vo = np.concatenate([[0], np.cumsum([a.shape[0] for a in arrs])]).astype(np.uint32)
        pos = np.ascontiguousarray(np.concatenate(arrs) if arrs else np.zeros((0, 3), np.float32), np.float32)
        return self._cook(lambda *a: lib().surtr_cook_points(self._h, ctypes.c_uint32(len(arrs)), _p(vo), _p(pos), ctypes.c_float(weld_dist),
                                                             ctypes.c_float(plane_tol), *a))

    def _cook_dev(self, fn, dev_hulls, rel_tol, weld_dist, plane_tol, dev_records, records_bytes, dev_points, points_cap, dev_src, dev_polys,
                  polys_cap, dev_idx, idx_cap):
        self._ck(fn(self._h, ctypes.c_void_p(dev_hulls or None), ctypes.c_float(rel_tol), ctypes.c_float(weld_dist), ctypes.c_float(plane_tol),
                    ctypes.c_void_p(dev_records), ctypes.c_size_t(records_bytes), ctypes.c_void_p(dev_points), ctypes.c_size_t(points_cap),
                    ctypes.c_void_p(dev_src), ctypes.c_void_p(dev_polys), ctypes.c_size_t(polys_cap), ctypes.c_void_p(dev_idx), ctypes.c_size_t(idx_cap)))

    def event_cook_dev(self, dev_hulls, rel_tol, weld_dist, plane_tol, dev_records, records_bytes, dev_points, points_cap, dev_src, dev_polys,
                       polys_cap, dev_idx, idx_cap):
        """surtr_event_cook_dev: header + records, points, src, polygons and indices into device buffers, on the context's stream,
        without a synchronisation.  dev_hulls: the buffer event_hulls_dev wrote (0 / None: every solid is cooked)."""
        self._cook_dev(lib().surtr_event_cook_dev, dev_hulls, rel_tol, weld_dist, plane_tol, dev_records, records_bytes, dev_points, points_cap,
                       dev_src, dev_polys, polys_cap, dev_idx, idx_cap)

    def pieces_cook_dev(self, dev_hulls, rel_tol, weld_dist, plane_tol, dev_records, records_bytes, dev_points, points_cap, dev_src, dev_polys,
                        polys_cap, dev_idx, idx_cap):
        self._cook_dev(lib().surtr_pieces_cook_dev, dev_hulls, rel_tol, weld_dist, plane_tol, dev_records, records_bytes, dev_points, points_cap,
                       dev_src, dev_polys, polys_cap, dev_idx, idx_cap)

    def pieces_raycast(self, rays):
        """surtr_pieces_raycast: rays f32[n, 7] (origin, direction, max_dist) against the Convex solids of the resident pieces,
        on the device -> RAY_HIT_DTYPE[n] (piece -1: no hit)."""
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 7)
        out = np.zeros(r.shape[0], RAY_HIT_DTYPE)
        self._ck(lib().surtr_pieces_raycast(self._h, ctypes.c_uint32(r.shape[0]), _p(r), _p(out)))
        return out

    def pieces_overlap(self, spheres, mass=None, min_mass=1e-4):
        """surtr_pieces_overlap: spheres f32[n, 4] (centre, radius) -> uint8[n, n_pieces]: 0 not touched, 1 touched, 2 touched
        but mass <= min_mass (mass: the MASS_DTYPE records of pieces_mass; None: no gate)."""
        sp = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        m = None if mass is None else np.ascontiguousarray(mass, MASS_DTYPE)
        n = ctypes.c_uint32()
        args = [self._h, ctypes.c_uint32(sp.shape[0]), _p(sp), _p(m), ctypes.c_float(min_mass)]
        self._ck(lib().surtr_pieces_overlap(*args, ctypes.byref(n), None))
        if m is not None and m.shape[0] != n.value:
            raise SurtrError(E_INVALID, "mass holds %d records for %d pieces" % (m.shape[0], n.value))
        out = np.zeros((sp.shape[0], n.value), np.uint8)
        self._ck(lib().surtr_pieces_overlap(*args, ctypes.byref(n), _p(out)))
        return out

    def pieces_raycast_dev(self, n_rays, dev_rays, dev_hits, capacity):
        """surtr_pieces_raycast_dev: device pointers, the context's stream, no synchronisation."""
        self._ck(lib().surtr_pieces_raycast_dev(self._h, ctypes.c_uint32(int(n_rays)), ctypes.c_void_p(dev_rays), ctypes.c_void_p(dev_hits),
                                                ctypes.c_size_t(capacity)))

    def pieces_overlap_dev(self, n_spheres, dev_spheres, dev_mask, capacity, dev_mass=None, min_mass=1e-4):
        self._ck(lib().surtr_pieces_overlap_dev(self._h, ctypes.c_uint32(int(n_spheres)), ctypes.c_void_p(dev_spheres),
                                                ctypes.c_void_p(dev_mass), ctypes.c_float(min_mass), ctypes.c_void_p(dev_mask),
                                                ctypes.c_size_t(capacity)))

    def pieces_query_status(self, n):
        """surtr_pieces_query_status: the QUERY_* bits of every piece as the last ray cast / overlap found them."""
        out = np.zeros(int(n), np.uint32)
        self._ck(lib().surtr_pieces_query_status(self._h, ctypes.c_uint32(int(n)), _p(out)))
        return out

    def download_piece(self, piece, set=1):
        """surtr_download_piece: resident piece `piece` read back (set 0 = Mesh, 1 = Convex) as a solid."""
        nv, nh = ctypes.c_uint32(), ctypes.c_uint32()
        args = [self._h, ctypes.c_uint32(int(piece)), ctypes.c_int(int(set))]
        self._ck(lib().surtr_download_piece(*args, ctypes.byref(nv), ctypes.byref(nh), None, None, None))
        pos = np.zeros((nv.value, 3), np.float32); off = np.zeros(nv.value + 1, np.uint32); nbr = np.zeros(nh.value, np.int32)
        self._ck(lib().surtr_download_piece(*args, ctypes.byref(nv), ctypes.byref(nh), _p(pos), _p(off), _p(nbr)))
        return {"pos": pos, "off": off, "nbr": nbr}

    def pieces_derived(self, set=0):
        """surtr_pieces_derived: what the pre-pass derives from the resident pieces of one set (0 = Mesh, 1 = Convex), read back
        as a dict of numpy arrays: llen, tri, rad, box [n, 6], perm, posr_s [V, 4], bsph / bsph2 / bsph3 [., 4], iperm,
        row_s [V, 8], dup, bo / bo2 / bo3, and the library's 'SB' and 'FAN' (vertices per level-1 sphere, spheres per coarser
        sphere).  A diagnostic for tests."""
        def get(which, dtype):
            b = ctypes.c_size_t()
            args = [self._h, ctypes.c_int(int(set)), ctypes.c_int(which)]
            self._ck(lib().surtr_pieces_derived(*args, None, ctypes.c_size_t(0), ctypes.byref(b)))
            buf = np.zeros(b.value, np.uint8)
            self._ck(lib().surtr_pieces_derived(*args, _p(buf), ctypes.c_size_t(b.value), ctypes.byref(b)))
            return buf.view(dtype)
        out = {name: get(which, dt) for which, (name, dt) in enumerate(_DERIVED)}
        for name, width in (("box", 6), ("posr_s", 4), ("bsph", 4), ("bsph2", 4), ("bsph3", 4), ("row_s", 8)):
            out[name] = out[name].reshape(-1, width)
        build = out.pop("build")
        out["SB"], out["FAN"] = int(build[0]), int(build[1])
        return out

    def event_refit(self):
        self._ck(lib().surtr_event_refit(self._h))

    def set_refit_point_limit(self, n):
        """FractureArgs::RefittingPointLimit, 4 (default) .. 32 (surtr_set_refit_point_limit): read by EVT_REFIT events,
        event_refit and refit_solid."""
        self._ck(lib().surtr_set_refit_point_limit(self._h, ctypes.c_uint32(int(n))))

    def get_refit_point_limit(self):
        n = ctypes.c_uint32()
        self._ck(lib().surtr_get_refit_point_limit(self._h, ctypes.byref(n)))
        return int(n.value)

    def hull_normals_device(self, points, limit):
        """For tests: face normals of the limited hull as the refit kernel builds it (surtr_hull_normals_device)."""
        p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
        cnt = ctypes.c_uint32()
        out = np.zeros((63, 3), np.float32)
        self._ck(lib().surtr_hull_normals_device(self._h, ctypes.c_uint32(p.shape[0]), _p(p), ctypes.c_uint32(int(limit)), ctypes.c_uint32(63),
                                                 _p(out), ctypes.byref(cnt)))
        return out[:cnt.value].copy()

    def event_counts(self):
        c = Counts()
        self._ck(lib().surtr_event_counts(self._h, ctypes.byref(c)))
        return c

    def pack_dev(self, dev_ptr, capacity):
        self._ck(lib().surtr_event_pack_dev(self._h, ctypes.c_void_p(dev_ptr), ctypes.c_size_t(capacity)))

    def download(self):
        c = self.event_counts()
        out = alloc_fragments(c)
        fr = _frag_struct(out)
        self._ck(lib().surtr_event_download(self._h, ctypes.byref(fr)))
        return shape_fragments(out)

    def load_fragments(self, meshes, convexes, frag_ids=None):
        """surtr_load_fragments: host pieces presented as the fragments of an event."""
        m = pack_solids(meshes)
        c = pack_solids(convexes)
        ids = None if frag_ids is None else np.ascontiguousarray(frag_ids, np.int32)
        self._ck(lib().surtr_load_fragments(self._h, ctypes.c_uint32(len(meshes)), _p(m[0]), _p(m[1]), _p(m[2]), _p(m[3]),
                                            _p(c[0]), _p(c[1]), _p(c[2]), _p(c[3]), _p(ids)))

    def event_triangulate(self, is_convex=False):
        self._ck(lib().surtr_event_triangulate(self._h, ctypes.c_int(int(is_convex))))

    def refit_solid(self, mesh, convex):
        """m_refittingTask for one Piece (surtr_refit_solid) -> the refitted Convex."""
        mp, mo, mn = _solid_arrays(mesh)
        cp, co, cn = _solid_arrays(convex)
        nv, nh = ctypes.c_uint32(), ctypes.c_uint32()
        args = [self._h, ctypes.c_uint32(mp.shape[0]), _p(mp), _p(mo), _p(mn), ctypes.c_uint32(cp.shape[0]), _p(cp), _p(co), _p(cn)]
        self._ck(lib().surtr_refit_solid(*args, ctypes.byref(nv), ctypes.byref(nh), None, None, None))
        opos = np.zeros((nv.value, 3), np.float32); ooff = np.zeros(nv.value + 1, np.uint32); onbr = np.zeros(nh.value, np.int32)
        self._ck(lib().surtr_refit_solid(*args, ctypes.byref(nv), ctypes.byref(nh), _p(opos), _p(ooff), _p(onbr)))
        return {"pos": opos, "off": ooff, "nbr": onbr}

    def extract_faces(self, solid):
        """Poly::ExtractFaces (surtr_extract_faces) -> (face_off, face_idx)."""
        p, o, n = _solid_arrays(solid)
        nf, ni = ctypes.c_uint32(), ctypes.c_uint32()
        args = [self._h, ctypes.c_uint32(p.shape[0]), _p(p), _p(o), _p(n)]
        self._ck(lib().surtr_extract_faces(*args, ctypes.byref(nf), ctypes.byref(ni), None, None))
        fo = np.zeros(nf.value + 1, np.uint32); fi = np.zeros(ni.value, np.int32)
        self._ck(lib().surtr_extract_faces(*args, ctypes.byref(nf), ctypes.byref(ni), _p(fo), _p(fi)))
        return fo, fi

    def triangulate(self, solid, is_convex=False, color=None):
        """Poly::ExtractFaces + Poly::RenderPolyhedron (surtr_triangulate) -> (vnc f32[n,9], idx u32[...])."""
        p, o, n = _solid_arrays(solid)
        col = None if color is None else np.ascontiguousarray(color, np.float32)
        ni = ctypes.c_uint32()
        args = [self._h, ctypes.c_uint32(p.shape[0]), _p(p), _p(o), _p(n), ctypes.c_int(int(is_convex)), _p(col)]
        self._ck(lib().surtr_triangulate(*args, None, ctypes.byref(ni), None))
        vnc = np.zeros((p.shape[0], 9), np.float32); idx = np.zeros(ni.value, np.uint32)
        self._ck(lib().surtr_triangulate(*args, _p(vnc), ctypes.byref(ni), _p(idx)))
        return vnc, idx

    def transform_pieces(self, world):
        """Poly::Transform of every resident piece (surtr_transform_pieces); world: f32[n,4,4] row-major XMMATRIX."""
        w = np.ascontiguousarray(world, np.float32).reshape(-1, 16)
        self._ck(lib().surtr_transform_pieces(self._h, ctypes.c_uint32(w.shape[0]), _p(w)))

    def pieces_from_event(self, keep=None):
        """surtr_pieces_from_event: the last event's fragments become the resident pieces; returns their number."""
        k = None if keep is None else np.ascontiguousarray(keep, np.uint8)
        n = ctypes.c_uint32()
        self._ck(lib().surtr_pieces_from_event(self._h, _p(k), ctypes.byref(n)))
        return n.value

    # ---- the scene: several bodies in the resident set (include/surtr_hip.h, scene_dev.hip)
    def scene_set_compounds(self, compound_off):
        """surtr_scene_set_compounds: compound c = resident pieces [compound_off[c], compound_off[c + 1])."""
        co = np.ascontiguousarray(compound_off, np.uint32)
        self._ck(lib().surtr_scene_set_compounds(self._h, ctypes.c_uint32(max(co.shape[0] - 1, 0)), _p(co)))

    def scene_compounds(self):
        """surtr_scene_get_compounds: the compound table as uint32[n_compounds + 1]."""
        n = ctypes.c_uint32()
        self._ck(lib().surtr_scene_get_compounds(self._h, ctypes.c_uint32(0), ctypes.byref(n), None))
        co = np.zeros(n.value + 1, np.uint32)
        self._ck(lib().surtr_scene_get_compounds(self._h, ctypes.c_uint32(co.shape[0]), ctypes.byref(n), _p(co)))
        return co

    def scene_transform_compound(self, compound, world):
        """surtr_scene_transform_compound: Poly::Transform of that compound's pieces only; world: f32[n,4,4], one per piece of it."""
        w = np.ascontiguousarray(world, np.float32).reshape(-1, 16)
        self._ck(lib().surtr_scene_transform_compound(self._h, ctypes.c_uint32(int(compound)), ctypes.c_uint32(w.shape[0]), _p(w)))

    def _targets_mask(self, t, outside):
        """The `outside` bytes of a fracture call over compounds t, checked against the compound table: one byte per piece of t."""
        om = None if outside is None else np.ascontiguousarray(outside, np.uint8).reshape(-1)
        if om is not None:
            co = self.scene_compounds()
            if any(not 0 <= int(c) < co.shape[0] - 1 for c in t) or om.shape[0] != sum(int(co[int(c) + 1]) - int(co[int(c)]) for c in t):
                raise SurtrError(E_INVALID, "outside holds %d bytes" % om.shape[0])
        return om

    def _scene_fracture(self, kind, targets, cell_begin, cell_end, outside, flags, sync):
        """The three fracture entrances: kind "event" (targets: one compound), "bodies" (a list) or "impacts" (a list per impact).
        sync -> Counts; else the _async symbol, and nothing waits for the event."""
        if kind == "event":
            t = [int(targets)]
            head = [ctypes.c_uint32(t[0])]
        elif kind == "bodies":
            t = np.ascontiguousarray(targets, np.uint32).reshape(-1)
            head = [ctypes.c_uint32(t.shape[0]), _p(t)]
        else:
            to, t = _impact_targets(targets)
            head = [ctypes.c_uint32(to.shape[0] - 1), _p(to), _p(t)]
        om = self._targets_mask(t, outside)
        args = [self._h] + head + [ctypes.c_uint32(cell_begin), ctypes.c_uint32(cell_end), _p(om), ctypes.c_uint32(flags)]
        if not sync:
            return self._ck(getattr(lib(), "surtr_scene_fracture_%s_async" % kind)(*args))
        c = Counts()
        self._ck(getattr(lib(), "surtr_scene_fracture_" + kind)(*args, ctypes.byref(c)))
        return c

    def scene_fracture_event(self, compound, cell_begin, cell_end, outside=None, flags=EVT_REFIT | EVT_RENDER):
        """surtr_scene_fracture_event: the event over the pieces of one compound; outside: one byte per piece of that compound."""
        return self._scene_fracture("event", compound, cell_begin, cell_end, outside, flags, True)

    def scene_fracture_event_async(self, compound, cell_begin, cell_end, outside=None, flags=EVT_REFIT | EVT_RENDER):
        self._scene_fracture("event", compound, cell_begin, cell_end, outside, flags, False)

    def scene_fracture_bodies(self, compounds, cell_begin, cell_end, outside=None, flags=EVT_REFIT | EVT_RENDER):
        """surtr_scene_fracture_bodies: one event over the pieces of several compounds (strictly descending); outside: one byte per
        piece of the listed compounds, concatenated in the order given (what scene_outside returns)."""
        return self._scene_fracture("bodies", compounds, cell_begin, cell_end, outside, flags, True)

    def scene_fracture_bodies_async(self, compounds, cell_begin, cell_end, outside=None, flags=EVT_REFIT | EVT_RENDER):
        self._scene_fracture("bodies", compounds, cell_begin, cell_end, outside, flags, False)

    def _two_call_bytes(self, symbol, args, capacity):
        """Count-then-fill of a byte mask: capacity is the bytes to offer (None: what the sizes call asks for)."""
        n = ctypes.c_uint32()
        self._ck(getattr(lib(), symbol)(*args, ctypes.c_uint32(0), ctypes.byref(n), None))
        cap = n.value if capacity is None else int(capacity)
        out = np.zeros(max(cap, 1), np.uint8)
        self._ck(getattr(lib(), symbol)(*args, ctypes.c_uint32(cap), ctypes.byref(n), _p(out)))
        return out[:n.value].copy()

    def scene_outside(self, compounds, sphere_points, origin, radius, capacity=None):
        """surtr_scene_outside: Surtr::ConvexOutOfSphere of every resident Convex of the listed compounds, on the device -> uint8, one
        per piece, compound after compound in the order given.  capacity: the bytes to offer (None: what the call asks for)."""
        t = np.ascontiguousarray(compounds, np.uint32).reshape(-1)
        sp = np.zeros((0, 3), np.float32) if sphere_points is None else np.ascontiguousarray(sphere_points, np.float32).reshape(-1, 3)
        org = np.ascontiguousarray(origin, np.float32)
        args = [self._h, ctypes.c_uint32(t.shape[0]), _p(t), ctypes.c_uint32(sp.shape[0]), _p(sp), _p(org), ctypes.c_float(radius)]
        return self._two_call_bytes("surtr_scene_outside", args, capacity)

    def scene_outside_dev(self, compounds, n_sphere, dev_sphere_points, origin, radius, dev_outside, capacity):
        """surtr_scene_outside_dev: cloud and mask in device memory, on the context's stream; nothing is read back."""
        t = np.ascontiguousarray(compounds, np.uint32).reshape(-1)
        org = np.ascontiguousarray(origin, np.float32)
        self._ck(lib().surtr_scene_outside_dev(self._h, ctypes.c_uint32(t.shape[0]), _p(t), ctypes.c_uint32(int(n_sphere)), ctypes.c_void_p(dev_sphere_points),
                                               _p(org), ctypes.c_float(radius), ctypes.c_void_p(dev_outside), ctypes.c_size_t(capacity)))

    # ---- several impacts in one frame (include/surtr_hip.h): `targets` is one list of compounds per impact
    def scene_fracture_impacts(self, targets, cell_begin, cell_end, outside=None, flags=EVT_REFIT | EVT_RENDER):
        """surtr_scene_fracture_impacts: one event over the targets of every impact, each over the cells of its impact's own
        placement (place_cells_impacts); outside: what scene_outside_impacts returns."""
        return self._scene_fracture("impacts", targets, cell_begin, cell_end, outside, flags, True)

    def scene_fracture_impacts_async(self, targets, cell_begin, cell_end, outside=None, flags=EVT_REFIT | EVT_RENDER):
        self._scene_fracture("impacts", targets, cell_begin, cell_end, outside, flags, False)

    def scene_outside_impacts(self, targets, sphere_points, origins, radii, capacity=None):
        """surtr_scene_outside_impacts: scene_outside with a sphere per impact, in one launch -> uint8, impact after impact, each as
        scene_outside returns it.  sphere_points: one cloud per impact (None or empty: no points)."""
        to, t = _impact_targets(targets)
        k, so, sp, org, rad = _impact_spheres(sphere_points, origins, radii, to.shape[0] - 1)
        if k != to.shape[0] - 1:
            raise SurtrError(E_INVALID, "%d spheres for %d impacts" % (k, to.shape[0] - 1))
        args = [self._h, ctypes.c_uint32(to.shape[0] - 1), _p(to), _p(t), _p(so), _p(sp), _p(org), _p(rad)]
        return self._two_call_bytes("surtr_scene_outside_impacts", args, capacity)

    def scene_outside_impacts_dev(self, targets, sphere_off, dev_sphere_points, origins, radii, dev_outside, capacity):
        """surtr_scene_outside_impacts_dev: cloud (all impacts' points, impact i's at [sphere_off[i], sphere_off[i + 1])) and mask in
        device memory, on the context's stream; nothing is read back."""
        to, t = _impact_targets(targets)
        so = np.ascontiguousarray(sphere_off, np.uint32).reshape(-1)
        org = np.ascontiguousarray(origins, np.float32).reshape(-1, 3)
        rad = np.ascontiguousarray(radii, np.float32).reshape(-1)
        if not so.shape[0] - 1 == org.shape[0] == rad.shape[0] == to.shape[0] - 1:
            raise SurtrError(E_INVALID, "one cloud range, origin and radius per impact")
        self._ck(lib().surtr_scene_outside_impacts_dev(self._h, ctypes.c_uint32(to.shape[0] - 1), _p(to), _p(t), _p(so), ctypes.c_void_p(dev_sphere_points),
                                                       _p(org), _p(rad), ctypes.c_void_p(dev_outside), ctypes.c_size_t(capacity)))

    def scene_apply_poses(self, compounds):
        """surtr_scene_apply_poses: scene_apply_pose for several compounds with the derived data rebuilt once."""
        t = np.ascontiguousarray(compounds, np.uint32).reshape(-1)
        self._ck(lib().surtr_scene_apply_poses(self._h, ctypes.c_uint32(t.shape[0]), _p(t)))

    def scene_commit(self, compound_off, compound_piece):
        """surtr_scene_commit with the compounds event_regroup returned for the last scene event: the event's compound is erased,
        what it broke into is pushed to the back.  Returns (n_pieces, first_new_compound, n_new_compounds, src): src[p] >= 0 the
        old resident piece new piece p was, -(f + 1) fragment f."""
        co = np.ascontiguousarray(compound_off, np.uint32)
        cp = np.ascontiguousarray(compound_piece, np.int32)
        if co.shape[0] < 1 or int(co[-1]) > cp.shape[0]:
            raise SurtrError(E_INVALID, "compound_off does not fit compound_piece")
        n, first, nnew = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        src = np.zeros(int(self.scene_compounds()[-1]) + int(co[-1]) + 1, np.int32)      # resident pieces + the event's pieces at most
        self._ck(lib().surtr_scene_commit(self._h, ctypes.c_uint32(co.shape[0] - 1), _p(co), _p(cp), ctypes.byref(n), ctypes.byref(first),
                                          ctypes.byref(nnew), _p(src)))
        return n.value, first.value, nnew.value, src[:n.value].copy()

    def _compound_list(self, compounds):
        if compounds is None:
            return None, 0
        t = np.ascontiguousarray(compounds, np.uint32).reshape(-1)
        return (t if t.shape[0] else np.zeros(1, np.uint32)), t.shape[0]      # (an empty list is a list: SURTR_E_INVALID, not "all")

    def scene_fragments(self, compounds=None, render_convex=False, flags=EVT_RENDER):
        """surtr_scene_fragments: the resident pieces of the listed compounds (None: all) become the current fragments on the device,
        triangulated with EVT_RENDER; read them with download() / pack_dev() / event_mass().  -> Counts."""
        t, n = self._compound_list(compounds)
        c = Counts()
        self._ck(lib().surtr_scene_fragments(self._h, ctypes.c_uint32(n), _p(t), ctypes.c_int(int(render_convex)), ctypes.c_uint32(flags), ctypes.byref(c)))
        return c

    def scene_fragments_async(self, compounds=None, render_convex=False, flags=EVT_RENDER):
        t, n = self._compound_list(compounds)
        self._ck(lib().surtr_scene_fragments_async(self._h, ctypes.c_uint32(n), _p(t), ctypes.c_int(int(render_convex)), ctypes.c_uint32(flags)))

    def scene_fragments_ms(self):
        """Milliseconds of the last scene_fragments' copy kernel (slot 12 of surtr_kernel_times; -1 without set_profiling)."""
        ms = (ctypes.c_float * 16)()
        self._ck(lib().surtr_kernel_times(self._h, ms))
        return float(ms[12])

    def scene_commit_times(self):
        """surtr_scene_commit_times: host milliseconds of the last commit (up to the end of the gather, from there to its end)."""
        a, b = ctypes.c_float(), ctypes.c_float()
        self._ck(lib().surtr_scene_commit_times(self._h, ctypes.byref(a), ctypes.byref(b)))
        return float(a.value), float(b.value)

    # ---- per-body poses: the scene's bodies where a solver has moved them
    def scene_set_poses(self, world):
        """surtr_scene_set_poses: one rigid pose per compound, f32[n_compounds, 4, 4] in transform_pieces' layout (x' = A x + b, the
        translation in the last column)."""
        w = np.ascontiguousarray(world, np.float32).reshape(-1, 16)
        self._ck(lib().surtr_scene_set_poses(self._h, ctypes.c_uint32(w.shape[0]), _p(w)))

    def scene_poses(self):
        """surtr_scene_get_poses: f32[n_compounds, 4, 4]."""
        n = ctypes.c_uint32()
        self._ck(lib().surtr_scene_get_poses(self._h, ctypes.c_uint32(0), ctypes.byref(n), None))
        w = np.zeros((n.value, 4, 4), np.float32)
        self._ck(lib().surtr_scene_get_poses(self._h, ctypes.c_uint32(n.value), ctypes.byref(n), _p(w)))
        return w

    def scene_apply_pose(self, compound):
        """surtr_scene_apply_pose: bakes the compound's pose into its pieces (nothing at all for the identity)."""
        self._ck(lib().surtr_scene_apply_pose(self._h, ctypes.c_uint32(int(compound))))

    def scene_raycast(self, rays):
        """surtr_scene_raycast: rays f32[n, 7] against the bodies where their poses put them -> SCENE_RAY_HIT_DTYPE[n]."""
        r = np.ascontiguousarray(rays, np.float32).reshape(-1, 7)
        out = np.zeros(r.shape[0], SCENE_RAY_HIT_DTYPE)
        self._ck(lib().surtr_scene_raycast(self._h, ctypes.c_uint32(r.shape[0]), _p(r), _p(out)))
        return out

    def scene_raycast_dev(self, n_rays, dev_rays, dev_hits, capacity):
        self._ck(lib().surtr_scene_raycast_dev(self._h, ctypes.c_uint32(int(n_rays)), ctypes.c_void_p(dev_rays), ctypes.c_void_p(dev_hits),
                                               ctypes.c_size_t(capacity)))

    def scene_overlap(self, spheres, body_mass=None, min_mass=1e-4):
        """surtr_scene_overlap: spheres f32[n, 4] -> uint8[n, n_compounds]: 0 no piece of the body is touched, 1 touched, 2 touched
        but the body's mass <= min_mass (body_mass: the records of scene_mass; None: no gate)."""
        sp = np.ascontiguousarray(spheres, np.float32).reshape(-1, 4)
        m = None if body_mass is None else np.ascontiguousarray(body_mass, MASS_DTYPE)
        n = ctypes.c_uint32()
        args = [self._h, ctypes.c_uint32(sp.shape[0]), _p(sp), _p(m), ctypes.c_float(min_mass)]
        self._ck(lib().surtr_scene_overlap(*args, ctypes.byref(n), None))
        if m is not None and m.shape[0] != n.value:
            raise SurtrError(E_INVALID, "body_mass holds %d records for %d compounds" % (m.shape[0], n.value))
        out = np.zeros((sp.shape[0], n.value), np.uint8)
        self._ck(lib().surtr_scene_overlap(*args, ctypes.byref(n), _p(out)))
        return out

    def scene_overlap_dev(self, n_spheres, dev_spheres, dev_body_mask, body_capacity, dev_piece_mask=None, piece_capacity=0, dev_body_mass=None,
                          min_mass=1e-4):
        self._ck(lib().surtr_scene_overlap_dev(self._h, ctypes.c_uint32(int(n_spheres)), ctypes.c_void_p(dev_spheres), ctypes.c_void_p(dev_body_mass),
                                               ctypes.c_float(min_mass), ctypes.c_void_p(dev_piece_mask), ctypes.c_size_t(piece_capacity),
                                               ctypes.c_void_p(dev_body_mask), ctypes.c_size_t(body_capacity)))

    def scene_mass(self, set=1, density=10.0):
        """surtr_scene_mass: one MASS_DTYPE record per compound, in the body frame, added up on the device."""
        return self._mass(lib().surtr_scene_mass, set, density)

    def scene_mass_dev(self, dev_ptr, capacity, set=1, density=10.0):
        self._ck(lib().surtr_scene_mass_dev(self._h, ctypes.c_int(int(set)), ctypes.c_float(density), ctypes.c_void_p(dev_ptr),
                                            ctypes.c_size_t(capacity)))

    # ---- scene upkeep: world bounds per body; remove, append and cull bodies (include/surtr_hip.h, upkeep_dev.hip)
    def scene_bounds(self, set=1):
        """surtr_scene_bounds: one BOUNDS_DTYPE record per compound, the world-space box of the body under its pose."""
        n = ctypes.c_uint32()
        self._ck(lib().surtr_scene_bounds(self._h, ctypes.c_int(int(set)), ctypes.byref(n), None))
        out = np.zeros(n.value, BOUNDS_DTYPE)
        self._ck(lib().surtr_scene_bounds(self._h, ctypes.c_int(int(set)), ctypes.byref(n), _p(out)))
        return out

    def scene_bounds_dev(self, dev_body, body_capacity, dev_piece=None, piece_capacity=0, set=1):
        """surtr_scene_bounds_dev: the records of the compounds (and, with dev_piece, of the resident pieces) into device memory, on
        the context's stream; nothing is read back."""
        self._ck(lib().surtr_scene_bounds_dev(self._h, ctypes.c_int(int(set)), ctypes.c_void_p(dev_body), ctypes.c_size_t(body_capacity),
                                              ctypes.c_void_p(dev_piece), ctypes.c_size_t(piece_capacity)))

    # ---- scene contacts: bodies within a margin of each other, through which pieces, how far apart, where (contact_dev.hip)
    def scene_contacts(self, margin):
        """surtr_scene_contacts: one CONTACT_DTYPE record per reported pair of pieces of two bodies, ascending by (piece_a, piece_b)."""
        n = ctypes.c_uint32()
        self._ck(lib().surtr_scene_contacts(self._h, ctypes.c_float(margin), ctypes.byref(n), None))
        out = np.zeros(n.value, CONTACT_DTYPE)
        if n.value:
            self._ck(lib().surtr_scene_contacts(self._h, ctypes.c_float(margin), ctypes.byref(n), _p(out)))
        return out

    def scene_contacts_totals(self, margin):
        """surtr_scene_contacts_totals: the header of a run (one CONTACT_HEADER_DTYPE record): records, candidate body and piece
        pairs, bodies and pieces of the scene."""
        h = np.zeros(1, CONTACT_HEADER_DTYPE)
        self._ck(lib().surtr_scene_contacts_totals(self._h, ctypes.c_float(margin), _p(h)))
        return h[0]

    def scene_contacts_dev(self, margin, dev_ptr, capacity):
        """surtr_scene_contacts_dev: a 64-byte header (CONTACT_HEADER_DTYPE), then the records, into `capacity` bytes of device
        memory, on the context's stream; nothing is read back."""
        self._ck(lib().surtr_scene_contacts_dev(self._h, ctypes.c_float(margin), ctypes.c_void_p(dev_ptr), ctypes.c_size_t(capacity)))

    def scene_contacts_times(self):
        """surtr_scene_contacts_times (after set_profiling(True)): ms of bounds, pair lists, distances, gather of the last _dev call."""
        ms = np.zeros(4, np.float32)
        self._ck(lib().surtr_scene_contacts_times(self._h, _p(ms)))
        return ms

    def scene_remove(self, compounds):
        """surtr_scene_remove: erases the listed compounds (any order).  Returns (n_pieces, src): src[p] the old resident piece of
        new piece p."""
        t = np.ascontiguousarray(compounds, np.uint32).reshape(-1)
        n = ctypes.c_uint32()
        src = np.zeros(int(self.scene_compounds()[-1]) + 1, np.int32)
        self._ck(lib().surtr_scene_remove(self._h, ctypes.c_uint32(t.shape[0]), _p(t if t.shape[0] else np.zeros(1, np.uint32)), ctypes.byref(n), _p(src)))
        return n.value, src[:n.value].copy()

    def scene_append(self, bodies, world=None):
        """surtr_scene_append: bodies is a list of bodies, each a list of pieces {'mesh', 'conv'} (solids as upload_pieces takes
        them); world: f32[n_bodies, 4, 4] or None (identity).  Returns the number of the first new compound."""
        off = np.zeros(len(bodies) + 1, np.uint32)
        off[1:] = np.cumsum([len(b) for b in bodies])
        flat = [p for b in bodies for p in b]
        if not flat:
            raise SurtrError(E_INVALID, "no piece to append")
        m = pack_solids([p["mesh"] for p in flat])
        c = pack_solids([p["conv"] for p in flat])
        w = None if world is None else np.ascontiguousarray(world, np.float32).reshape(-1, 16)
        if w is not None and w.shape[0] != len(bodies):
            raise SurtrError(E_INVALID, "%d poses for %d bodies" % (w.shape[0], len(bodies)))
        first = ctypes.c_uint32()
        self._ck(lib().surtr_scene_append(self._h, ctypes.c_uint32(len(bodies)), _p(off), _p(m[0]), _p(m[1]), _p(m[2]), _p(m[3]),
                                          _p(c[0]), _p(c[1]), _p(c[2]), _p(c[3]), _p(w), ctypes.byref(first)))
        return first.value

    def scene_cull(self, min_mass=1e-4, keep_box=None, set=1, density=10.0, apply=True):
        """surtr_scene_cull: marks the bodies of mass <= min_mass (CULL_LIGHT) and those whose Convex bounds are disjoint from
        keep_box = (lo xyz, hi xyz) (CULL_OUTSIDE) on the device and, with apply, removes them.  Returns (reason uint8[n_compounds] as
        of before the removal, n_removed).  If every body is marked nothing is removed and SurtrError(E_INVALID) carries the reasons
        in its `reason` attribute."""
        kb = None if keep_box is None else np.ascontiguousarray(keep_box, np.float32).reshape(6)
        n, removed = ctypes.c_uint32(), ctypes.c_uint32()
        args = [self._h, ctypes.c_int(int(set)), ctypes.c_float(density), ctypes.c_float(min_mass), _p(kb)]
        self._ck(lib().surtr_scene_cull(*args, ctypes.c_int(0), ctypes.byref(n), None, ctypes.byref(removed)))
        reason = np.zeros(max(n.value, 1), np.uint8)
        rc = lib().surtr_scene_cull(*args, ctypes.c_int(int(bool(apply))), ctypes.byref(n), _p(reason), ctypes.byref(removed))
        if rc:
            e = SurtrError(rc, lib().surtr_last_error(self._h).decode())
            e.reason = reason[:n.value].copy()
            raise e
        return reason[:n.value].copy(), removed.value

    def upload_stats(self):
        ms, na = ctypes.c_float(), ctypes.c_uint32()
        self._ck(lib().surtr_upload_stats(self._h, ctypes.byref(ms), ctypes.byref(na)))
        return float(ms.value), int(na.value)

    def clip_polyhedron(self, solid, planes):
        pos = np.ascontiguousarray(solid["pos"], np.float32).reshape(-1, 3)
        off = np.ascontiguousarray(solid["off"], np.uint32)
        nbr = np.ascontiguousarray(solid["nbr"], np.int32)
        pl = np.ascontiguousarray(planes, np.float32).reshape(-1, 4)
        nv = ctypes.c_uint32()
        nh = ctypes.c_uint32()
        args = [self._h, ctypes.c_uint32(pos.shape[0]), _p(pos), _p(off), _p(nbr), ctypes.c_uint32(pl.shape[0]), _p(pl)]
        self._ck(lib().surtr_clip_polyhedron(*args, ctypes.byref(nv), ctypes.byref(nh), None, None, None))
        opos = np.zeros((nv.value, 3), np.float32)
        ooff = np.zeros(nv.value + 1, np.uint32)
        onbr = np.zeros(nh.value, np.int32)
        self._ck(lib().surtr_clip_polyhedron(*args, ctypes.byref(nv), ctypes.byref(nh), _p(opos), _p(ooff), _p(onbr)))
        return {"pos": opos, "off": ooff, "nbr": onbr}


_FIELDS = [("frag_ids", np.int32, lambda c: 3 * c.n_frag), ("mesh_vert_off", np.uint32, lambda c: c.n_frag + 1),
           ("mesh_pos", np.float32, lambda c: 3 * c.mesh_verts), ("mesh_nbr_off", np.uint32, lambda c: c.mesh_verts + 1),
           ("mesh_nbr", np.int32, lambda c: c.mesh_nbrs), ("conv_vert_off", np.uint32, lambda c: c.n_frag + 1),
           ("conv_pos", np.float32, lambda c: 3 * c.conv_verts), ("conv_nbr_off", np.uint32, lambda c: c.conv_verts + 1),
           ("conv_nbr", np.int32, lambda c: c.conv_nbrs), ("vnc", np.float32, lambda c: 9 * c.mesh_verts),
           ("idx_off", np.uint32, lambda c: c.n_frag + 1), ("idx", np.uint32, lambda c: c.n_idx),
           ("frag_status", np.uint32, lambda c: c.n_frag)]


def alloc_fragments(c):
    return {name: np.zeros(max(int(size(c)), 0), dt) for name, dt, size in _FIELDS}


def _frag_struct(out):
    fr = Fragments()
    for name, _, _ in _FIELDS:
        setattr(fr, name, out[name].ctypes.data)
    return fr


def shape_fragments(out):
    out = dict(out)
    out["frag_ids"] = out["frag_ids"].reshape(-1, 3)
    out["mesh_pos"] = out["mesh_pos"].reshape(-1, 3)
    out["conv_pos"] = out["conv_pos"].reshape(-1, 3)
    out["vnc"] = out["vnc"].reshape(-1, 9)
    return out


def unpack_blob(host_blob):
    """host_blob: contiguous uint8 numpy array holding one packed fragment blob."""
    b = np.ascontiguousarray(host_blob, np.uint8)
    c = Counts()
    rc = lib().surtr_blob_unpack_host(_p(b), ctypes.c_size_t(b.nbytes), ctypes.byref(c), None)
    if rc:
        raise SurtrError(rc)
    out = alloc_fragments(c)
    fr = _frag_struct(out)
    rc = lib().surtr_blob_unpack_host(_p(b), ctypes.c_size_t(b.nbytes), ctypes.byref(c), ctypes.byref(fr))
    if rc:
        raise SurtrError(rc)
    return c, shape_fragments(out)


def blob_bytes(counts):
    return int(lib().surtr_event_blob_bytes(ctypes.byref(counts)))


def neighbors_from_mesh(pos, tris):
    """Poly::ExtractNeighborFromMesh through the C ABI (host helper)."""
    pos = np.ascontiguousarray(pos, np.float32).reshape(-1, 3)
    tris = np.ascontiguousarray(tris, np.int32).reshape(-1, 3)
    off = np.zeros(pos.shape[0] + 1, np.uint32)
    nbr = np.zeros(6 * tris.shape[0], np.int32)
    rc = lib().surtr_neighbors_from_mesh(ctypes.c_uint32(pos.shape[0]), ctypes.c_uint32(tris.shape[0]), _p(tris), _p(off), _p(nbr))
    if rc:
        raise SurtrError(rc)
    return {"pos": pos, "off": off, "nbr": nbr[:off[-1]].copy()}


def voronoi_cells(seeds):
    s = np.ascontiguousarray(seeds, np.float64).reshape(-1, 3)
    nf = ctypes.c_uint32()
    nfv = ctypes.c_uint32()
    rc = lib().surtr_voronoi_cells(ctypes.c_uint32(s.shape[0]), _p(s), ctypes.byref(nf), ctypes.byref(nfv), None, None, None, None)
    if rc:
        raise SurtrError(rc)
    cfo = np.zeros(s.shape[0] + 1, np.uint32)
    gen = np.zeros(nf.value, np.int32)
    fvo = np.zeros(nf.value + 1, np.uint32)
    verts = np.zeros((nfv.value, 3), np.float64)
    rc = lib().surtr_voronoi_cells(ctypes.c_uint32(s.shape[0]), _p(s), ctypes.byref(nf), ctypes.byref(nfv), _p(cfo), _p(gen), _p(fvo),
                                   _p(verts))
    if rc:
        raise SurtrError(rc)
    return {"cell_face_off": cfo, "face_gen": gen, "face_vert_off": fvo, "verts": verts}


def pattern_from_cells(cells):
    """First three vertices of every face, narrowed to float (what ConstructFacePlane reads)."""
    fvo = cells["face_vert_off"]
    v = cells["verts"].astype(np.float32)
    nf = fvo.shape[0] - 1
    v012 = np.stack([v[fvo[:-1] + k] for k in range(3)], 1).reshape(nf, 9)
    return cells["cell_face_off"], np.ascontiguousarray(v012)


def merge_fragments(parts):
    """Concatenates the fragment sets of consecutive cell blocks (one per rank, in rank order) into one
    set with rebased offsets: the cell-major order of Surtr::ApplyFracture (Src/Surtr.cpp:2133-2146)."""
    out = {}
    out["frag_ids"] = np.concatenate([p["frag_ids"].reshape(-1, 3) for p in parts])
    for pre in ("mesh", "conv"):
        vo, no, vbase, nbase = [np.zeros(1, np.uint32)], [np.zeros(1, np.uint32)], 0, 0
        for p in parts:
            pvo, pno = p[pre + "_vert_off"].astype(np.int64), p[pre + "_nbr_off"].astype(np.int64)
            vo.append((pvo[1:] + vbase).astype(np.uint32))
            no.append((pno[1:] + nbase).astype(np.uint32))
            vbase += int(pvo[-1])
            nbase += int(pno[-1])
        out[pre + "_vert_off"] = np.concatenate(vo)
        out[pre + "_nbr_off"] = np.concatenate(no)
        out[pre + "_pos"] = np.concatenate([p[pre + "_pos"].reshape(-1, 3) for p in parts])
        out[pre + "_nbr"] = np.concatenate([p[pre + "_nbr"] for p in parts])
    io, ibase = [np.zeros(1, np.uint32)], 0
    for p in parts:
        pio = p["idx_off"].astype(np.int64)
        io.append((pio[1:] + ibase).astype(np.uint32))
        ibase += int(pio[-1])
    out["idx_off"] = np.concatenate(io)
    out["idx"] = np.concatenate([p["idx"] for p in parts])
    out["vnc"] = np.concatenate([p["vnc"].reshape(-1, 9) for p in parts])
    return out


def cell_block(rank, world, n_cells):
    """Contiguous cell block of a rank: [floor(r*C/G), floor((r+1)*C/G))."""
    return (rank * n_cells) // world, ((rank + 1) * n_cells) // world


def balanced_blocks(costs, world):
    """Cut points of `world` CONTIGUOUS blocks of units (cells of an event, or the pairs of a pair list) with costs `costs`:
    block r = [cuts[r], cuts[r + 1]).  Order is untouched -- results concatenated in rank order are still in unit order
    (Src/Surtr.cpp:2133-2146) -- only where the cuts fall changes: cut r sits where the running cost passes r / world of the total
    (SURVEY.md section 8e).  Deterministic in its inputs, so every rank computes the same cuts from the same costs."""
    c = np.asarray(costs, np.float64)
    n = c.shape[0]
    if n == 0 or world <= 1:
        return [0] + [n] * max(world, 1)
    cum = np.concatenate([[0.0], np.cumsum(c)])
    cuts = [0]
    for r in range(1, world):
        k = int(np.searchsorted(cum, cum[-1] * r / world, side="left"))
        # the unit whose cost straddles the target goes to the side that leaves the smaller excess
        if k > 0 and k <= n and abs(cum[k - 1] - cum[-1] * r / world) <= abs(cum[min(k, n)] - cum[-1] * r / world):
            k -= 1
        cuts.append(min(max(k, cuts[-1]), n))
    cuts.append(n)
    return cuts


def pair_block(rank, world, n_pairs):
    """Contiguous block of a (fragment-major) pair list for a rank: [floor(r*P/G), floor((r+1)*P/G)) -- the sharding of a
    recursive refracture (BASELINE configs[4]): results concatenated in rank order are in list
    order, i.e. the order in which the reference's per-compound fan-outs would return them (Src/Surtr.cpp:2129-2146)."""
    return (rank * n_pairs) // world, ((rank + 1) * n_pairs) // world


def coord_key(x):
    """For tests: (sign bit, |x| * 10^6 rounded half-to-even) of a float32, the key of a coordinate in the device hull's edge keys."""
    neg, scaled = ctypes.c_uint32(), ctypes.c_uint64()
    rc = lib().surtr_coord_key(ctypes.c_float(x), ctypes.byref(neg), ctypes.byref(scaled))
    if rc:
        raise SurtrError(rc)
    return int(neg.value), int(scaled.value)


def hull_normals(points, limit):
    """VMACH::ConvexHull(points, limit) face normals (host helper)."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    cnt = ctypes.c_uint32()
    rc = lib().surtr_hull_normals(ctypes.c_uint32(p.shape[0]), _p(p), ctypes.c_uint32(limit), ctypes.c_uint32(0), None, ctypes.byref(cnt))
    if rc:
        raise SurtrError(rc)
    out = np.zeros((cnt.value, 3), np.float32)
    rc = lib().surtr_hull_normals(ctypes.c_uint32(p.shape[0]), _p(p), ctypes.c_uint32(limit), ctypes.c_uint32(cnt.value), _p(out), ctypes.byref(cnt))
    if rc:
        raise SurtrError(rc)
    return out


def kdop_planes(points, normals):
    """Kdop::Calc(Polyhedron) slab planes (host helper surtr_kdop_planes): Min plane then Max plane per normal."""
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    out = np.zeros((2 * n.shape[0], 4), np.float32)
    rc = lib().surtr_kdop_planes(ctypes.c_uint32(p.shape[0]), _p(p), ctypes.c_uint32(n.shape[0]), _p(n), _p(out))
    if rc:
        raise SurtrError(rc)
    return out


def kdop_ach_planes(points, normals, max_axis_scale, plane_gap_inv=2000.0):
    p = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = np.ascontiguousarray(normals, np.float32).reshape(-1, 3)
    out = np.zeros((2 * n.shape[0], 4), np.float32)
    rc = lib().surtr_kdop_ach_planes(ctypes.c_uint32(p.shape[0]), _p(p), ctypes.c_uint32(n.shape[0]), _p(n), ctypes.c_double(max_axis_scale),
                                     ctypes.c_float(plane_gap_inv), _p(out))
    if rc:
        raise SurtrError(rc)
    return out


def convex_out_of_sphere(solid, sphere_points, origin, radius):
    pos = np.ascontiguousarray(solid["pos"], np.float32).reshape(-1, 3)
    off = np.ascontiguousarray(solid["off"], np.uint32)
    nbr = np.ascontiguousarray(solid["nbr"], np.int32)
    sp = np.ascontiguousarray(sphere_points, np.float32).reshape(-1, 3)
    org = np.ascontiguousarray(origin, np.float32)
    out = ctypes.c_int()
    rc = lib().surtr_convex_out_of_sphere(ctypes.c_uint32(pos.shape[0]), _p(pos), _p(off), _p(nbr), ctypes.c_uint32(sp.shape[0]), _p(sp),
                                          _p(org), ctypes.c_float(radius), ctypes.byref(out))
    if rc:
        raise SurtrError(rc)
    return bool(out.value)


def regroup(convexes, piece_cell, n_outside=0, partial=False, sphere_points=None, origin=(0, 0, 0), radius=1.0):
    """Bind sets + MergeOutOfImpact + HandleConvexIsland on un-refitted Convex solids -> (compound_off, compound_piece)."""
    cvo, cpos, coff, cnbr = pack_solids(convexes)
    pc = np.ascontiguousarray(piece_cell, np.int32)
    sp = np.zeros((0, 3), np.float32) if sphere_points is None else np.ascontiguousarray(sphere_points, np.float32).reshape(-1, 3)
    org = np.ascontiguousarray(origin, np.float32)
    n = len(convexes)
    co = np.zeros(n + 2, np.uint32)
    cp = np.zeros(max(n, 1), np.int32)
    nc = ctypes.c_uint32()
    rc = lib().surtr_regroup(ctypes.c_uint32(n), ctypes.c_uint32(n_outside), _p(pc), _p(cvo), _p(cpos), _p(coff), _p(cnbr),
                             ctypes.c_int(int(partial)), ctypes.c_uint32(sp.shape[0]), _p(sp), _p(org), ctypes.c_float(radius),
                             ctypes.byref(nc), _p(co), _p(cp))
    if rc:
        raise SurtrError(rc)
    return co[:nc.value + 1].copy(), cp[:co[nc.value]].copy()


def moments(solid):
    """Poly::Moments (Src/Poly.cpp:55-87) of one solid: (volume, centroid)."""
    pos = np.ascontiguousarray(solid["pos"], np.float32).reshape(-1, 3)
    off = np.ascontiguousarray(solid["off"], np.uint32)
    nbr = np.ascontiguousarray(solid["nbr"], np.int32)
    vol = ctypes.c_double(0.0)
    cen = np.zeros(3, np.float32)
    rc = lib().surtr_moments(ctypes.c_uint32(pos.shape[0]), _p(pos), _p(off), _p(nbr), ctypes.byref(vol), _p(cen))
    if rc:
        raise SurtrError(rc)
    return float(vol.value), cen


def combine_mass(compound_off, compound_piece, records):
    """surtr_combine_mass: the records of the compounds of surtr_event_regroup (compound_off, compound_piece as it returns
    them) from the records of its pieces (the skipped resident pieces, then the fragments; see include/surtr_hip.h)."""
    co = np.ascontiguousarray(compound_off, np.uint32)
    cp = np.ascontiguousarray(compound_piece, np.int32)
    rec = np.ascontiguousarray(records, MASS_DTYPE)
    nc = max(co.shape[0] - 1, 0)
    if cp.size and (cp.min() < 0 or cp.max() >= rec.shape[0]):
        raise SurtrError(E_INVALID, "compound_piece names a piece without a record")
    out = np.zeros(nc, MASS_DTYPE)
    rc = lib().surtr_combine_mass(ctypes.c_uint32(nc), _p(co), _p(cp), _p(rec), _p(out))
    if rc:
        raise SurtrError(rc)
    return out


def read_obj(path, scale=(1, 1, 1), translate=(0, 0, 0)):
    """Surtr::LoadModelData conventions (Src/Surtr.cpp:2683-2727) for a Wavefront OBJ: (verts f32[n,3], tris i32[m,3])."""
    sc = np.asarray(scale, np.float32); tr = np.asarray(translate, np.float32)
    nv, nt = ctypes.c_uint32(0), ctypes.c_uint32(0)
    rc = lib().surtr_read_obj(path.encode(), _p(sc), _p(tr), ctypes.c_uint32(0), ctypes.c_uint32(0), None, None, ctypes.byref(nv), ctypes.byref(nt))
    if rc:
        raise SurtrError(rc)
    pos = np.zeros((nv.value, 3), np.float32); tris = np.zeros((nt.value, 3), np.int32)
    rc = lib().surtr_read_obj(path.encode(), _p(sc), _p(tr), nv, nt, _p(pos), _p(tris), ctypes.byref(nv), ctypes.byref(nt))
    if rc:
        raise SurtrError(rc)
    return pos, tris


def write_obj(path, fragments):
    """One OBJ object per fragment from the render buffers of engine.download()."""
    fr = fragments
    ids = np.ascontiguousarray(fr["frag_ids"], np.int32)
    rc = lib().surtr_write_obj(path.encode(), ctypes.c_uint32(ids.shape[0]), _p(ids), _p(np.ascontiguousarray(fr["mesh_vert_off"], np.uint32)),
                               _p(np.ascontiguousarray(fr["vnc"], np.float32)), _p(np.ascontiguousarray(fr["idx_off"], np.uint32)),
                               _p(np.ascontiguousarray(fr["idx"], np.uint32)))
    if rc:
        raise SurtrError(rc)
