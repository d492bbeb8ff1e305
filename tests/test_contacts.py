"""surtr_scene_contacts: which bodies of the resident scene are within a margin of each other, through which pieces, how far apart,
where and along which normal (include/surtr_hip.h carries the definition; contact_ref.py is the float64 checker, which runs no GJK).

Shapes are the smallest at which each part can go wrong: feature pairs of two one-piece bodies at chosen gaps; solids of 63, 64, 65
and 129 vertices (one vertex per lane, then the strided support function) and the blob's Convex of a few hundred; posed bodies
against the same bodies baked; the 306-box lattice in compounds of 1 .. 70 pieces for the broad and mid phases; 1, 2 and 65 bodies;
capacities; refusals; the bodies a real fracture leaves.  A CPU tier on the emulation and a GPU tier that runs the same functions,
one child process per case."""
import ctypes
import textwrap

import numpy as np
import pytest
from scipy.spatial import ConvexHull

import contact_ref as CR
import test_pick_queries as PQ
import test_pieces_derived as PD
import test_scene as TS
import test_scene_poses as TSP
import test_scene_upkeep as TSU
from helpers import run_gpu_child
from surtr_amd import engine, scenes

EYE = np.eye(4, dtype=np.float32)
GAPS = (0.05, 0.5)
MARGINS = (0.1, 1.0)
# The margins of the two scenes whose distances are not chosen, picked on the reference so that no pair lies in the band about the
# margin (Reference.classes asserts it on every run, before the engine is asked): the posed lattice and the exploded fractured cube.
# Reference distances next to them: lattice under poses 8.103 | 8.758 (k = 0.067); lattice as it lies 1.036 | 1.130 (k = 0.042);
# fractured cube 0.252 | 0.462 (k = 0.008), with two pairs of Convex solids overlapping by 0.118 and 0.030.
LATTICE_MARGIN = 8.4
LATTICE_PLAIN_MARGIN = 1.08
FRACTURE_MARGIN = 0.36
FRACTURE_REST_MARGIN = 0.1      # the same bodies where the fracture left them: 0.059 | 0.142, and the pairs that share a cut face


# ------------------------------------------------------------------ solids and scenes
def hull_solid(points):
    """The convex polyhedron of the points as a solid with neighbour rings (faces triangulated by Qhull), volume positive."""
    p = np.asarray(points, np.float32)
    h = ConvexHull(p.astype(np.float64))
    assert len(h.vertices) == len(p)
    tris = h.simplices.astype(np.int32)
    out = np.cross(p[tris[:, 1]] - p[tris[:, 0]], p[tris[:, 2]] - p[tris[:, 0]]).astype(np.float64)
    flip = np.einsum("ij,ij->i", out, h.equations[:, :3]) < 0
    tris[flip] = tris[flip][:, ::-1]
    for t in (tris, tris[:, ::-1].copy()):
        s = engine.neighbors_from_mesh(p, t)
        if engine.moments(s)[0] > 0:
            return s
    raise AssertionError("no orientation with a positive volume")


def body(solid):
    return [{"mesh": solid, "conv": solid}]


def box(extent, centre):
    return scenes.box_solid(np.asarray(extent, np.float32), centre, factor=1.0)


def feature_world(kind, gap):
    """Two bodies of one piece each whose closest features are of the kind named, `gap` apart (the overlapping kinds ignore it)."""
    g = float(gap)
    if kind == "tip_to_tip":
        a = PQ.regular_tetrahedron()
        u = np.ones(3) / np.sqrt(3.0)
        b = hull_solid(2 * np.ones(3) + g * u - np.asarray(a["pos"], np.float64))
    elif kind == "vertex_to_face":
        a = hull_solid([[1, 0, 0], [-1, 1, 0.3], [-1, -1, 0.2], [-1, 0.1, -1]])
        b = box((2, 3, 3), (2 + g, 0, 0))
    elif kind == "crossed_edges":
        a = hull_solid([[1, 0, 0], [-1, 0, 0], [0, 1, -1], [0, -1, -1]])
        b = hull_solid([[0, 1, g], [0, -1, g], [1, 0, g + 1], [-1, 0, g + 1]])
    elif kind == "face_to_face":
        a, b = box((2, 2, 2), (0, 0, 0)), box((2, 2, 2), (2 + g, 0.5, -0.25))
    elif kind == "containment":
        a, b = box((4, 4, 4), (0, 0, 0)), box((1, 1, 1), (0.3, 0.2, 0.1))
    elif kind == "penetrating":
        a, b = box((2, 2, 2), (0, 0, 0)), box((2, 2, 2), (1.8, 0.3, 0.2))
    elif kind == "touching":
        a, b = box((1, 2, 2), (-0.5, 0, 0)), box((1, 2, 2), (0.5, 0, 0))
    else:
        raise KeyError(kind)
    return [body(a), body(b)]


SEPARATED = ("tip_to_tip", "vertex_to_face", "crossed_edges", "face_to_face")
OVERLAPPING = ("containment", "penetrating", "touching")
VERTEX_COUNTS = (63, 64, 65, 129)


def vertex_count_world():
    """bipyramid(k) of 63, 64, 65 and 129 vertices, each with a tetrahedron 0.05 above its upper apex: eight bodies, 6 apart."""
    world = []
    for i, nv in enumerate(VERTEX_COUNTS):
        s = PD.bipyramid(nv - 2)
        assert s["pos"].shape[0] == nv
        d = np.float32([6 * i, 0, 0])
        tet = hull_solid(np.float32([[0.05, 0.02, 1.35], [0.6, 0.1, 2.3], [-0.4, 0.5, 2.3], [-0.2, -0.6, 2.3]]) + d)
        pair = [body(TS.shifted(s, d)), body(tet)]
        world += pair if i % 2 == 0 else pair[::-1]      # (the large solid as A and as B)
    return world


def blob_world(E):
    """The blob's Convex of test_scene.bodies (a few hundred vertices) and a tetrahedron 2 above its topmost vertex."""
    b = TS.bodies(E)
    k = int(np.argmax([c["pos"].shape[0] for c in b["convexes"]]))
    conv = b["convexes"][k]
    assert conv["pos"].shape[0] > 129
    top = np.asarray(conv["pos"], np.float64)[np.argmax(conv["pos"][:, 2])]
    tet = hull_solid(top + np.float64([[0, 0, 2], [6, 1, 12], [-4, 5, 12], [-2, -6, 12]]))
    return [[{"mesh": b["meshes"][k], "conv": conv}], body(tet)]


def row_world():
    """65 bodies of one piece: a bar along 64 unit boxes, 0.2 from each: row 0 has 64 candidates, one more than a wave of columns;
    neighbouring boxes are 0.2 apart as well."""
    return [body(box((80, 1, 1), (38.4, 1.2, 0)))] + [body(box((1, 1, 1), (1.2 * i, 0, 0))) for i in range(64)]


def unpose(world, poses):
    """The bodies in their body frames: what a pose brings to where `world` has them (rounded to float)."""
    out = []
    for c, W in zip(world, poses):
        A, b = TSP.split(W)
        out.append([{k: dict(p[k], pos=((np.asarray(p[k]["pos"], np.float64) - b) @ A).astype(np.float32)) for k in ("mesh", "conv")} for p in c])
    return out


def table_of(world):
    return np.cumsum([0] + [len(c) for c in world])


_REF = {}


def reference(E, key, world, poses, margin, nonfinite=()):
    """The reference side of a scene, computed once per process and left unchanged: the world vertices are what a second engine
    holds after scene_apply_poses."""
    if (key, margin) not in _REF:
        ref = TSU.engine_of(E, world, poses)
        if poses is not None:
            ref.scene_apply_poses(list(range(len(world))))
        n = sum(len(c) for c in world)
        pos = [np.asarray(ref.download_piece(p, 1)["pos"], np.float32).reshape(-1, 3) for p in range(n)]
        ref.close()
        _REF[(key, margin)] = CR.Reference(pos, table_of(world), margin, nonfinite)
    return _REF[(key, margin)]


def contacts_of(E, world, poses, margin):
    eng = TSU.engine_of(E, world, poses)
    h = eng.scene_contacts_totals(margin)
    rec = eng.scene_contacts(margin)
    assert int(h["n_records"]) == rec.shape[0] and int(h["status"]) == 0
    assert eng.scene_contacts(margin).tobytes() == rec.tobytes(), "two calls give the same bytes"
    eng.close()
    return h, rec


def check_scene(E, key, world, poses, margin, touching=(), nonfinite=()):
    ref = reference(E, key, world, poses, margin, nonfinite)
    ref.classes(touching)                       # the cap-zero conditions, before the engine is asked
    h, rec = contacts_of(E, world, poses, margin)
    CR.check_totals(ref, h)
    CR.check_records(ref, rec, touching)
    return ref, rec


# ------------------------------------------------------------------ cases (run on the emulation and on the GPU)
def run_feature(E, kind):
    for gap in (GAPS if kind in SEPARATED else (0.0,)):
        for margin in MARGINS:
            world = feature_world(kind, gap)
            ref, rec = check_scene(E, (kind, gap), world, None, margin, touching=[(0, 1)] if kind == "touching" else ())
            if kind in SEPARATED:
                assert gap > margin or (0, 1) in ref.gap
                if (0, 1) in ref.gap:      # (boxes further apart than the margin: no candidate) -- the scene is what it was designed to be
                    assert abs(ref.gap[(0, 1)] - gap) <= 1e-6, (kind, gap, ref.gap)
                assert rec.shape[0] == (1 if gap <= margin else 0), (kind, gap, margin)
                if rec.shape[0]:
                    assert abs(float(rec["distance"][0]) - gap) <= ref.tol(0, 1)
            else:
                assert rec.shape[0] == 1
                if kind != "touching":
                    assert rec["status"][0] == engine.CONTACT_OVERLAP


def run_vertex_counts(E):
    world = vertex_count_world()
    ref, rec = check_scene(E, "vertex_counts", world, None, 0.1)
    assert rec.shape[0] == len(VERTEX_COUNTS) and sorted(ref.solid[p].pos.shape[0] for p in ref.solid if ref.solid[p].pos.shape[0] > 4) == list(VERTEX_COUNTS)


def run_blob(E):
    world = blob_world(E)
    ref, rec = check_scene(E, "blob", world, None, 4.0)
    assert rec.shape[0] == 1 and 1.0 < rec["distance"][0] <= 2.0


POSED_KINDS = ("tip_to_tip", "crossed_edges", "face_to_face")


def run_poses(E):
    """One body turned and moved by a pose of test_scene_poses, one at the bit-exact identity: checked against the reference, and
    the same bytes as the scene with the poses baked in by scene_apply_poses."""
    for i, kind in enumerate(POSED_KINDS):
        designed = feature_world(kind, 0.05)
        c = i
        cen = np.asarray(designed[1][0]["conv"]["pos"], np.float64).mean(0)
        poses = np.asarray([EYE, TSP.pose_about(TSP.rotation(TSP.AXES[c], TSP.ANGLES[c]), cen, TSP.OFFSETS[c])], np.float32)
        world = unpose(designed, poses)
        assert (poses[0] == EYE).all() and not (poses[1] == EYE).all()
        ref, rec = check_scene(E, ("posed", kind), world, poses, 0.1)
        assert rec.shape[0] == 1 and abs(float(rec["distance"][0]) - 0.05) <= 1e-4
        baked = TSU.engine_of(E, world, poses)
        baked.scene_apply_poses([0, 1])
        assert baked.scene_contacts(0.1).tobytes() == rec.tobytes()
        baked.close()


def run_lattice(E):
    """test_pick_queries.scene_d's 306 boxes in compounds of 1, 2, 61, 64, 65, 70 and 43 pieces: under test_scene_poses' poses
    (bodies moved apart) and as they lie (compounds side by side in the lattice)."""
    world, poses = TSU.lattice_world(E)
    ref, rec = check_scene(E, "lattice_posed", world, poses, LATTICE_MARGIN)
    ref2, rec2 = check_scene(E, "lattice_plain", world, None, LATTICE_PLAIN_MARGIN)
    assert len(ref.body_pairs) >= 1 and len(ref.piece_pairs) >= 8 and rec.shape[0] >= 8
    assert len(ref2.body_pairs) >= 6 and len(ref2.piece_pairs) >= 8 and rec2.shape[0] >= 4
    return ref, rec


def run_few_bodies(E):
    one = feature_world("face_to_face", 0.05)[:1]
    eng = TSU.engine_of(E, one)
    h = eng.scene_contacts_totals(1.0)
    assert eng.scene_contacts(1.0).shape[0] == 0 and [int(h[k]) for k in ("n_records", "n_body_pairs", "n_piece_pairs", "n_bodies", "n_pieces")] == [0, 0, 0, 1, 1]
    eng.close()
    two = [feature_world("face_to_face", 0.05)[0] + feature_world("face_to_face", 0.05)[1]]      # the same two pieces in ONE body: never paired
    eng = TSU.engine_of(E, two)
    assert eng.scene_contacts(1.0).shape[0] == 0
    eng.close()
    ref, rec = check_scene(E, "row", row_world(), None, 0.3)
    assert rec.shape[0] == 64 + 63 and (rec["body_a"][:64] == 0).all() and list(rec["body_b"][:64]) == list(range(1, 65))


def dev_call(eng, mem, margin, nbytes):
    buf = mem.zeros(nbytes, 0xAB)
    mem.sync()
    rc = engine.lib().surtr_scene_contacts_dev(eng._h, ctypes.c_float(margin), ctypes.c_void_p(mem.ptr(buf)), ctypes.c_size_t(nbytes))
    return rc, mem.down(buf)


def run_capacity(E, mem):
    world = row_world()
    eng = TSU.engine_of(E, world)
    want = eng.scene_contacts(0.3)
    n = want.shape[0]
    assert n > 2
    rc, got = dev_call(eng, mem, 0.3, 64 * (n + 1))                         # fits exactly
    h = got[:64].view(engine.CONTACT_HEADER_DTYPE)[0]
    assert rc == 0 and int(h["status"]) == 0 and int(h["n_records"]) == n and got[64:].tobytes() == want.tobytes()
    rc, got = dev_call(eng, mem, 0.3, 64 * n)                               # one short: the header alone, with the totals
    h2 = got[:64].view(engine.CONTACT_HEADER_DTYPE)[0]
    assert rc == 0 and int(h2["status"]) == engine.E_CAPACITY and (got[64:] == 0xAB).all()
    assert [int(h2[k]) for k in h2.dtype.names[1:7]] == [int(h[k]) for k in h.dtype.names[1:7]]
    rc, got = dev_call(eng, mem, 0.3, 63)                                   # not even the header
    assert rc == engine.E_CAPACITY and (got == 0xAB).all()
    # the host form's count-then-fill with a too-small *n
    cnt = ctypes.c_uint32(n - 1)
    out = np.full(n, 0xAB, np.uint8).repeat(64).view(engine.CONTACT_DTYPE)
    rc = engine.lib().surtr_scene_contacts(eng._h, ctypes.c_float(0.3), ctypes.byref(cnt), out.ctypes.data_as(ctypes.c_void_p))
    assert rc == engine.E_CAPACITY and cnt.value == n and (out.view(np.uint8) == 0xAB).all()
    eng.close()


def run_refusals(E):
    world = feature_world("face_to_face", 0.05)
    eng = TSU.engine_of(E, world)
    before = eng.scene_contacts(0.1)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(engine.SurtrError) as e:
            eng.scene_contacts(bad)
        assert e.value.code == engine.E_INVALID
        with pytest.raises(engine.SurtrError) as e:
            eng.scene_contacts_totals(bad)
        assert e.value.code == engine.E_INVALID
    assert eng.scene_contacts(0.1).tobytes() == before.tobytes()
    eng.close()
    empty = E.Engine(0)
    with pytest.raises(engine.SurtrError) as e:
        empty.scene_contacts(0.1)
    assert e.value.code == engine.E_STATE
    empty.close()
    # a body with a coordinate that is not finite is in no pair; everything else is unchanged
    a, b = world
    third = body(box((2, 2, 2), (-2.05, 0.1, 0.2)))
    clean, rec_clean = check_scene(E, "nonfinite_clean", [a, b, third], None, 0.1)
    ref, rec = check_scene(E, "nonfinite", [a, [TSU.with_inf(b[0])], third], None, 0.1, nonfinite=[1])
    assert rec_clean.shape[0] == 2 and rec.shape[0] == 1
    assert rec.tobytes() == rec_clean[(rec_clean["body_a"] != 1) & (rec_clean["body_b"] != 1)].tobytes()


def fractured(E):
    """The cube with an 8-cell pattern, as test_scene_poses' harness scene: four bodies of two fragments, one click (regroup, refit,
    commit), then every body moved away from the cube's centre by a pose (its centre's offset times 0.4), so that the bodies made stand apart."""
    sc = scenes.cube_scene(8)
    eng = E.Engine(0)
    eng.upload_pieces([sc["mesh"]], [sc["convex"]])
    eng.upload_pattern(sc["face_off"], sc["v012"])
    eng.place_cells(sc["scale"], sc["translate"])
    eng.fracture_event(0, 8)
    n = eng.pieces_from_event()
    eng.scene_set_compounds(list(range(0, n, 2)) + [n])
    click = TSP.python_body_click(eng, [-10.0, 0.3, 0.2], [1.0, 0.0, 0.0], 4.0, 8, False)
    assert len(click["compounds_made"]) >= 1
    table = eng.scene_compounds()
    eng.scene_apply_poses(list(range(len(table) - 1)))
    pieces = [{"mesh": eng.download_piece(p, 0), "conv": eng.download_piece(p, 1)} for p in range(int(table[-1]))]
    eng.close()
    world = [pieces[int(table[c]):int(table[c + 1])] for c in range(len(table) - 1)]
    mid = np.concatenate([np.asarray(p["conv"]["pos"], np.float64) for p in pieces]).mean(0)
    poses = []
    for c in world:
        u = np.concatenate([np.asarray(p["conv"]["pos"], np.float64) for p in c]).mean(0) - mid
        poses.append(PQ.world(np.eye(3), 0.4 * u))
    return world, np.asarray(poses, np.float32)


def run_fracture(E):
    world, poses = fractured(E)
    assert len(world) >= 5
    # where the fracture left them the bodies share their cut faces: the touching pairs are named by the reference (a gap within the
    # certificate's tolerance; the next one is 0.059) and either status is accepted for them; coplanar support points by the dozen
    ref0 = reference(E, "fractured_at_rest", world, None, FRACTURE_REST_MARGIN)
    touching = [pq for pq, g in ref0.gap.items() if abs(g) <= ref0.tol(*pq)]
    assert len(touching) >= 16 and min(abs(g) for pq, g in ref0.gap.items() if pq not in touching) > 0.05
    check_scene(E, "fractured_at_rest", world, None, FRACTURE_REST_MARGIN, touching=touching)
    ref, rec = check_scene(E, "fractured", world, poses, FRACTURE_MARGIN)
    assert rec.shape[0] >= 4
    # ImpactsFromContacts' midpoints: one per body pair, at its closest record; a sphere there of half the distance (and the
    # certificate's tolerance) touches both bodies
    eng = TSU.engine_of(E, world, poses)
    best = {}
    for r in rec:
        key = (int(r["body_a"]), int(r["body_b"]))
        if key not in best or r["distance"] < best[key]["distance"]:
            best[key] = r
    spheres = [list((np.asarray(r["point_a"], np.float64) + np.asarray(r["point_b"], np.float64)) / 2) + [float(r["distance"]) / 2 + 1e-4] for r in best.values()]
    mask = eng.scene_overlap(spheres)
    for (a, b), m in zip(best, mask):
        assert m[a] == 1 and m[b] == 1, (a, b)
    eng.close()


def run_dev_forms(E, torch):
    """The _dev form on a second stream with the in-flight hint at 6, beside a running event on another context, equals the host
    form byte for byte."""
    world, poses = TSU.lattice_world(E)
    eng = TSU.engine_of(E, world, poses)
    want = eng.scene_contacts(LATTICE_MARGIN)
    n = want.shape[0]
    sc = scenes.blob_scene(64)
    busy = E.Engine(0)
    busy.upload_pieces([sc["mesh"]], [sc["convex"]])
    busy.upload_pattern(sc["face_off"], sc["v012"])
    busy.place_cells(sc["scale"], sc["translate"])
    results = []
    for k in range(2):
        ctx = TSU.engine_of(E, world, poses)
        st = torch.cuda.Stream()
        ctx.set_stream(st.cuda_stream)
        ctx.set_events_in_flight(6)
        with torch.cuda.stream(st):
            buf = torch.full((64 * (n + 1),), 0xAB, dtype=torch.uint8, device="cuda")
            st.synchronize()
            busy.fracture_event_async(0, sc["n_cells"])
            ctx.scene_contacts_dev(LATTICE_MARGIN, buf.data_ptr(), buf.numel())
            st.synchronize()
            results.append(buf.cpu().numpy().tobytes())
        torch.cuda.synchronize()
        ctx.close()
    assert results[0] == results[1] and results[0][64:] == want.tobytes()
    h = np.frombuffer(results[0][:64], engine.CONTACT_HEADER_DTYPE)[0]
    assert int(h["status"]) == 0 and int(h["n_records"]) == n
    busy.close()
    eng.close()


# ------------------------------------------------------------------ the checker refuses what is wrong
def _designed():
    world = row_world()
    return world, 0.3


@pytest.fixture()
def checked(emul_engine):
    world, margin = _designed()
    ref, rec = check_scene(emul_engine, "row", world, None, margin)
    return ref, rec.copy()


def refused(ref, rec):
    with pytest.raises(AssertionError):
        CR.check_records(ref, rec)


def test_checker_refuses_a_witness_off_its_hull(checked):
    ref, rec = checked
    rec["point_a"][3] += np.float32(1e-3 * ref.L) * rec["normal"][3]
    refused(ref, rec)


def test_checker_refuses_a_scaled_distance(checked):
    ref, rec = checked
    rec["distance"][5] *= np.float32(1.01)
    refused(ref, rec)


def test_checker_refuses_a_negated_normal(checked):
    ref, rec = checked
    rec["normal"][7] = -rec["normal"][7]
    refused(ref, rec)


def test_checker_refuses_a_dropped_record(checked):
    ref, rec = checked
    refused(ref, np.delete(rec, 70))


def test_checker_refuses_swapped_records(checked):
    ref, rec = checked
    rec[[10, 11]] = rec[[11, 10]]
    refused(ref, rec)


def test_checker_refuses_a_same_body_pair(checked):
    ref, rec = checked
    extra = rec[:1].copy()
    extra["body_b"], extra["piece_b"] = extra["body_a"], extra["piece_a"]
    refused(ref, np.concatenate([extra, rec]))


def test_checker_refuses_exchanged_bodies(checked):
    ref, rec = checked
    rec["body_a"][2], rec["body_b"][2] = rec["body_b"][2], rec["body_a"][2]
    refused(ref, rec)


# ------------------------------------------------------------------ CPU tier (emulation)
@pytest.mark.parametrize("kind", SEPARATED + OVERLAPPING)
def test_feature_pairs(emul_engine, kind):
    run_feature(emul_engine, kind)


def test_vertex_counts_across_the_wave_edge(emul_engine):
    run_vertex_counts(emul_engine)


def test_a_solid_of_a_few_hundred_vertices(emul_engine):
    run_blob(emul_engine)


def test_posed_bodies_equal_baked_bodies(emul_engine):
    run_poses(emul_engine)


def test_broad_and_mid_phase_on_the_lattice(emul_engine):
    run_lattice(emul_engine)


def test_one_two_and_sixty_five_bodies(emul_engine):
    run_few_bodies(emul_engine)


def test_capacity_exact_fit_and_one_short(emul_engine):
    run_capacity(emul_engine, TSP.HostMem())


def test_refusals_and_a_nonfinite_body(emul_engine):
    run_refusals(emul_engine)


def test_contacts_after_a_real_fracture(emul_engine):
    run_fracture(emul_engine)


# ------------------------------------------------------------------ GPU tier
GPU_CHILD = textwrap.dedent("""
    import sys
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    import torch
    from surtr_amd import engine
    import test_scene_poses as TSP
    import test_contacts as T
    case = sys.argv[1]
    if case.startswith("feature_"):
        T.run_feature(engine, case[8:])
    elif case == "capacity":
        T.run_capacity(engine, TSP.TorchMem(torch))
    elif case == "dev_forms":
        T.run_dev_forms(engine, torch)
    else:
        getattr(T, "run_" + case)(engine)
    print("ok", case)
""")


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["feature_" + k for k in SEPARATED + OVERLAPPING] +
                         ["vertex_counts", "blob", "poses", "lattice", "few_bodies", "capacity", "refusals", "fracture", "dev_forms"])
def test_gpu_contacts(case):
    run_gpu_child(GPU_CHILD, case, 60)
