"""The oracle pinned to the reference's own geometry code, compiled.

`make -C oracle ref` compiles Src/Poly.cpp, Src/Kdop.cpp and Src/VMACH.cpp of the reference, unchanged but for one construct g++
rejects, against stand-in headers of ours (oracle/ref_shim) into oracle/_ref/ref_driver.  oracle/ref_compiled.py runs batches of
cases through it in a child process and compares, function by function, with the oracle call that cites the same lines:

    Poly::ClipPolyhedron -> oracle.clip            Poly::ExtractFaces -> oracle.extract_faces
    Poly::RenderPolyhedron (IsCCW, EarClipping) -> oracle.render      Poly::ExtractNeighborFromMesh -> oracle.neighbours_from_mesh
    Poly::Moments -> oracle.moments                Poly::Transform -> oracle.transform
    Kdop::KdopContainer::Calc -> oracle.kdop_planes                   the refitting step (hull normals, Calc, ClipWithPolyhedron) -> oracle.refit
    VMACH::ConvexHull's face normals -> oracle.hull_normals

Topology (rings, offsets, face loops, indices, vertex order) is compared with array_equal.  Coordinates, planes, normals and moments
are compared as numbers, exactly: both sides state the same float32 arithmetic, and over every case below (designed, fixtures,
fragments, random) the measured largest difference is 0.  The engine's results are compared with the recorded reference values
within helpers.RTOL.

Tests that need the compiled reference skip where the reference tree is absent; the others replay tests/golden/reference_compiled.npz
(the inputs and the compiled reference's outputs for the designed cases and 40 of the random clips; tests/golden/make_golden.py
--reference-compiled writes it), so the pin holds on every machine."""
import os
import textwrap

import numpy as np
import pytest

import reference_cases as C
from helpers import RTOL, run_gpu_child
from oracle import ref_compiled as RC

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "reference_compiled.npz")
ENGINE_OPS = ("clip", "faces", "render", "refit", "neighbours")


@pytest.fixture(scope="module")
def compiled_reference():
    """oracle/_ref/ref_driver, built from the reference tree; where there is no tree, the driver that an earlier build left (it
    needs nothing of the tree to run); skips where there is neither."""
    if RC.reference_present():
        return RC.build()
    if os.path.exists(RC.DRIVER):
        return RC.DRIVER
    pytest.skip("neither the reference tree nor a built oracle/_ref on this machine: the fixture-replay tests carry the pin")


@pytest.fixture(scope="module")
def recorded():
    return RC.load(FIXTURE)


def _agree(cases, results, may_leave_out):
    """Every case: the oracle against the compiled reference, exactly.  A case that has no reference result, or a different one, is
    a failure unless may_leave_out(case, reference result, oracle result) allows leaving it out; returns the names left out."""
    left_out = []
    for c, r in zip(cases, results):
        got = RC.oracle_result(c)
        try:
            assert "aborted" not in r and "failed" not in r, (c["name"], r, got["links"])
            assert RC.compare(c["op"], got, r, c["name"], exact=True) == 0.0
        except AssertionError:
            if not may_leave_out(c, r, got):
                raise
            left_out.append(c["name"])
    return left_out


def _never(c, r, got):
    return False


# ------------------------------------------------------------------------------------------------------------------ with the reference
def test_designed_cases(compiled_reference, oracle):
    """The unit box and a tetrahedron under every op; planes through a vertex, an edge and a face, exactly and within the
    reference's tolerances; planes that remove everything and nothing; two planes on an edge; a clip that leaves two islands; faces
    of 3, 4, 5, 17, 64 and 65 vertices; reflex and collinear corners; closed, open and non-manifold soups.  None is left out."""
    cases = C.designed()
    ref = RC.run(cases)
    assert _agree(cases, ref, _never) == []
    # the cases are what they were designed to be, by the compiled reference's own results
    by = {c["name"]: r for c, r in zip(cases, ref)}
    assert by["box/moments"]["vol"][0] == 1.0 and abs(by["tetrahedron/moments"]["vol"][0] - 1.0 / 6.0) < 1e-6
    assert by["box/removes-everything"]["pos"].shape[0] == 0 and by["box/removes-nothing"]["pos"].shape[0] == 8
    assert by["box/two-planes-on-an-edge"]["pos"].shape[0] == 8 and by["box/plane-through-edge-0"]["pos"].shape[0] == 6
    assert np.array_equal(by["box/plane-through-face-0"]["pos"], C.unit_box()["pos"]) and by["box/plane-through-face-7"]["pos"].shape[0] == 0
    assert by["box/plane-through-vertex-0"]["pos"].shape[0] == 8 and by["box/plane-through-vertex-5"]["pos"].shape[0] == 10
    assert by["tetrahedron/plane-through-vertex-14"]["pos"].shape[0] == 5
    for k in range(7):
        _, n = oracle.islands(by["u-prism/two-islands-%d" % k])
        assert n == 2 and by["u-prism/two-islands-%d" % k]["pos"].shape[0] == 16, k
    for n in (3, 4, 5, 17, 64, 65):
        sizes = np.diff(by["prism-%d/faces" % n]["fo"].astype(np.int64))
        assert sorted(set(sizes.tolist())) == sorted({n, 4}) and (sizes == n).sum() == (2 if n != 4 else 6)
        assert by["prism-%d/render" % n]["idx"].shape[0] == 3 * (2 * (n - 2) + 2 * n)
    assert by["reflex-corner-r0/render"]["idx"].shape[0] == 3 * (2 * 4 + 2 * 6)
    assert by["collinear-5-r0/render"]["idx"].shape[0] < 3 * (2 * 3 + 2 * 5)           # the caps have no ears: dropped
    assert by["soup/open-cube"].get("threw") or by["soup/open-cube"]["off"][-1] > 0
    assert by["soup/tetrahedron"]["off"].tolist() == [0, 3, 6, 9, 12]


def test_golden_fixtures(compiled_reference, oracle):
    """The committed fixtures that are valid solids; the degenerate ones only where the oracle says the reference stays inside its
    arrays (reference_cases.golden_cases).  None is left out."""
    cases = C.golden_cases(oracle)
    assert len(cases) >= 20
    assert _agree(cases, RC.run(cases), _never) == []


def test_scene_fragments(compiled_reference, oracle):
    """Every op on the fragments of the 12-cell blob and the 8-cell cube: faces with reflex corners, refits at limits 4, 9 and 32.
    A hull or refit may be left out only where the oracle says that the reference's limited hull used an inner point that
    FindInnerPoint never set (Src/VMACH.cpp:950-961: what it returns there is whatever its stack holds).  That happens on one
    fragment, whose first tetrahedron names one point twice, from limit 9 on; of its three cases one differs (the hull at limit 9:
    one face wound the other way) and is left out."""
    cases = C.fragment_cases(oracle)
    left_out = _agree(cases, RC.run(cases), lambda c, r, got: c["op"] in ("hull", "refit") and "aborted" not in r and got["inner_point_undefined"] > 0)
    assert len(left_out) <= 1, left_out


def test_random_clips(compiled_reference, oracle):
    """200 clips of the two scenes' fragments by 1 to 24 random planes (reference_cases.random_clips, seed 20261021).  A case may be
    left out only when the compiled reference aborts on an index outside a vector AND the oracle counts a link off the array for the
    same case; at most 2 % of them.  With these seeds the compiled reference aborts on 0 of the 200 (and the oracle counts no link
    off the array on any), 156 clips leave a solid and 21 leave it whole."""
    cases = C.random_clips(oracle)
    assert len(cases) == 200
    ref = RC.run(cases)
    left_out = _agree(cases, ref, lambda c, r, got: "aborted" in r and got["links"] > 0)
    assert len(left_out) <= 0.02 * len(cases), left_out
    assert sum(r["pos"].shape[0] > 0 for r in ref if "pos" in r) >= 150


def test_fixture_is_what_the_compiled_reference_gives(compiled_reference, oracle, recorded):
    """The committed fixture holds exactly the recorder's cases and, bit for bit, what the compiled reference returns for them."""
    cases, results = recorded
    want = C.designed() + C.recorded_random(C.random_clips(oracle))
    assert [c["name"] for c in cases] == [c["name"] for c in want]
    for c, w in zip(cases, want):
        for k in w:
            if isinstance(w[k], dict):
                assert all(np.array_equal(c[k][f], w[k][f]) for f in w[k]), (c["name"], k)
            else:
                assert np.array_equal(np.asarray(c[k]), np.asarray(w[k])), (c["name"], k)
    for c, r, now in zip(cases, results, RC.run(cases)):
        assert r.keys() == now.keys(), c["name"]
        for k in r:
            assert np.asarray(r[k]).tobytes() == np.asarray(now[k]).tobytes(), (c["name"], k)


# ------------------------------------------------------------------------------------------------------------------ without it
def test_fixture_replay_on_the_oracle(oracle, recorded):
    """The recorded cases against the oracle, exactly, with no oracle/_ref in play."""
    cases, results = recorded
    assert len(cases) >= 400 and sum(c["name"].startswith("random-") for c in cases) == C.N_RECORDED
    assert {c["op"] for c in cases} == set(RC.OPS)
    for c, r in zip(cases, results):
        assert RC.compare(c["op"], RC.oracle_result(c), r, c["name"], exact=True) == 0.0


def _mutations(cases, results):
    """(name, op, mutated result, the recorded result): each one a wrong answer that differs from the right one in one small way."""
    by = {c["name"]: (c, r) for c, r in zip(cases, results)}

    def copy(r):
        return {k: np.array(v, copy=True) for k, v in r.items()}

    out = []
    c, r = by["box/plane-through-vertex-0"]
    m = copy(r); a, b = int(m["off"][0]), int(m["off"][1]); m["nbr"][a:b] = np.roll(m["nbr"][a:b], 1)
    out.append(("a ring rotated", "clip", m, r))
    m = copy(r); a = int(m["off"][2]); m["nbr"][[a, a + 1]] = m["nbr"][[a + 1, a]]
    out.append(("two ring entries swapped", "clip", m, r))
    m = copy(r); m["pos"][3, 1] = np.nextafter(np.nextafter(m["pos"][3, 1], np.float32(np.inf)), np.float32(np.inf))
    out.append(("one coordinate off by 2 ulp", "clip", m, r))
    c, r = by["prism-5/faces"]
    m = copy(r); a, b = int(m["fo"][0]), int(m["fo"][1]); m["fi"][a:b] = m["fi"][a:b][::-1]
    out.append(("a face loop reversed", "faces", m, r))
    m = copy(r); a, b = int(m["fo"][1]), int(m["fo"][2]); m["fi"][a:b] = np.roll(m["fi"][a:b], 1)
    out.append(("a face loop started elsewhere", "faces", m, r))
    c, r = by["reflex-corner-r0/render"]
    m = copy(r); m["idx"][3:6] = m["idx"][[4, 5, 3]]
    out.append(("an index triple permuted", "render", m, r))
    m = copy(r); m["vnc"][1, 6] = np.nextafter(np.nextafter(m["vnc"][1, 6], np.float32(0)), np.float32(0))
    out.append(("one colour off by 2 ulp", "render", m, r))
    c, r = by["box/kdop-ach"]
    m = copy(r); m["planes"][3, 3] = np.nextafter(np.nextafter(m["planes"][3, 3], np.float32(np.inf)), np.float32(np.inf))
    out.append(("one plane offset off by 2 ulp", "kdop", m, r))
    c, r = by["soup/cube"]
    m = copy(r); a, b = int(m["off"][5]), int(m["off"][6]); m["nbr"][a:b] = m["nbr"][a:b][::-1]
    out.append(("a soup's ring reversed", "neighbours", m, r))
    return out


def test_the_comparison_refuses_wrong_answers(recorded):
    """Mutations of a right answer -- a ring rotated, two ring entries swapped, a face loop reversed, an index triple permuted, one
    coordinate off by 2 ulp, and four more -- are each refused by the comparison that the tests above use; the right answer passes."""
    muts = _mutations(*recorded)
    assert len(muts) >= 5
    for name, op, m, r in muts:
        assert not all(np.asarray(m[k]).tobytes() == np.asarray(r[k]).tobytes() for k in r), name
        assert RC.compare(op, r, r, name, exact=True) == 0.0
        with pytest.raises(RC.Differs):
            RC.compare(op, m, r, name, exact=True)
    # ... and a coordinate off by 2 ulp passes the engine's comparison (within RTOL), a wrong ring does not
    name, op, m, r = muts[2]
    assert 0.0 < RC.compare(op, m, r, name, exact=False, rtol=RTOL) < 1e-6
    with pytest.raises(RC.Differs):
        RC.compare(muts[0][1], muts[0][2], muts[0][3], muts[0][0], exact=False, rtol=RTOL)


# ------------------------------------------------------------------------------------------------------------------ the engine
def engine_result(eng, c):
    op = c["op"]
    if op == "clip":
        return eng.clip_polyhedron(c["solid"], c["planes"])
    if op == "faces":
        fo, fi = eng.extract_faces(c["solid"])
        return {"fo": fo, "fi": fi}
    if op == "render":
        vnc, idx = eng.triangulate(c["solid"], is_convex=bool(c["convex"]), color=c["colour"])
        return {"vnc": vnc, "idx": idx}
    if op == "refit":
        eng.set_refit_point_limit(int(c["limit"]))
        return eng.refit_solid(c["mesh"], c["convex"])
    if op == "neighbours":
        s, _ = eng.neighbors_from_mesh(c["pos"], c["tris"])
        return {"off": s["off"], "nbr": s["nbr"]}
    raise KeyError(op)


def closed_manifold(tris):
    """Every directed edge once, and its reverse too: the welded, closed, consistently wound soups that
    surtr_neighbors_from_mesh_dev is specified for (it refuses the others with SURTR_E_TOPOLOGY)."""
    t = np.asarray(tris).reshape(-1, 3)
    edges = [(int(a), int(b)) for q in t for a, b in ((q[0], q[1]), (q[1], q[2]), (q[2], q[0]))]
    return len(set(edges)) == len(edges) and all((b, a) in set(edges) for a, b in edges)


def replay_on_engine(E):
    """The recorded cases of the engine's single-solid entry points (clip_polyhedron, extract_faces, triangulate, refit_solid,
    neighbors_from_mesh: the device functions the event kernels use) against the compiled reference's recorded results: topology
    exact, coordinates within helpers.RTOL.  Where the reference threw the engine must refuse; a soup that is no closed manifold
    it may refuse with SURTR_E_TOPOLOGY, as its interface says, and must otherwise match.  Returns (cases compared, cases refused,
    largest relative difference)."""
    cases, results = RC.load(FIXTURE)
    eng = E.Engine(0)
    n, refused, worst = 0, [], 0.0
    try:
        for c, r in zip(cases, results):
            if c["op"] not in ENGINE_OPS:
                continue
            may_refuse = r.get("threw") or (c["op"] == "neighbours" and not closed_manifold(c["tris"]))
            try:
                got = engine_result(eng, c)
            except E.SurtrError as e:
                assert may_refuse and e.code == 2, (c["name"], str(e))
                refused.append(c["name"])
                continue
            assert not r.get("threw"), c["name"]
            worst = max(worst, RC.compare(c["op"], got, r, c["name"], exact=False, rtol=RTOL))
            n += 1
    finally:
        eng.close()
    assert n >= 340 and len(refused) <= 5, (n, refused)
    return n, refused, worst


def test_fixture_replay_on_the_engine(emul_engine):
    n, refused, worst = replay_on_engine(emul_engine)
    print("%d cases, %d soups refused, largest relative difference %.3g" % (n, len(refused), worst))


GPU_CHILD = textwrap.dedent("""
    import sys, time
    sys.path.insert(0, %(root)r); sys.path.insert(0, %(tests)r)
    from surtr_amd import engine
    import test_reference_compiled as T
    t0 = time.time()
    n, refused, worst = T.replay_on_engine(engine)
    print("%%d cases, %%d soups refused, largest relative difference %%.3g, seconds %%.1f" %% (n, len(refused), worst, time.time() - t0))
    print("ok", sys.argv[1])
""")


@pytest.mark.gpu
def test_gpu_fixture_replay_on_the_engine():
    run_gpu_child(GPU_CHILD, "replay", 120)
