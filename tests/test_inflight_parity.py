"""Every event of the several-contexts-in-flight arrangement that bench.py measures equals the event of one context run alone, bit
for bit (tests/inflight_driver.py builds bench.py's scene and arrangement, launches R rounds x E contexts and unpacks every blob).

GPU tier: the driver in a child process per configuration -- case x SURTR_CATCH_POLL (default, or 0: no catcher workgroup polls,
everything the record clipper hands on is the sweep launch's) x GPU_MAX_HW_QUEUES (the inherited value, or 32; never below 4).
One child at a time; once a child ends by a signal, with 124 / 134 / 137 / 139 or on its time limit, the remaining
parametrisations fail without starting anything.

CPU tier: the same driver in-process on the single-lane emulation (bumpy_torus(100, 60) x 256 cells, six engines, the hint at
6).  The emulation runs every launch synchronously in launch order, so this checks that the contexts keep their state apart and
that the growth paths (a context whose events change size and cell_begin without a sync) give the reference's event -- it says
nothing about timing: whether the main kernel and its catcher really overlap is the GPU tier's to find out."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DRIVER = os.path.join(HERE, "inflight_driver.py")
E = 6      # bench.py's IN_FLIGHT_DEFAULT
ROUNDS = {"whole": 30, "blocks8": 16, "mixed": 12, "refracture": 8}
TIME_LIMIT = {"whole": 600, "blocks8": 420, "mixed": 420, "refracture": 600}      # seconds per child (scene, oracle, two passes)
ABNORMAL = (124, 134, 137, 139)
_children = {"abnormal": None}


def _check_report(rep, case, rounds, catch_poll_zero):
    assert rep["error"] is None, rep["error"]
    assert rep["events_checked"] == rounds * E and rep["events_ok"] == rounds * E, (rep["events_checked"], rep["events_ok"], rep["bad"][:3])
    assert rep["pass_b"]["events_checked"] == rounds * E and rep["pass_b"]["events_ok"] == rounds * E, (rep["pass_b"], rep["bad"][:3])
    assert not rep["bad"], rep["bad"][:3]
    for ev in rep["per_event"]:
        # every workgroup of the main kernel started and signed off (the catcher's "nobody will fill it" rests on that)
        if case != "refracture" or ev["main_started"]:
            assert ev["main_started"] == ev["main_signed_off"] == ev["main_grid"], ev
            assert ev["q89"] == ev["pushed"], ev      # (split arrangement: every pair handed on goes through the list)
        else:
            # (configs[4]'s small pieces take the one-kernel arrangement: it hands on in place, the list stays empty)
            assert ev["main_signed_off"] == 0 and ev["pushed"] == 0 and ev["poll_claimed"] == 0, ev
        if catch_poll_zero:
            assert ev["poll_claimed"] == 0 and ev["q94"] >= ev["pushed"], ev      # the sweep took every hand-over
            assert ev["sweep_cursor"] >= ev["pushed"], ev


# ------------------------------------------------------------------------------------------------------------------ GPU tier
_GPU = [(case, poll, q) for case in ("whole", "blocks8") for poll in ("default", "0") for q in ("inherited", "32")] + \
       [("mixed", "default", "inherited"), ("refracture", "default", "inherited")]


@pytest.mark.gpu
@pytest.mark.parametrize("case,catch_poll,queues", _GPU, ids=["%s-poll_%s-queues_%s" % p for p in _GPU])
def test_inflight_parity_gpu(tmp_path, case, catch_poll, queues):
    """bench.py's arrangement on BASELINE configs[3] (and configs[4] for `refracture`): six contexts, R rounds, every blob checked.
    Measured on an MI355X: on `whole` the record clipper hands on 2 pairs per event and the catcher clips 37 (its own classes
    13..12 included) in every configuration -- 360 hand-overs over the 180 events of pass B, all of them the sweep's with
    CATCH_POLL=0; 24 over the 96 events of `blocks8`.  Each child takes 4-10 s; the counts are in the JSON report it writes."""
    if _children["abnormal"] is not None:
        pytest.fail("not run: an earlier child ended abnormally (%s)" % _children["abnormal"])
    env = dict(os.environ)
    env.pop("SURTR_CATCH_POLL", None)
    if catch_poll != "default":
        env["SURTR_CATCH_POLL"] = catch_poll
    if queues != "inherited":
        env["GPU_MAX_HW_QUEUES"] = queues
    assert int(env.get("GPU_MAX_HW_QUEUES", "4")) >= 4
    out = tmp_path / "report.json"
    cmd = [sys.executable, DRIVER, "--case", case, "--rounds", str(ROUNDS[case]), "--in-flight", str(E), "--json", str(out)]
    try:
        proc = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=TIME_LIMIT[case])
    except subprocess.TimeoutExpired:
        _children["abnormal"] = "%s: time limit of %d s" % (case, TIME_LIMIT[case])
        raise
    if proc.returncode < 0 or proc.returncode in ABNORMAL:
        _children["abnormal"] = "%s: exit status %d" % (case, proc.returncode)
    tail = (proc.stdout[-2000:] + "\n" + proc.stderr[-4000:])
    assert out.exists(), "no report (exit status %d):\n%s" % (proc.returncode, tail)
    rep = json.loads(out.read_text())
    print(json.dumps({k: rep.get(k) for k in ("case", "gpu_max_hw_queues", "surtr_catch_poll", "events_checked", "events_ok", "wall_s")}),
          json.dumps(rep.get("pass_b", {}).get("counters")))
    _check_report(rep, case, ROUNDS[case], catch_poll == "0")
    assert proc.returncode == 0, tail
    if case == "whole":
        assert rep["pass_b"]["counters"]["pushed"] > 0, "no pair was handed on: the catcher and the sweep went untested"


# ------------------------------------------------------------------------------------------------------------------ CPU tier
def _emul_run(emul_lib_path, oracle, monkeypatch, lib, case, catch_poll, rounds=3):
    import inflight_driver
    monkeypatch.setenv("SURTR_WAVE", "1")
    if catch_poll is None:
        monkeypatch.delenv("SURTR_CATCH_POLL", raising=False)
    else:
        monkeypatch.setenv("SURTR_CATCH_POLL", catch_poll)
    rep = inflight_driver.run(case, rounds, E, emul_lib=os.path.join(os.path.dirname(emul_lib_path), lib), torus=(100, 60), n_cells=256,
                              threads=8)
    _check_report(rep, case, rounds, catch_poll == "0")
    assert rep["ok"]
    return rep


@pytest.mark.parametrize("catch_poll", [None, "0"], ids=["poll_default", "poll_0"])
@pytest.mark.parametrize("case", ["whole", "blocks8", "mixed"])
def test_inflight_parity_emulation(emul_lib_path, oracle, monkeypatch, case, catch_poll):
    _emul_run(emul_lib_path, oracle, monkeypatch, "libsurtr_emul.so", case, catch_poll)


@pytest.mark.parametrize("catch_poll", [None, "0"], ids=["poll_default", "poll_0"])
@pytest.mark.parametrize("case", ["whole", "blocks8", "mixed"])
def test_inflight_parity_emulation_many_hand_overs(emul_lib_path, oracle, monkeypatch, case, catch_poll):
    """The small-record-room build: many pairs run out of room in the record clipper and are handed on (per event: ~170 on the
    whole event, ~20 on a 32-cell block), through the polling catcher or -- CATCH_POLL=0 -- the sweep alone."""
    rep = _emul_run(emul_lib_path, oracle, monkeypatch, "libsurtr_emul_rec.so", case, catch_poll)
    tot = rep["pass_b"]["counters"]
    assert tot["pushed"] > 10 and tot["q94"] >= tot["pushed"], tot
    if catch_poll is None:
        assert tot["poll_claimed"] > 0, tot


def test_inflight_parity_emulation_refracture(emul_lib_path, oracle, monkeypatch):
    """configs[4]'s shape, small: 12 first-level fragments x 6 cells each through fracture_pairs_async on six contexts."""
    import inflight_driver
    monkeypatch.setenv("SURTR_WAVE", "1")
    rep = inflight_driver.run("refracture", 2, E, emul_lib=os.path.join(os.path.dirname(emul_lib_path), "libsurtr_emul.so"),
                              refr=(12, 6, (48, 32)), threads=8)
    _check_report(rep, "refracture", 2, False)
    assert rep["ok"]


def test_inflight_driver_shapes():
    """The event plan of each case: blocks8 walks every context through all eight blocks; mixed starts context 0 small."""
    import inflight_driver
    p = inflight_driver.shapes("blocks8", 4096, 8, E)
    for k in range(E):
        assert sorted(p[r][k] for r in range(8)) == [(b * 512, (b + 1) * 512) for b in range(8)]
    m = inflight_driver.shapes("mixed", 4096, 4, E)
    assert [m[r][0] for r in range(4)] == [(512, 1024), (0, 4096), (2048, 4096), (512, 1024)]
    assert all(m[r][k] == (0, 4096) for r in range(4) for k in range(1, E))
