"""v = -A'q2 as a LANE of the A' product behind the two recurrences (csrc/fpsq_spmv.hip.h k_spmv_seam): ONE launch for
p1 = g - A'q1 and v in fpsq_solve_two_mixed / fpsq_ys_gs (and fpsq_qp_objgrad with rho = 0), where two single-lane products ran.
Compared, bit for bit, with the two settings that form the same vectors otherwise:

  FPSQ_TAIL_LANES=2   a single-lane product launch each for v and p1 in the seam entry points (one launch more per call);
  FPSQ_CRAIG_X=2      v ALWAYS by the stand-alone single-lane product k_spmv<1, ..>, also at the end of an evaluation: the
                      independent kernel.

At the end of an evaluation with rho > 0 the default and FPSQ_TAIL_LANES=2 launch the same kernel (v by the single-lane pass
inside k_spmv<2, .., GRAD>: three lanes side by side there were measured and lost, profiles/tail_three_lanes.md); the comparison
with FPSQ_CRAIG_X=2 is what checks that tail here, on shapes tests/test_gpu_craig_x_from_y.py does not have.

Every setting runs in a fresh child process (tests/tail_lanes_worker.py: the handle reads the variables at its creation), once
for the whole module; the cases are the smallest shapes at which the kernels take another path (see the worker's CASES), each at
delta in {0, sqrt(eps)} and rho in {0, 1}."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tail_lanes_worker import CASES, DELTAS, RHOS

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETTINGS = {"three": {}, "two": {"FPSQ_TAIL_LANES": "2"}, "alone": {"FPSQ_CRAIG_X": "2"}}
GRID = [(name, di, int(rho)) for name in CASES for di in range(len(DELTAS)) for rho in RHOS]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("tail_lanes")
    out = {}
    for tag, extra in SETTINGS.items():
        env = {k: v for k, v in os.environ.items() if k not in ("FPSQ_TAIL_LANES", "FPSQ_CRAIG_X", "FPSQ_FUSE_TAIL")}
        env.update(extra)
        path = os.path.join(str(d), tag + ".npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tail_lanes_worker.py"), path], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, (tag, r.stdout[-2000:], r.stderr[-4000:])
        with np.load(path) as z:
            out[tag] = {k: z[k] for k in z.files}
    return out


def _same(runs, key, others=("two", "alone")):
    a = runs["three"][key]
    assert np.all(np.isfinite(a)), key
    for o in others:
        assert np.array_equal(a, runs[o][key]), (key, o)


@pytest.mark.parametrize("name,di,rho", GRID)
def test_objgrad_is_bitwise_the_two_trip_and_the_stand_alone_v(runs, name, di, rho):
    key = f"{name}/{di}/{rho}/"
    assert runs["three"][key + "at_sorted"][0] >= 1  # (column-sorted padded A' blocks: the layout the kernel serves)
    for call in range(2):
        for what in ("fx", "gx", "gs", "ys", "st"):  # (st: return code, statistics and iteration counts of both recurrences)
            _same(runs, key + f"objgrad{call}/{what}")
        # v itself (the handle's Cx) is what the seam entry points hand out: the same bits from every entry point and setting
        _same(runs, key + f"mixed{call}/v")
        assert np.array_equal(runs["three"][key + f"mixed{call}/v"], runs["three"][key + f"ys_gs{call}/v"])


@pytest.mark.parametrize("name,di,rho", GRID)
def test_seam_entry_points_are_bitwise_and_one_launch_shorter(runs, name, di, rho):
    key = f"{name}/{di}/{rho}/"
    for call in range(2):
        for what in ("p1", "q1", "v", "q2", "st"):
            _same(runs, key + f"mixed{call}/{what}")
        for what in ("gs", "ys", "v", "w", "st"):
            _same(runs, key + f"ys_gs{call}/{what}")
    # the second call of a kind (iteration count known: nothing depends on timing): ONE launch for p1 and v where the other two
    # settings run two; the loop is the same loop
    for entry in ("mixed1", "ys_gs1"):
        l3, l2, l1 = (runs[s][key + entry + "/launches"] for s in ("three", "two", "alone"))
        assert l3[0] == l2[0] - 1 == l1[0] - 1, (entry, l3, l2, l1)
        assert np.array_equal(l3[1:], l2[1:]) and np.array_equal(l3[1:], l1[1:]), (entry, l3, l2, l1)


@pytest.mark.parametrize("name,di,rho", GRID)
def test_hprod_reads_the_v_the_tail_stored(runs, name, di, rho):
    key = f"{name}/{di}/{rho}/"
    for call in range(2):
        _same(runs, key + f"hprod{call}/hv")
        _same(runs, key + f"hprod{call}/st")


def test_no_bounded_wait_expired_and_no_call_was_repeated(runs):
    for tag, r in runs.items():
        for name, di, rho in GRID:
            assert tuple(r[f"{name}/{di}/{rho}/counters"]) == (0, 0, 0), (tag, name, di, rho)
