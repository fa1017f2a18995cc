"""The sweep's wave priority by knot stage (PRIO() in knot<>, hsddp_sweep.hip) changes no result.

A knot raises its wave's issue priority for its latency chains and drops it for its dense stages
(DESIGN.md §3.1 "Wave priority").  The instruction is scalar: it ignores EXEC, orders nothing and
computes nothing, so every result must stay what it was, bit for bit.  What can go wrong is a
priority instruction the compiler moved into lane-dependent code or between a VALU write and a DPP
read, and a priority left over into the per-phase code, the retry kernels or the split's barriers.
Priority only arbitrates where two waves share a SIMD, so the shape is the smallest that forces
that on a 256-CU device: B = 4 100 = 2 050 element pairs, one wave each (1 024 SIMDs).

The batch is tests/tiled_case.py's: copies of five base problems, 2 phases x 3 knots, in an order
that makes every ordered pair of base problems sweep partners —
  0, 1, 4  trot (FR + HL, then FL + HR): paired with each other both halves are live on one trot
           mask, so both specialised knot loops run (phase_knots_masked<MASK_TROT_A / _B>)
  2        pace: masks without a loop of their own
  3        crawl: three-leg stance
and every pair of unequal masks (trot beside pace, ...) takes the runtime-mask loop.  Every copy's
record (gains, dU, cost, status and the rest: tiled_case.same) must equal its base problem's from a
B = 5 handle, which at that size is swept by the column split (k_riccati_cs): the other kernel that
shares the knot body.  Two inner iterations, no early exit.

Regularisation retries: synthetic.py has no element whose sweep fails at this size with the default
weights, and weights belong to the handle.  So the second case runs the same batch with
test_gpu_parity.py::test_retries_match_oracle's r_qJd = -0.5, under which every element's first
sweep of every iteration fails the PSD test: the first 128 failures go to k_riccati_retry, the rest
through k_riccati's in-kernel attempt loop (a failed half beside a live one, and the knot loop's
early exit).
"""
import ctypes
import functools

import numpy as np
import pytest

import hsddp
import tiled_case as TC
from hsddp import synthetic as syn

pytestmark = pytest.mark.gpu

B = 4100
OPTS = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=2)
LAYOUTS = [("trot", 2, 3), ("trot", 2, 3), ("pace", 2, 3), ("crawl", 2, 3), ("trot", 2, 3)]
R_QJD = {"default": None, "retries": -0.5}


def _weights(r_qJd):
    if r_qJd is None:
        return None
    w = hsddp.Weights()
    hsddp._lib.lib().hsddp_default_weights(ctypes.byref(w))
    w.r_qJd = r_qJd
    return w


@functools.lru_cache(None)
def _base():
    """The five base problems as an ordinary batch: one layout, per-element contacts and references."""
    prob = syn.make_layout_batch(LAYOUTS)
    for k in ("layouts", "P"):
        del prob[k]
    return prob


def _masks(contacts):
    c = np.asarray(contacts)[:-1] != 0  # (the last row is the contact after the horizon)
    return (c * (1 << np.arange(4))).sum(axis=1).tolist()


def test_base_problems_reach_the_loops():
    con = _base()["contacts"]
    assert _masks(con[0]) == _masks(con[1]) == _masks(con[4]) == [0b1001, 0b0110]  # both trot masks
    assert all(m not in (0b1001, 0b0110) and bin(m).count("1") == 2 for m in _masks(con[2]))
    assert all(bin(m).count("1") == 3 for m in _masks(con[3]))
    index = TC.draw(5, B, 0)
    pairs = {(int(index[a]), int(index[c])) for a, c in TC.sweep_pairs(index) if c >= 0}
    assert {(i, j) for i in range(5) for j in range(5)} <= pairs
    assert len(TC.sweep_pairs(index)) == 2050


@pytest.mark.parametrize("case", list(R_QJD))
def test_every_element_equals_its_base_problem(case):
    prob, w = _base(), _weights(R_QJD[case])
    small = hsddp.Solver(prob, hsddp.load_settings(**OPTS), weights=w)
    small.solve()
    snap = TC.snapshot(small)
    small.close()
    el = snap["el"]
    assert np.all(el["iters"] == 2) and np.all(np.isfinite(snap["K"])) and np.all(np.isfinite(el["cost"]))
    assert np.all(el["status"] == 0), el["status"]
    if case == "retries":
        # a sweep that succeeds after retries leaves mu / 20 > 0 as the next regularisation
        assert np.all(el["reg"] > 0), el["reg"]
    index = TC.draw(5, B, 0)
    big = hsddp.Solver(TC.tile(prob, index), hsddp.load_settings(**OPTS), weights=w)
    big.solve()
    TC.same(big, snap, index)
    big.close()
