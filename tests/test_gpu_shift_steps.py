"""The search direction (dX, dU, du) through the receding-horizon shift.

hsddp_update_problem keeps dX, dU and du between solves (the next solve rewrites them before any
trial reads them), so the shift has to move their rows with the knots, element by element, as
Trajectory::pop_front / push_back_state do (TrajectoryManagement.cpp:137,141,199,203): the next
initial rollout forms fma(0, dX, Xbar) and Ubar + 0 du, which is Xbar and Ubar only while every
entry it meets is finite — and dX is indexed b S 24 with S = Kc + P, so after a shift that changes
P an element's window at the new stride would otherwise cover rows its neighbours wrote.

  * the gather is data movement: hsddp_download_working's dX and dU after a shift equal, bit for bit,
    mpc_oracle.shift_working applied to the rows downloaded before it;
  * isolation: one element whose x0 carries a NaN at one tick leaves every other element of the
    batch bit-equal to a run without it, across shifts that change P.
"""
import os
import sys

import numpy as np
import pytest

import hsddp
from hsddp import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mpc_oracle as M  # noqa: E402
from divergence_case import scenario_batch  # noqa: E402

pytestmark = pytest.mark.gpu

# (U is left to the solve-level tests: an element whose working rows are its nominal ones shares the
# nominal buffer, whose first control row the shift zeroes)
WORK = ("X", "Defect", "dX", "dU")


def _nominal(s):
    """Xbar, Ubar of the handle (no gains: those need the new layout's contacts after a shift)"""
    Xbar, Ubar = np.empty((s.B, s.S, 24)), np.empty((s.B, s.Kc, 24))
    hsddp.check(hsddp.lib().hsddp_download_trajectory(s._h, hsddp.dp(Xbar), hsddp.dp(Ubar), None))
    return Xbar, Ubar


def _expect(before, b, horizons, reach, flags, S):
    """element b's working rows and search direction after the shift, padded with zero rows to S"""
    S0 = sum(n + 1 for n in horizons)
    X, U, D, dX, dU = M.shift_working(horizons, reach, before["X"][b][:S0], before["U"][b], before["Defect"][b][:S0],
                                      flags, dX=before["dX"][b][:S0], dU=before["dU"][b])
    pad = lambda a: np.concatenate([a, np.zeros((S - a.shape[0], 24))])  # noqa: E731
    return {"X": pad(X), "U": U, "Defect": pad(D), "dX": pad(dX), "dU": dU}


@pytest.mark.parametrize("steps", [[1, 1, 1, 1, 1, 1, 1], [3, 4, 2], [9]])
def test_shift_gathers_the_search_direction(steps):
    """tests/test_gpu_mpc.py::test_shift_matches_oracle's shifts (B, P, N = 6, 4, 5): each of the
    three lists passes from 4 to 5 phases at least once, so the state rows' element stride changes."""
    B, P, N = 6, 4, 5
    sc, prob = scenario_batch(B, P, N)
    s = hsddp.Solver(prob, hsddp.load_settings(no_early_exit=1, max_AL_iter=1, max_DDP_iter=2))
    s.solve()
    changed = 0
    for n in steps:
        before, lay0 = s.working(), s.layout()
        assert before["dX"].any() and before["dU"].any() and np.all(np.isfinite(before["dX"]))
        flags = sc.step(n)
        lay = s.shift(flags)
        changed += len(lay["horizons"]) != len(lay0["horizons"])
        after = s.working()
        for b in range(B):
            want = _expect(before, b, lay0["horizons"], lay0["reach_end"], flags, s.S)
            for f in WORK:
                assert np.array_equal(after[f][b], want[f]), (n, b, f)
        inp = sc.inputs(_nominal(s)[0][:, 0])
        s.update_problem(inp["contacts"], inp["x0"], inp["ref_x"], inp["ref_u"], inp["ref_foot"])
        kept = s.working()  # the update keeps them (multiple shooting)
        assert np.array_equal(kept["dX"], after["dX"]) and np.array_equal(kept["dU"], after["dU"])
        s.solve()
    s.close()
    assert changed >= 1


def test_shift_elements_gathers_each_elements_own_rows():
    """tests/test_gpu_layouts.py::test_shift_elements_equals_uniform_shifts' setup: group A ends on
    five phases, group B on four, so the handle's stride grows and group B's rows are padded."""
    B, P, N = 7, 4, 10
    prob = syn.make_batch(B, P, N, "trot")
    for k in ("ref_x", "ref_u", "ref_foot"):
        prob[k] = np.ascontiguousarray(np.repeat(prob[k], B, axis=0))
    flagsA, flagsB = [1, 1, 0], [0, 0, 0]
    ga = [0, 2, 3, 6]
    cc = np.array([flagsA if b in ga else flagsB for b in range(B)], np.int32)
    s = hsddp.Solver(prob, hsddp.load_settings(no_early_exit=1, max_AL_iter=1, max_DDP_iter=2))
    s.solve()
    before, lay0, S0 = s.working(), s.layout(), s.S
    assert before["dX"].any() and before["dU"].any()
    lay = s.shift_elements(cc)
    assert sorted(set(lay["n_phases"])) == [4, 5] and s.S == S0 + 1
    after = s.working()
    s.close()
    for b in range(B):
        want = _expect(before, b, lay0["horizons"], lay0["reach_end"], list(cc[b]), s.S)
        for f in WORK:
            assert np.array_equal(after[f][b], want[f]), (b, f)


def test_shift_gathers_after_a_failed_line_search():
    """tests/test_gpu_parity.py::test_failed_line_search_keeps_the_last_trial's setup: with gamma =
    1e6 every trial is rejected and the working rows stay in a buffer of their own (nominal !=
    working: the gather's second branch); with the shipped gamma the step is accepted (nominal ==
    working).  One step without a contact change, (8, 8) -> (7, 9)."""
    prob = syn.make_batch(4, 2, 8, "trot")
    split = []
    for gamma in (1e6, None):
        kw = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=1)
        if gamma:
            kw["gamma"] = gamma
        s = hsddp.Solver(prob, hsddp.load_settings(**kw))
        s.solve()
        before, lay0 = s.working(), s.layout()
        split.append(not np.array_equal(before["X"], _nominal(s)[0]))
        assert before["dX"].any() and before["dU"].any()
        lay = s.shift([0])
        assert lay["horizons"] == [7, 9]
        after = s.working()
        s.close()
        for b in range(4):
            want = _expect(before, b, lay0["horizons"], lay0["reach_end"], [0], s.S)
            for f in WORK:
                assert np.array_equal(after[f][b], want[f]), (gamma, b, f)
    assert split == [True, False]


def _loop(B, P, N, ticks, x0s=None, poison=None):
    """test_gpu_mpc.py::test_mpc_loop_matches_oracle's loop (MS 1): a full solve, then per tick one
    shift, new inputs, a solve with max_AL_iter = 2, max_DDP_iter = 1.  x0s: each tick's x0 (None:
    the shifted Xbar[0], recorded); poison = (tick, element): that x0 gets one NaN entry.  Returns
    (per-tick downloads, per-tick x0, per-tick number of phases)."""
    sc, prob = scenario_batch(B, P, N)
    s = hsddp.Solver(prob, hsddp.load_settings(MS=1))
    s.solve()
    s.set_options(hsddp.load_settings(max_AL_iter=2, max_DDP_iter=1, MS=1))
    out, used, phases = [], [], []
    for it in range(ticks):
        lay = s.shift(sc.step(1))
        x0 = _nominal(s)[0][:, 0].copy() if x0s is None else x0s[it].copy()
        used.append(x0.copy())
        if poison and poison[0] == it:
            x0[poison[1], 7] = np.nan
        inp = sc.inputs(x0)
        s.update_problem(inp["contacts"], inp["x0"], inp["ref_x"], inp["ref_u"], inp["ref_foot"])
        s.solve()  # (an error return raises)
        out.append({**s.trajectory(), **s.working(), **s.element_info(), **s.constraint_params(),
                    **s.constraint_values()})
        phases.append(len(lay["horizons"]))
    s.close()
    return out, used, phases


def test_a_non_finite_element_does_not_reach_its_neighbours():
    """B, P, N = 8, 4, 5: element 3's x0 carries a NaN at the second tick only.  Its search direction
    is non-finite after that solve; the shifts that follow change P three times (4 -> 5 -> 4 -> 5),
    and every field of every other element stays bit-equal to a loop that never saw the NaN.  Of
    element 3 itself only that a status and its finiteness are reported without an error return:
    the reference's is NaN as well."""
    B, P, N, ticks, bad, at = 8, 4, 5, 7, 3, 1
    ctl, x0s, phases = _loop(B, P, N, ticks)
    assert all(np.all(np.isfinite(x)) for x in x0s)
    got, _, phases2 = _loop(B, P, N, ticks, x0s=x0s, poison=(at, bad))
    assert phases2 == phases
    assert sum(a != b for a, b in zip(phases[at:], phases[at + 1:])) >= 2, phases  # P changes after the NaN tick
    assert not np.all(np.isfinite(got[at]["dX"][bad]))
    others = [b for b in range(B) if b != bad]
    for it, (g, c) in enumerate(zip(got, ctl)):
        assert set(g) == set(c)
        for f in g:
            assert np.array_equal(g[f][others], c[f][others]), (it, f)
        assert g["status"].shape == (B,)
