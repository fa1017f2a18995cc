"""GPU checks of hsddp_set_element_budgets (T3): MultiPhaseDDP::solve's loop bounds (MultiPhaseDDP.cpp:
257, 304) per element, in one batch.

B = 6 of mixed 4 x 5 (tests/solver_params.py's smallest shape with touchdowns, resets, flight phases
and per-element references) at its non-default weights and constraint parameters with the ReB / AL
schedule on, so the update at the end of an element's last outer iteration shows in its parameters.
The elements take (max_AL, max_DDP) = (1,0), (1,1), (2,1), (2,3), (3,2), (0,2).  With early exits on
(thresholds at which some element's exit test fires before its bound, which the test asserts: the
budget and the exit flags then meet in one element) and with no_early_exit = 1:

* every element equals, bit for bit, the same element of a handle-wide solve of the same batch with
  its pair as the options — six handle-wide solves;
* every element equals the oracle's solve of that element with its pair under
  test_gpu_parameters.compare's rule (imported), and the solver-info histories have the oracle's
  lengths; iters, outer_iters, n_ls_trials exactly (compare's DECISIONS);
* with no_early_exit = 1 an element runs exactly max_AL x max_DDP inner iterations;
* NULL / NULL restores the handle-wide result bit for bit;
* B = 5 (sweep pairs whose halves have different budgets) and B = 1 alike.
"""
import os
import sys

import numpy as np
import pytest

import hsddp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import oracle_lib as O  # noqa: E402
import solver_params as SP  # noqa: E402
from test_gpu_parameters import compare  # noqa: E402

pytestmark = pytest.mark.gpu

BUDGETS = [(1, 0), (1, 1), (2, 1), (2, 3), (3, 2), (0, 2)]
# solver_params' exit thresholds fire only after more iterations than these budgets allow; these are
# loose enough that the elements with (2,3) and (3,2) stop before their bounds (asserted below)
EXIT_THRESHOLDS = {"cost_thresh": 0.9, "dynamics_feas_thresh": 0.5, "tconstr_thresh": 0.05, "pconstr_thresh": 0.5}
MODES = {"fixed": {**SP.SCHEDULE, "no_early_exit": 1},
         "exits": {**{k: v for k, v in SP._EXITS.items() if not k.startswith("max_")}, **EXIT_THRESHOLDS}}
FIELDS = ("Xbar", "Ubar", "K", "X", "U", "Defect", "dX", "dU", "cost", "feas", "merit", "max_tconstr", "max_pconstr",
          "iters", "outer_iters", "status", "n_ls_trials", "reb_delta", "reb_eps", "td_mask", "al_sigma", "al_lambda",
          "grf_g", "td_h")


def _prob(B):
    from hsddp import synthetic as syn
    gait, P, N, mixed = SP.SHAPES[SP.SHAPE_IDS.index("mixed4x5")]
    return syn.make_batch(B, P, N, gait, mixed=mixed)


def _solver(prob, opts):
    return hsddp.Solver(prob, hsddp.load_settings(**opts), cparams=SP.hsddp_cparams(), weights=SP.hsddp_weights())


def _snapshot(s):
    out = {**s.trajectory(), **s.working(), **s.element_info(), **s.constraint_params(), **s.constraint_values()}
    out["hist"] = s.solver_info(16)
    return out


def _differences(a, b, e):
    bad = [f for f in FIELDS if not np.array_equal(a[f][e], b[f][e], equal_nan=True)]
    bad += ["hist_" + k for k in a["hist"] if not np.array_equal(a["hist"][k][e], b["hist"][k][e])]
    return bad


def _new_problem(s, prob):
    """the handle back at the new problem (as Solver's constructor leaves it)"""
    s.upload_problem(prob["contacts"], prob["x0"], prob["ref_x"], prob["ref_u"], prob["ref_foot"])
    s.warm_start(prob.get("Xbar"), prob.get("Ubar"), prob.get("K"))


@pytest.mark.parametrize("B", [6, 5, 1])
@pytest.mark.parametrize("mode", list(MODES))
def test_each_element_runs_its_own_budget(mode, B):
    prob = _prob(B)
    base = MODES[mode]
    budgets = BUDGETS[:B] if B > 1 else [(2, 3)]
    # handle-wide options larger than some budgets and smaller than others: not what the elements run
    A = _solver(prob, {**base, "max_AL_iter": 2, "max_DDP_iter": 2})
    A.set_element_budgets([q[0] for q in budgets], [q[1] for q in budgets])
    st = A.solve()
    a = _snapshot(A)
    bad = {}
    wide = {}
    for q in sorted(set(budgets)):  # the handle-wide solves, one per pair
        W = _solver(prob, {**base, "max_AL_iter": q[0], "max_DDP_iter": q[1]})
        W.solve()
        wide[q] = _snapshot(W)
        W.close()
    for b, q in enumerate(budgets):
        bad[b] = _differences(a, wide[q], b)
        if mode == "fixed":
            assert a["iters"][b] == q[0] * q[1], (b, q, a["iters"])
            assert a["outer_iters"][b] == q[0], (b, q, a["outer_iters"])
        assert len(a["hist"]["cost"][b]) == len(wide[q]["hist"]["cost"][b])
    assert not any(bad.values()), {k: v for k, v in bad.items() if v}
    # the host ran the largest element's iterations
    if mode == "fixed":
        assert st.outer_iterations == max(q[0] for q in budgets)
        assert st.inner_iterations == max(q[0] for q in budgets) * max(q[1] for q in budgets)
    # the oracle, element by element with its own pair
    early = 0
    for b, q in enumerate(budgets):
        opts = O.default_options(**{**base, "max_AL_iter": q[0], "max_DDP_iter": q[1]})
        kw = dict(elements=[b], weights=SP.WEIGHTS, cparams=SP.CPARAMS)
        r = O.solve_batch(prob, opts, **kw)
        r2 = O.solve_batch(dict(prob, x0=prob["x0"] * (1 + 1e-15)), opts, **kw)
        g = {f: a[f][b:b + 1] for f in FIELDS}
        g["params"] = {f: a[f][b:b + 1] for f in ("reb_delta", "reb_eps", "td_mask", "al_sigma", "al_lambda")}
        compare(g, r, r2, f"{mode} B={B} element {b} budget {q}")
        assert len(a["hist"]["cost"][b]) == len(r["solver_info"][0]), (b, q)
        early += int(r["iters"][0]) < q[0] * q[1]
    assert mode == "fixed" or early >= 1  # an exit test fired inside some element's budget
    # NULL / NULL: the handle-wide options again
    A.set_element_budgets(None, None)
    _new_problem(A, prob)
    A.solve()
    W = _solver(prob, {**base, "max_AL_iter": 2, "max_DDP_iter": 2})
    W.solve()
    a2, w = _snapshot(A), _snapshot(W)
    bad = {b: _differences(a2, w, b) for b in range(B)}
    assert not any(bad.values()), {k: v for k, v in bad.items() if v}
    A.close(); W.close()


def test_budget_refusals_leave_the_handle_unchanged():
    from hsddp._lib import ip
    import re
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "hsddp.h")).read()
    E = int(re.search(r"\bHSDDP_ERR_ARG\s*=\s*(-?\d+)", hdr).group(1))
    prob = _prob(6)
    opts = {**MODES["fixed"], "max_AL_iter": 2, "max_DDP_iter": 1}
    A, C = _solver(prob, opts), _solver(prob, opts)
    f = hsddp.lib().hsddp_set_element_budgets
    ok = np.full(6, 2, np.int32)
    neg = ok.copy(); neg[3] = -1
    big = np.full(6, 1 << 11, np.int32)
    assert f(A._h, ip(neg), ip(ok)) == E and f(A._h, ip(ok), ip(neg)) == E  # negative bounds
    assert f(A._h, ip(ok), None) == E and f(A._h, None, ip(ok)) == E        # one array missing
    assert f(A._h, ip(big), ip(big)) == E                                    # beyond the history
    for s in (A, C):
        s.solve()
    a, c = _snapshot(A), _snapshot(C)
    bad = {b: _differences(a, c, b) for b in range(6)}
    assert not any(bad.values()), {k: v for k, v in bad.items() if v}
    A.close(); C.close()
