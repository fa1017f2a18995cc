"""The two CPU references away from the shipped weights, constraint parameters and options.

* The oracle's first backward sweep + linear rollout against the independent numpy restatement
  (tests/numpy_riccati.py) at solver_params.WEIGHTS / CPARAMS, at dt = 0.02 and 0.004, from warm-start
  controls that put friction-pyramid rows on both branches of the relaxed barrier (g > delta: -log g;
  g <= delta: the quadratic extension, ConstraintsBase.h:204-263) — 1e-9 relative, as
  test_oracle_solver.test_first_sweep_matches_numpy_riccati at the defaults.
* Every case of tests/test_gpu_parameters.py on the oracle alone: the path the case is there for is
  taken (the ReB schedule moves rows apart and hits the grf_delta_min clamp, td_sigma_max caps the
  penalty, the multipliers move, early exits stop elements at different iterations), and every
  branch decision repeats under a 1e-15 relative change of x0, so the GPU comparison needs no
  screening of elements.
"""
import numpy as np
import pytest

import numpy_riccati as NR
import oracle_lib as O
import solver_params as SP
from hsddp import synthetic as syn


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


SWEEP_SHAPES = [("trot", 2, 8, 0.01), ("jump", 8, 4, 0.01), ("pronk", 3, 4, 0.02), ("trot", 3, 5, 0.004)]


def sweep_problem(gait, P, N, dt):
    """B = 3 with the warm-start controls of solver_params.warm_controls; the constraint parameters
    of the sweep comparisons (CPARAMS with grf_eps = 0.3)."""
    prob = syn.make_batch(3, P, N, gait, dt=dt)
    prob["Ubar"] = SP.warm_controls(prob, 0.004 if gait == "pronk" else 0.002)
    return prob, SP.oracle_cparams(grf_eps=0.3)


def assert_both_branches(prob, cp):
    g = SP.pyramid_rows(prob, prob["Ubar"], cp["mu_fric"])
    above = int(np.sum(g > cp["grf_delta"]))
    assert g.size > 0 and above >= 0.2 * g.size and g.size - above >= 0.2 * g.size, (above, g.size)


def numpy_sweep(prob, b, cp, w):
    X, U, D = NR.initial_rollout(prob, b)
    return NR.sweep(prob, b, X, U, D, delta=cp["grf_delta"], eps=cp["grf_eps"], sigma=cp["td_sigma"],
                    lam=cp["td_lambda"], w=w, mu=cp["mu_fric"], ground=cp["ground_height"])


@pytest.mark.parametrize("gait,P,N,dt", SWEEP_SHAPES)
def test_first_sweep_matches_numpy_riccati_at_nondefault_parameters(gait, P, N, dt):
    prob, cp = sweep_problem(gait, P, N, dt)
    assert_both_branches(prob, cp)
    opt = O.default_options(no_early_exit=1, max_AL_iter=1, max_DDP_iter=1)
    r = O.solve_batch(prob, opt, weights=SP.WEIGHTS, cparams=cp)
    for b in range(3):
        ref = numpy_sweep(prob, b, cp, SP.WEIGHTS)
        assert _rel(r["K"][b], ref["K"]) < 1e-9
        assert _rel(r["dU"][b], ref["dU"]) < 1e-9
        assert _rel(r["dX"][b], ref["dX"]) < 1e-9


def test_numpy_restatement_defaults_are_the_oracles():
    """numpy_riccati.DEFAULT_W restates orc_default_weights; MU and the sweep's default delta, eps,
    sigma, lambda restate default_problem."""
    p, _ = O.default_problem([1])
    for k, v in NR.DEFAULT_W.items():
        got = getattr(p.w, k)
        assert (list(got) == list(v)) if hasattr(got, "__len__") else (got == v), k
    assert (p.mu_fric, p.grf_delta, p.grf_eps, p.td_sigma, p.td_lambda, p.ground_height) == (NR.MU, .1, .1, 50., 0., 0.)


def test_parameter_sets_hide_nothing():
    """No two of WEIGHTS' values are equal and none is zero."""
    flat = [float(a) for v in SP.WEIGHTS.values() for a in (v if isinstance(v, tuple) else (v,))]
    assert len(set(flat)) == len(flat) and all(a != 0 for a in flat)
    with pytest.raises(ValueError):
        O.knot_eval((1, 1, 1, 1), (1, 1, 1, 1), np.zeros(24), np.zeros(24), None, None, None, weights={"q_eul": (1, 2)})
    with pytest.raises(KeyError):
        O.default_problem([1], cparams={"mu": 0.4})


# ---- the GPU cases on the oracle alone ------------------------------------------------------------
@pytest.mark.parametrize("shape_id", SP.SHAPE_IDS)
@pytest.mark.parametrize("name", list(SP.CASES))
def test_case_takes_its_path_and_repeats_its_decisions(name, shape_id):
    case = SP.CASES[name]
    prob = SP.shape_batch(*SP.SHAPES[SP.SHAPE_IDS.index(shape_id)], dt=case["dt"])
    r = SP.oracle_solve(prob, case)
    r2 = SP.oracle_solve(prob, case, 1 + 1e-15)
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(r[f], r2[f]), f
    assert np.all(np.isfinite(r["Xbar"])) and np.all(np.isfinite(r["cost"]))
    for f in ("Xbar", "Ubar", "K", "X", "U", "dX", "dU"):
        assert _rel(r2[f], r[f]) < 1e-6, f  # (the GPU tolerance is 10 x this deviation: it stays a tight one)
    got = SP.fired(name, shape_id, r)
    assert all(got.values()), got
    if name == "alpha_reject":  # ten trials per iteration: 0.5^k > 1e-3 for k = 0 .. 9
        assert np.all(r["n_ls_trials"] == 20)
    if name == "retries":
        assert np.all(r["status"] == 0)


# ---- every non-default value matters ---------------------------------------------------------------
def _one_at_a_time():
    """(label, weights, cparams): solver_params.WEIGHTS / CPARAMS with one value back at its default."""
    out = []
    for k, v in SP.WEIGHTS.items():
        d = NR.DEFAULT_W[k]
        if isinstance(v, tuple):
            for j in range(len(v)):
                out.append((f"{k}[{j}]", {**SP.WEIGHTS, k: v[:j] + (float(d[j]),) + v[j + 1:]}, SP.CPARAMS))
        else:
            out.append((k, {**SP.WEIGHTS, k: float(d)}, SP.CPARAMS))
    p, _ = O.default_problem([1])
    for k in SP.CPARAMS:
        out.append((k, SP.WEIGHTS, {**SP.CPARAMS, k: getattr(p, k)}))
    return out


def test_every_nondefault_value_moves_the_schedule_case():
    """The comparison of the schedule case (trot 3 x 6) would notice any single weight or constraint
    parameter read from the wrong place: with that one value back at its default the oracle's own
    result moves by more than 1e-6 of the largest entry of some compared array, a thousand times
    the GPU tolerance (foot_term_cost enters the cost alone, td_sigma_max the final al_sigma)."""
    case = SP.CASES["schedule"]
    prob = SP.shape_batch(*SP.SHAPES[0])
    base = SP.oracle_solve(prob, case)
    blind = []
    for label, w, cp in _one_at_a_time():
        r = SP.oracle_solve(prob, {**case, "weights": w, "cparams": cp})
        if max(_rel(r[f], base[f]) for f in ("Xbar", "Ubar", "K", "dX", "dU", "cost", "al_sigma")) <= 1e-6:
            blind.append(label)
    assert blind == []
