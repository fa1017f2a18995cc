"""GPU solves against the oracle away from the shipped weights, constraint parameters and options.

The shipped values coincide where the kernels rebuild them by index arithmetic (tests/solver_params.py
lists the coincidences), so a swapped index, a stale precomputed scalar (1 / delta, log delta on the
uniform-ReB fast path) or a z term dropped as structurally zero computes the shipped problem
correctly.  Every case here runs hsddp.Solver(prob, options, cparams=, weights=) and the oracle with
the same values on B = 6 of trot 3 x 6, jump 8 x 3 and mixed 4 x 5 — the smallest shapes with
touchdowns, resets, flight phases and per-element references — and compares every element:

* Xbar, Ubar, K, X, U, dX, dU and cost, feas, max_tconstr, max_pconstr within max(1e-9, 10 x the
  oracle's own deviation under x0 (1 + 1e-15)) relative to the largest entry
  (test_gpu_parity.test_fixed_iterations_match_oracle's rule);
* iters, outer_iters, status, n_ls_trials exactly;
* the ReB / AL parameters after the solve (reb_delta, reb_eps, al_sigma, al_lambda) at 1e-9, td_mask
  exactly.

No element is screened: tests/test_oracle_parameters.py checks that the oracle repeats every branch
decision of every case under the perturbation, and that each case takes the path it is there for
(solver_params.FIRED; asserted again here on the reference each comparison uses).
"""
import numpy as np
import pytest

import hsddp
import solver_params as SP

pytestmark = pytest.mark.gpu

ARRAYS = ("Xbar", "Ubar", "K", "X", "U", "dX", "dU")
SCALARS = ("cost", "feas", "max_tconstr", "max_pconstr")
DECISIONS = ("iters", "outer_iters", "status", "n_ls_trials")


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


def gpu_solve(prob, case, fp32=False):
    s = hsddp.Solver(prob, hsddp.load_settings(**case["options"]),
                     cparams=None if case["cparams"] is None else SP.hsddp_cparams(case["cparams"]),
                     weights=None if case["weights"] is None else SP.hsddp_weights(case["weights"]),
                     riccati_fp32=fp32)
    s.solve()
    out = {**s.trajectory(), **s.working(), **s.element_info(), "params": s.constraint_params(),
           "hist": s.solver_info()}
    s.close()
    return out


def problem(name, shape_id):
    case = SP.CASES[name]
    return case, SP.shape_batch(*SP.SHAPES[SP.SHAPE_IDS.index(shape_id)], dt=case["dt"])


def reference(name, shape_id, prob):
    """The oracle's solve and its perturbed twin; the case's path conditions hold on it."""
    case = SP.CASES[name]
    r, r2 = SP.oracle_solve(prob, case), SP.oracle_solve(prob, case, 1 + 1e-15)
    for f in DECISIONS:
        assert np.array_equal(r[f], r2[f]), f  # (nothing to screen)
    got = SP.fired(name, shape_id, r)
    assert all(got.values()), got
    return r, r2


def compare(g, r, r2, where):
    for f in ARRAYS + SCALARS:
        e, tol = rel(g[f], r[f]), max(1e-9, 10 * rel(r2[f], r[f]))
        print(f"{where} {f}: rel {e:.3e} (bound {tol:.3e})")
        assert e < tol, (where, f, e, tol)
    for f in DECISIONS:
        assert np.array_equal(g[f], r[f]), (where, f, g[f], r[f])
    assert np.array_equal(g["params"]["td_mask"], r["td_mask"]), where
    for f in ("reb_delta", "reb_eps", "al_sigma", "al_lambda"):
        e = rel(g["params"][f], r[f])
        print(f"{where} {f}: rel {e:.3e}")
        assert e < 1e-9, (where, f, e)


PLAIN = ["schedule", "uniform", "below_min", "below_min_schedule", "al_off", "reb_off", "both_off", "alpha_half",
         "alpha_03", "merit", "dt_coarse", "dt_fine", "single_shooting"]


@pytest.mark.parametrize("shape_id", SP.SHAPE_IDS)
@pytest.mark.parametrize("name", PLAIN)
def test_case_matches_oracle(name, shape_id):
    """schedule: update_ReB 7, update_relax 0.1, update_penalty 3 (per-row delta / eps, both clamps).
    uniform: the shipped 1 / 1 — the uniform-ReB fast path with non-default delta, eps, 1 / delta,
    log delta and mu.  below_min: grf_delta < grf_delta_min, with and without the schedule.  al_off /
    reb_off / both_off: the AL_active = 0 and ReB_active = 0 branches.  alpha_half / alpha_03: other
    line-search step sequences (ls_steps).  merit: merit_scale, merit_offset, dynamics_feas_thresh.
    dt_coarse / dt_fine: dt = 0.02 / 0.004.  single_shooting: MS = 0 with the schedule."""
    case, prob = problem(name, shape_id)
    r, r2 = reference(name, shape_id, prob)
    compare(gpu_solve(prob, case), r, r2, f"{name} {shape_id}")


@pytest.mark.parametrize("shape_id", SP.SHAPE_IDS)
def test_rejecting_line_search_runs_ten_trials(shape_id):
    """alpha = 0.5: the step sequence 1, 0.5 ... 0.5^9 > 1e-3 has ten trials, past the four of
    alpha = 0.1; gamma = 1e6 rejects them all, so two iterations run twenty and the nominal rows stay
    (quirk A2, MultiPhaseDDP.cpp:345-353)."""
    case, prob = problem("alpha_reject", shape_id)
    r, r2 = reference("alpha_reject", shape_id, prob)
    g = gpu_solve(prob, case)
    compare(g, r, r2, f"alpha_reject {shape_id}")
    assert np.all(g["n_ls_trials"] == 20)
    g0 = gpu_solve(prob, {**case, "options": {**case["options"], "max_DDP_iter": 0}})
    assert np.array_equal(g["Xbar"], g0["Xbar"]) and np.array_equal(g["Ubar"], g0["Ubar"])


@pytest.mark.parametrize("shape_id", SP.SHAPE_IDS)
def test_retries_match_oracle_at_nondefault_weights(monkeypatch, shape_id):
    """WEIGHTS with r_qJd = -0.5 and update_regularization = 3: every first sweep fails the PSD test
    and the schedule mu = 1e-3, 3e-3, 9e-3 ... runs (MultiPhaseDDP.cpp:141-181).  The parallel
    retry equals the sequential loop bit for bit, and the oracle."""
    case, prob = problem("retries", shape_id)
    r, r2 = reference("retries", shape_id, prob)
    assert np.all(r["status"] == 0)
    g = gpu_solve(prob, case)
    compare(g, r, r2, f"retries {shape_id}")
    monkeypatch.setenv("HSDDP_SEQUENTIAL_RETRY", "1")
    q = gpu_solve(prob, case)
    for f in ARRAYS + SCALARS + DECISIONS:
        assert np.array_equal(g[f], q[f]), f


@pytest.mark.parametrize("shape_id", SP.SHAPE_IDS)
def test_early_exits_match_oracle(shape_id):
    """The termination tests at other thresholds, with the schedule on: the elements stop after
    different iteration counts; the per-iteration buffers (get_solver_info) equal the oracle's entry
    for entry, as test_gpu_parity.test_solver_info_history_matches_oracle."""
    case, prob = problem("early_exits", shape_id)
    r, r2 = reference("early_exits", shape_id, prob)
    g = gpu_solve(prob, case)
    compare(g, r, r2, f"early_exits {shape_id}")
    h = g["hist"]
    for b in range(prob["batch"]):
        ref = r["solver_info"][b]
        assert len(h["cost"][b]) == len(ref) > 1, b
        got = np.stack([h[k][b] for k in ("cost", "dyn_feas", "eqn_feas", "ineq_feas")], 1)
        assert np.allclose(got, ref, rtol=1e-6, atol=1e-9), b


def test_fp32_one_iteration_at_nondefault_parameters():
    """The fp32 Riccati mode (lxx / luu rebuilt by index arithmetic and cast to float in the sweep) at
    WEIGHTS + CPARAMS, trot 3 x 6, one inner iteration, against the fp64 oracle with
    test_gpu_fp32.py's tolerances: 5e-5 on K / dU / dX / Xbar / Ubar, 5e-6 on the cost, equal
    line-search trial counts.  A wrong index gives errors of order 1.  Measured on MI355X: 3.4e-7 on K,
    2.5e-7 on dU, 3.0e-7 on dX and Xbar, 2.1e-6 on Ubar, 1.6e-7 on the cost; the fp64 path on the same
    inputs is within 7e-15."""
    case = SP._case({"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 1})
    prob = SP.shape_batch(*SP.SHAPES[0])
    r, r2 = SP.oracle_solve(prob, case), SP.oracle_solve(prob, case, 1 + 1e-15)
    compare(gpu_solve(prob, case), r, r2, "fp64 on the fp32 case's inputs")
    g = gpu_solve(prob, case, fp32=True)
    for f in ("K", "dU", "dX", "Xbar", "Ubar"):
        e = rel(g[f], r[f])
        print(f"fp32 {f}: rel {e:.3e}")
        assert e < 5e-5, (f, e)
    e = rel(g["cost"], r["cost"])
    print(f"fp32 cost: rel {e:.3e}")
    assert e < 5e-6, e
    assert np.array_equal(g["n_ls_trials"], r["n_ls_trials"])
