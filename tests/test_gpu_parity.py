"""GPU parity tests: the HIP product path (through the C-ABI) against the oracle.

Tolerances (fp64): model primitives 1e-12 relative to the largest entry (different operation
order than the CasADi graph); one/three inner iterations 1e-9 relative on K, dU, dX, X, U, Xbar,
Ubar (or 10x the oracle's own deviation under a 1e-15 relative perturbation of x0, where that is
larger: three jump iterations amplify rounding to ~1e-9) and exact equality of every branch decision (line-search trial counts, iteration counts,
statuses); full solves 1e-7 relative on elements whose own oracle solution is insensitive to a
1e-15 relative perturbation of x0 (the "chaos screen": a few jump elements wander for 50
iterations and flip line-search decisions on rounding alone — the oracle disagrees with itself
there).  Full-size (B = 4096) runs are checked through size-independent properties.
"""
import numpy as np
import pytest

import hsddp
import oracle_lib as O
from hsddp import synthetic as syn

pytestmark = pytest.mark.gpu


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


# ---- model primitives ------------------------------------------------------------------------
def test_model_matches_golden(golden):
    xn = hsddp.model.dynamics(golden["x"], golden["u"], golden["c"], float(golden["dt"]))
    A, B = hsddp.model.dynamics_partial(golden["x"], golden["u"], golden["c"], float(golden["dt"]))
    assert rel(xn, golden["xn"]) < 1e-12
    for q in range(A.shape[0]):
        assert rel(A[q], golden["A"][q]) < 1e-12
        assert rel(B[q], golden["B"][q]) < 1e-12
        # compact device representation: every reference structural zero of B stays zero
        assert np.all(B[q][golden["B"][q] == 0] == 0)


def test_kinematics_and_reset_match_golden(golden):
    m = golden["fx"].shape[0]
    for leg in range(4):
        p = hsddp.model.foot_position(golden["fx"], np.full(m, leg))
        J = hsddp.model.foot_jacobian(golden["fx"], np.full(m, leg))
        assert rel(p, golden["fp"][:, leg]) < 1e-12
        assert rel(J, golden["fJ"][:, leg]) < 1e-12
    xn = hsddp.model.resetmap(golden["rx"], golden["rc"], golden["rcn"])
    Px = hsddp.model.resetmap_partial(golden["rx"], golden["rc"], golden["rcn"])
    assert rel(xn, golden["rxn"]) < 1e-12
    assert rel(Px, golden["rPx"]) < 1e-12


def test_model_edge_cases():
    # flight (no stance) and all-stance, zero batch
    x = np.zeros((2, 24)); x[:, 5] = 0.25
    u = np.ones((2, 24))
    c = np.array([[0, 0, 0, 0], [1, 1, 1, 1]], float)
    xn = hsddp.model.dynamics(x, u, c)
    for q in range(2):
        assert rel(xn[q], O.hkd_step(x[q], u[q], 0.01, c[q])) < 1e-14
    hsddp.model.dynamics(np.zeros((0, 24)), np.zeros((0, 24)), np.zeros((0, 4)))


# ---- solver ----------------------------------------------------------------------------------
def _run(prob, **kw):
    s = hsddp.Solver(prob, hsddp.load_settings(**kw))
    s.solve()
    out = {**s.trajectory(), **s.working(), **s.element_info()}
    s.close()
    return out


def _chaotic(prob, kw, elems, perturbed=False):
    """Elements whose oracle solution changes under a 1e-15 relative x0 perturbation (and, with
    perturbed=True, the perturbed oracle run)."""
    a = O.solve_batch(prob, O.default_options(**kw), n_threads=8, elements=elems)
    p2 = dict(prob); p2["x0"] = prob["x0"] * (1 + 1e-15)
    b = O.solve_batch(p2, O.default_options(**kw), n_threads=8, elements=elems)
    bad = set()
    for j, e in enumerate(elems):
        if a["n_ls_trials"][j] != b["n_ls_trials"][j] or abs(a["cost"][j] - b["cost"][j]) > 1e-8 * abs(a["cost"][j]):
            bad.add(e)
    return (a, bad, b) if perturbed else (a, bad)


def _divergence(h1, h2, tol=1e-6):
    """First solver-info entry (MultiPhaseDDP::get_solver_info, float32 cost) where two histories
    differ by more than tol relative, or the shorter length."""
    n = min(len(h1), len(h2))
    for i in range(n):
        if abs(float(h1[i]) - float(h2[i])) > tol * max(abs(float(h1[i])), 1e-30):
            return i
    return n


@pytest.mark.parametrize("n_iter", [1, 3])
@pytest.mark.parametrize("gait,P,N", [("trot", 4, 50), ("jump", 8, 25), ("pronk", 4, 20)])
def test_fixed_iterations_match_oracle(gait, P, N, n_iter):
    prob = syn.make_batch(8, P, N, gait)
    kw = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=n_iter)
    g = _run(prob, **kw)
    r = O.solve_batch(prob, O.default_options(**kw), n_threads=8)
    # the oracle's own rounding envelope: its deviation under a 1e-15 relative change of x0
    # (three jump iterations amplify rounding to ~1e-9 in dX; everywhere else it is ~1e-13)
    p2 = dict(prob); p2["x0"] = prob["x0"] * (1 + 1e-15)
    r2 = O.solve_batch(p2, O.default_options(**kw), n_threads=8)
    for f in ("Xbar", "Ubar", "K", "X", "U", "dX", "dU"):
        assert rel(g[f], r[f]) < max(1e-9, 10 * rel(r2[f], r[f])), f
    for f in ("cost", "feas", "max_tconstr"):
        assert rel(g[f], r[f]) < 1e-9, f
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], r[f]), f


@pytest.mark.parametrize("B,gait,P,N", [(1, "trot", 1, 50), (5, "trot", 2, 10), (7, "pronk", 3, 4),
                                         (9, "jump", 8, 3)])
def test_short_horizons_match_oracle(B, gait, P, N):
    """Horizons with S < 64 state slots: one k_rollout wave spans several elements (C1 is 1 x 50,
    batch 1); ragged batch sizes."""
    prob = syn.make_batch(B, P, N, gait)
    kw = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=2)
    g = _run(prob, **kw)
    r = O.solve_batch(prob, O.default_options(**kw), n_threads=8)
    for f in ("Xbar", "Ubar", "K", "X", "U", "dX", "dU"):
        assert rel(g[f], r[f]) < 1e-9, f
    for f in ("cost", "feas"):
        assert rel(g[f], r[f]) < 1e-9, f
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], r[f]), f


@pytest.mark.parametrize("gait,P,N,mixed", [("trot", 4, 50, False), ("jump", 8, 25, False),
                                              ("trot", 4, 50, True)])
def test_full_solve_matches_oracle(gait, P, N, mixed):
    prob = syn.make_batch(16, P, N, gait, mixed=mixed)
    s = hsddp.Solver(prob, hsddp.load_settings())
    s.solve()
    g = {**s.trajectory(), **s.working(), **s.element_info()}
    ghist = s.solver_info()["cost"]
    s.close()
    r, chaotic, r2 = _chaotic(prob, {}, list(range(16)), perturbed=True)
    ok = [b for b in range(16) if b not in chaotic]
    # measured on the oracle: no chaotic element on trot / mixed, one (element 2) on jump 8x25,
    # whose final cost moves 17 % under a 1e-15 relative x0 perturbation
    assert len(ok) >= 15
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f][ok], r[f][ok]), f
    for f in ("Xbar", "Ubar"):
        assert rel(g[f][ok], r[f][ok]) < 1e-7, f
    assert rel(g["cost"][ok], r["cost"][ok]) < 1e-9
    # a screened element still ends with the oracle's status and a finite trajectory, and its
    # per-iteration cost history (get_solver_info) follows the oracle's up to the entry where the
    # oracle departs from its own perturbed run; past that point the cost is not comparable
    # (measured: the GPU's rounding takes element 2 of jump 8x25 to a final cost of 9.4e3 against
    # the oracle's 1.16e3, and the perturbed oracle run to yet another)
    for b in sorted(chaotic):
        assert g["status"][b] == r["status"][b], b
        assert np.all(np.isfinite(g["Xbar"][b])) and np.all(np.isfinite(g["Ubar"][b])), b
        ho, hp, hg = r["solver_info"][b][:, 0], r2["solver_info"][b][:, 0], ghist[b]
        d = _divergence(ho, hp)
        assert d >= 2, (b, d)  # the screen is not hiding a difference from the first iterations
        assert _divergence(hg, ho) >= d, (b, d, _divergence(hg, ho))


def test_regularization_overflow_status():
    """Negative control weights make Quu indefinite for every mu <= 1e2: the element must stop
    with the reference's bad_solve outcome (MultiPhaseDDP.cpp:162-167, :421-427)."""
    prob = syn.make_batch(2, 2, 10, "trot")
    w = hsddp.Weights()
    hsddp._lib.lib().hsddp_default_weights(__import__("ctypes").byref(w))
    w.r_qJd = -1e5
    s = hsddp.Solver(prob, hsddp.load_settings(), weights=w)
    s.solve()
    info = s.element_info()
    s.close()
    assert np.all(info["status"] == 1)
    assert np.all(info["iters"] == 1)


def test_repeat_solve_is_deterministic():
    prob = syn.make_batch(64, 4, 50, "trot")
    a = _run(prob, no_early_exit=1, max_AL_iter=1, max_DDP_iter=3)
    b = _run(prob, no_early_exit=1, max_AL_iter=1, max_DDP_iter=3)
    for f in ("Xbar", "Ubar", "K", "cost"):
        assert np.array_equal(a[f], b[f]), f


def test_full_batch_properties():
    """B = 4096 (the metric config): every element runs, costs fall, gathered sample matches."""
    B = 4096
    prob = syn.make_batch(B, 4, 50, "trot")
    s = hsddp.Solver(prob, hsddp.load_settings(no_early_exit=1, max_AL_iter=1, max_DDP_iter=3))
    s.begin()
    c0 = s.element_info()["cost"].copy()
    st = s.iterate(3)
    info = s.element_info()
    tr = s.trajectory()
    s.close()
    assert np.all(np.isfinite(info["cost"])) and np.all(info["status"] == 0)
    assert np.all(info["iters"] == 3)
    assert np.mean(info["cost"] < c0) > 0.99
    assert st.n_backward_launches == 3
    # spot-check a sample of elements against the oracle: the strided eight (all even, so each the
    # first half-wave of its sweep pair and lane group 0 of its k_decide wave), then odd elements at
    # every residue mod 4 and the last element (every element: test_gpu_batch_sizes.py)
    sample = list(range(0, B, 512)) + [1, 1027, 2046, 3073, B - 1]
    assert {b % 4 for b in sample} == {0, 1, 2, 3} and sum(b % 2 for b in sample) >= 4
    r = O.solve_batch(prob, O.default_options(no_early_exit=1, max_AL_iter=1, max_DDP_iter=3),
                      n_threads=8, elements=sample)
    assert rel(tr["Xbar"][sample], r["Xbar"]) < 1e-9
    assert rel(tr["K"][sample], r["K"]) < 1e-9


def test_warm_start_round_trip():
    """Warm start from a previous solution (the MPC update's reuse of Xbar/Ubar/K)."""
    prob = syn.make_batch(4, 4, 20, "trot")
    s = hsddp.Solver(prob, hsddp.load_settings(no_early_exit=1, max_AL_iter=1, max_DDP_iter=2))
    s.solve()
    tr = s.trajectory()
    s.warm_start(tr["Xbar"], tr["Ubar"], tr["K"])
    s.solve()
    g = {**s.trajectory(), **s.element_info()}
    s.close()
    p2 = dict(prob); p2["Xbar"], p2["Ubar"], p2["K"] = tr["Xbar"], tr["Ubar"], tr["K"]
    r = O.solve_batch(p2, O.default_options(no_early_exit=1, max_AL_iter=1, max_DDP_iter=2))
    assert rel(g["Xbar"], r["Xbar"]) < 1e-9 and rel(g["K"], r["K"]) < 1e-9


def _stack(idx, P, N, gait):
    ps = [syn.make_batch(1, P, N, gait, first_element=i) for i in idx]
    q = dict(ps[0]); q["batch"] = len(idx)
    for k in ("contacts", "x0", "Xbar", "Ubar"):
        q[k] = np.concatenate([p[k] for p in ps])
    return q


def test_parallel_retry_equals_sequential(monkeypatch):
    """Regularisation retries (backward_sweep_regularized, MultiPhaseDDP.cpp:141-181) evaluated in
    parallel (k_riccati_retry / k_riccati_select) give the sequential loop's result bit for bit, on
    jump elements whose sweeps fail in inner iterations 9-12 (element 760 of the synthetic batch
    exhausts the schedule on the oracle).  These elements are chaotic by then (1e-9 differences of
    rounding at iteration 2 grow to O(1) by iteration 9, on the oracle against itself as on the
    GPU), so the oracle comparison of the retry path is test_retries_match_oracle's."""
    prob = _stack([377, 760, 656, 321, 0], 8, 25, "jump")
    kw = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=12)
    g = _run(prob, **kw)
    monkeypatch.setenv("HSDDP_SEQUENTIAL_RETRY", "1")
    q = _run(prob, **kw)
    for f in ("Xbar", "Ubar", "K", "X", "U", "dU", "dX", "cost", "feas", "iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], q[f]), f


def _weights(**kw):
    w = hsddp.Weights()
    hsddp._lib.lib().hsddp_default_weights(__import__("ctypes").byref(w))
    for k, v in kw.items():
        setattr(w, k, v)
    return w


@pytest.mark.parametrize("B,cap", [(5, None), (200, None), (7, "2")])
def test_retries_match_oracle(monkeypatch, B, cap):
    """A deterministic retry workload: r_qJd = -0.5 makes dt R_qJd = -5e-3, so every element's
    first sweep fails the PSD test and the schedule mu = 1e-3, 2e-3, 4e-3, 8e-3 ... runs until the
    joint-velocity diagonals turn positive (MultiPhaseDDP.cpp:141-181).  B = 200 defers more than
    the 128 elements one launch's parallel retry holds: the rest take the in-kernel sequential loop
    of the same launch (and HSDDP_RETRY_CAP=2 sends most of a small batch there).  Parallel,
    overflow and sequential paths give one result, equal to the oracle's."""
    if cap:
        monkeypatch.setenv("HSDDP_RETRY_CAP", cap)
    prob = syn.make_batch(B, 2, 10, "trot")
    kw = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=3)
    w = _weights(r_qJd=-0.5)

    def run():
        s = hsddp.Solver(prob, hsddp.load_settings(**kw), weights=w)
        s.solve()
        out = {**s.trajectory(), **s.working(), **s.element_info()}
        s.close()
        return out

    g = run()
    monkeypatch.setenv("HSDDP_SEQUENTIAL_RETRY", "1")
    q = run()
    for f in ("Xbar", "Ubar", "K", "dU", "cost", "status", "n_ls_trials"):
        assert np.array_equal(g[f], q[f]), f
    sample = list(range(0, B, max(1, B // 8)))
    r = O.solve_batch(prob, O.default_options(**kw), n_threads=8, elements=sample, weights={"r_qJd": -0.5})
    assert np.array_equal(g["status"][sample], r["status"]) and np.all(r["status"] == 0)
    assert np.array_equal(g["n_ls_trials"][sample], r["n_ls_trials"])
    for f in ("Xbar", "Ubar", "K", "dU"):
        assert rel(g[f][sample], r[f]) < 1e-9, f


def test_solver_info_history_matches_oracle():
    """get_solver_info (MultiPhaseDDP.cpp:532-541): the per-element buffers of a full solve with
    early exits — the initial entry and one per inner iteration that passes the later-termination
    test (:277-280, :358-371) — equal the oracle's entry for entry (float32 values)."""
    prob = syn.make_batch(6, 4, 20, "trot")
    s = hsddp.Solver(prob, hsddp.load_settings())
    s.solve()
    h = s.solver_info()
    info = s.element_info()
    s.close()
    r = O.solve_batch(prob, O.default_options(), n_threads=8)
    assert np.array_equal(info["iters"], r["iters"])
    for b in range(6):
        ref = r["solver_info"][b]
        assert len(h["cost"][b]) == len(ref) > 1, b
        got = np.stack([h[k][b] for k in ("cost", "dyn_feas", "eqn_feas", "ineq_feas")], 1)
        assert np.allclose(got, ref, rtol=1e-6, atol=1e-9), b


@pytest.mark.parametrize("gait,P,N", [("trot", 2, 8), ("jump", 8, 4)])
def test_trajectory_exports_match_numpy_restatement(gait, P, N):
    """The dense Trajectory fields a reference caller reads (TrajectoryManagement.h:49-81): the LQ
    model A, B, lx, lu, lxx, luu of the first LQ_approximation (SinglePhase.cpp:264-296), the
    terminal Phix, Phixx (+ AL) and reset-map Jacobian Px per phase, and the value function G[0],
    H[0] per phase of the first sweep (SinglePhase.cpp:365) — against the independent dense numpy
    restatement (tests/numpy_riccati.py) at the initial rollout.  l and Phi are those of the last
    compute_cost (the last line-search trial, SinglePhase.cpp:235-262): they sum to the accepted cost."""
    import numpy_riccati as NR
    B = 3
    prob = syn.make_batch(B, P, N, gait)
    s = hsddp.Solver(prob, hsddp.load_settings(no_early_exit=1, max_AL_iter=1, max_DDP_iter=1))
    s.set_value_export(True)
    s.solve()
    lq, tm, v, info = s.lq(), s.terminal(), s.value(), s.element_info()
    s.close()
    k0 = np.cumsum([0] + list(prob["horizons"]))
    for b in range(B):
        X, U, D = NR.initial_rollout(prob, b)
        ref = NR.sweep(prob, b, X, U, D)
        for i in range(P):
            ks, Phix, Phixx, Px = ref["lq"][i]
            for k in range(prob["horizons"][i]):
                kc = k0[i] + k
                for name, want in zip(("A", "B", "lx", "lu", "lxx", "luu"), ks[k]):
                    assert rel(lq[name][b, kc], want) < 1e-12, (b, kc, name)
            assert rel(tm["Phix"][b, i], Phix) < 1e-12, (b, i)
            assert rel(tm["Phixx"][b, i], Phixx) < 1e-12, (b, i)
            if Px is None:
                assert np.all(tm["Px"][b, i] == 0)
            else:
                assert rel(tm["Px"][b, i], Px) < 1e-12, (b, i)
        assert rel(v["G"][b], ref["G0"]) < 1e-9, b
        assert rel(v["H"][b], ref["H0"]) < 1e-9, b
        if info["n_ls_trials"][b] < 4:  # accepted: the last trial's slot costs are the element's cost
            total = lq["l"][b].sum() + tm["Phi"][b].sum()
            assert abs(total - info["cost"][b]) <= 1e-12 * abs(total), b


@pytest.mark.parametrize("gait,P,N", [("trot", 2, 8), ("jump", 8, 4)])
def test_trajectory_exports_at_nondefault_parameters(gait, P, N):
    """The same exports at solver_params.WEIGHTS / CPARAMS (grf_eps = 0.3) from warm-start controls
    with friction-pyramid rows on both sides of delta: the log branch of the barrier, non-zero z
    foot-placement terms, td_lambda != 0 and ground_height != 0 in the exported records."""
    import solver_params as SP
    from test_oracle_parameters import assert_both_branches, numpy_sweep, sweep_problem
    B = 3
    prob, cp = sweep_problem(gait, P, N, 0.01)
    assert_both_branches(prob, cp)
    s = hsddp.Solver(prob, hsddp.load_settings(no_early_exit=1, max_AL_iter=1, max_DDP_iter=1),
                     cparams=SP.hsddp_cparams(cp), weights=SP.hsddp_weights())
    s.set_value_export(True)
    s.solve()
    lq, tm, v, info = s.lq(), s.terminal(), s.value(), s.element_info()
    s.close()
    k0 = np.cumsum([0] + list(prob["horizons"]))
    for b in range(B):
        ref = numpy_sweep(prob, b, cp, SP.WEIGHTS)
        for i in range(P):
            ks, Phix, Phixx, Px = ref["lq"][i]
            for k in range(prob["horizons"][i]):
                kc = k0[i] + k
                for name, want in zip(("A", "B", "lx", "lu", "lxx", "luu"), ks[k]):
                    assert rel(lq[name][b, kc], want) < 1e-12, (b, kc, name)
            assert rel(tm["Phix"][b, i], Phix) < 1e-12, (b, i)
            assert rel(tm["Phixx"][b, i], Phixx) < 1e-12, (b, i)
            if Px is None:
                assert np.all(tm["Px"][b, i] == 0)
            else:
                assert rel(tm["Px"][b, i], Px) < 1e-12, (b, i)
        assert rel(v["G"][b], ref["G0"]) < 1e-9, b
        assert rel(v["H"][b], ref["H0"]) < 1e-9, b
        if info["n_ls_trials"][b] < 4:  # accepted: the last trial's slot costs are the element's cost
            total = lq["l"][b].sum() + tm["Phi"][b].sum()
            assert abs(total - info["cost"][b]) <= 1e-12 * abs(total), b


def test_failed_line_search_keeps_the_last_trial():
    """Quirk A2 (MultiPhaseDDP.cpp:345-353) on the device: gamma = 1e6 rejects every trial, so the
    nominal rows stay and the working rows are the last trial (eps = 0.001) — the buffer-flip
    bookkeeping of k_decide.  The second iteration's LQ linearises about that
    trial: its result equals the oracle's (test_oracle_pinning pins the oracle's A2)."""
    prob = syn.make_batch(4, 2, 8, "trot")
    g0 = _run(prob, no_early_exit=1, max_AL_iter=1, max_DDP_iter=0)
    g1 = _run(prob, no_early_exit=1, max_AL_iter=1, max_DDP_iter=1, gamma=1e6)
    assert np.all(g1["n_ls_trials"] == 4) and np.all(g1["status"] == 0)
    assert np.array_equal(g1["Xbar"], g0["Xbar"]) and np.array_equal(g1["Ubar"], g0["Ubar"])
    assert np.allclose(g1["X"], g1["Xbar"] + 1e-3 * g1["dX"], rtol=1e-14, atol=1e-14)
    for n in (1, 2):
        kw = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=n, gamma=1e6)
        g = _run(prob, **kw)
        r = O.solve_batch(prob, O.default_options(**kw), n_threads=8)
        for f in ("X", "U", "Xbar", "Ubar", "K", "dU"):
            assert rel(g[f], r[f]) < 1e-9, (n, f)
        assert np.array_equal(g["n_ls_trials"], r["n_ls_trials"])


@pytest.mark.parametrize("gait,P,N", [("trot", 4, 50), ("jump", 8, 25)])
def test_nonuniform_reb_schedule_matches_oracle(gait, P, N):
    """update_ReB = 7, update_relax = 0.1 (HSDDP_OPTION's defaults, not the shipped INFO file's 1 / 1):
    update_REB_params (ConstraintsBase.h:168-183) moves each GRF row's (delta, eps) after every
    outer iteration, so the per-knot parameter arrays are read and, after each outer update, k_lq
    recomputes the slot costs the last line search left (Params::lq_slots).  Three outer x three
    inner iterations against the oracle."""
    prob = syn.make_batch(8, P, N, gait)
    kw = dict(no_early_exit=1, max_AL_iter=3, max_DDP_iter=3, update_ReB=7.0, update_relax=0.1)
    g = _run(prob, **kw)
    r = O.solve_batch(prob, O.default_options(**kw), n_threads=8)
    p2 = dict(prob); p2["x0"] = prob["x0"] * (1 + 1e-15)
    r2 = O.solve_batch(p2, O.default_options(**kw), n_threads=8)
    for f in ("Xbar", "Ubar", "K", "dU"):
        assert rel(g[f], r[f]) < max(1e-9, 10 * rel(r2[f], r[f])), f
    for f in ("cost", "feas", "max_pconstr"):
        assert rel(g[f], r[f]) < max(1e-9, 10 * rel(r2[f], r[f])), f
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], r[f]), f
