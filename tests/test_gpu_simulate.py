"""hsddp_simulate_policy / hsddp_update_problem_simulated on the GPU against tests/sim_reference.py
(the header's pseudo-code on the oracle's primitives, pinned to the oracle's own rollout by
tests/test_simulate_host.py).

Tolerance, as test_gpu_single_shooting.py: relative error below max(1e-9, 10 x the helper's own
deviation under a 1e-15 relative perturbation of x_init); steps and status equal.  The policies
come from two fixed inner iterations (no_early_exit = 1, max_AL_iter = 1, max_DDP_iter = 2), so
the gains are not zero.
"""
import os
import sys

import numpy as np
import pytest

import hsddp
import sim_reference as R
from hsddp import synthetic as syn

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
from mpc_scenario import Scenario  # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(HERE, "golden")
FIXED = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=2)
TICK = dict(max_AL_iter=2, max_DDP_iter=1)
FIELDS = ("X", "U", "x_end", "cost", "min_grf", "max_td")


def rel(a, b):
    """max |a - b| / max |b| over the finite entries of b; infinite entries must be the same ones"""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin])
    if not fin.any():
        return 0.0
    return float(np.max(np.abs(a[fin] - b[fin])) / max(1e-300, np.max(np.abs(b[fin]))))


def perturbed(Xbar0, M, seed):
    """[B][M][24]: Xbar[b, 0] plus uniform noise of +-0.05 rad, +-0.02 m, +-0.2 on the rates and
    +-0.05 on the leg entries"""
    rng = np.random.default_rng(seed)
    B = Xbar0.shape[0]
    amp = np.concatenate([np.full(3, 0.05), np.full(3, 0.02), np.full(6, 0.2), np.full(12, 0.05)])
    return Xbar0[:, None, :] + rng.uniform(-1, 1, (B, M, 24)) * amp


def solved(prob, **kw):
    s = hsddp.Solver(prob, hsddp.load_settings(**FIXED), **kw)
    s.solve()
    tr = s.trajectory()
    assert np.any(tr["K"] != 0)
    return s, tr


def flat(out):
    """simulate_policy's dict with the summary's fields beside the arrays"""
    q = {k: out[k] for k in ("x_end", "X", "U") if k in out}
    for f in ("cost", "min_grf", "max_td", "steps", "status"):
        q[f] = out["summary"][f]
    return q


def check(g, ref, ref2, n, where, fields=FIELDS):
    want, env = R.prefix(ref, n), R.prefix(ref2, n)
    assert np.array_equal(g["steps"], want["steps"]), where
    assert np.array_equal(g["status"], want["status"]), where
    for f in fields:
        e, tol = rel(g[f], want[f]), max(1e-9, 10 * rel(env[f], want[f]))
        print(f"{where} n={n} {f}: rel {e:.3e} (bound {tol:.3e})")
        assert e < tol, (where, n, f, e, tol)


# ---- 1. shared layout: two waves per element, the second part-filled ----------------------------
@pytest.fixture(scope="module")
def shared_case():
    prob = syn.make_batch(3, 3, 4, "trot")
    s, tr = solved(prob)
    x = perturbed(tr["Xbar"][:, 0], 70, seed=21)
    ref = R.simulate(prob, tr, x, 12)
    ref2 = R.simulate(prob, tr, x * (1 + 1e-15), 12)
    assert np.all(ref["status"] == 0)
    yield s, x, ref, ref2
    s.close()


@pytest.mark.parametrize("n", [1, 4, 5, 12])
def test_shared_layout_matches_helper(shared_case, n):
    """n = 1 inside a phase, 4 exactly a phase end (x_end has passed the reset map), 5 one past it,
    12 the whole horizon (no reset after the last phase)."""
    s, x, ref, ref2 = shared_case
    g = flat(s.simulate_policy(x, n, trajectories=True))
    check(g, ref, ref2, n, "shared")
    # without trajectories the same end states and summaries
    q = flat(s.simulate_policy(x, n))
    for f in ("x_end", "cost", "min_grf", "max_td", "steps", "status"):
        assert np.array_equal(q[f], g[f]), f


def test_x_init_defaults_to_x0(shared_case):
    s, x, ref, ref2 = shared_case
    x0 = np.repeat(s.prob["x0"][:, None, :], 2, axis=1)
    a, b = flat(s.simulate_policy(None, 5, n_samples=2)), flat(s.simulate_policy(x0, 5))
    for f in ("x_end", "cost", "min_grf", "max_td", "steps", "status"):
        assert np.array_equal(a[f], b[f]), f
    with pytest.raises(hsddp.HSDDPError):
        s.simulate_policy(x[:2], 1)  # [2][70][24] for B = 3


# ---- 2. per-element layouts ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [3, 12])
def test_per_element_layouts_match_helper(n):
    prob = syn.make_layout_batch([("trot", 2, 6), ("jump", 4, 3), ("pronk", 3, 4), ("bound", 6, 2)])
    cj = prob["contacts"][1, :5]
    assert np.any(np.all(cj[:4] == 0, axis=1))  # the jump has a flight phase
    d = np.diff(cj, axis=0)
    assert np.any(d == 1) and np.any(d == -1)   # ... and both reset directions
    s, tr = solved(prob)
    x = perturbed(tr["Xbar"][:, 0], 5, seed=22)
    ref = R.simulate(prob, tr, x, n)
    ref2 = R.simulate(prob, tr, x * (1 + 1e-15), n)
    g = flat(s.simulate_policy(x, n, trajectories=True))
    s.close()
    check(g, ref, ref2, n, "layouts")


@pytest.mark.parametrize("n", [7, 24])
def test_odd_mask_layouts_match_helper(n):
    """crawl, amble, hop and gray on their own layouts: friction margins over one and three stance
    legs (min_grf), the gain rows of stance and swing legs side by side within a leg triple, reset
    maps where one leg lifts as another lands, and touchdown heights of a single leg and of three
    legs at once (max_td).  n = 7: one knot past crawl's first phase end; 24: the whole horizon."""
    prob = syn.make_layout_batch([("crawl", 4, 6), ("amble", 8, 3), ("hop", 8, 3), ("gray", 12, 2)])
    c = prob["contacts"]
    assert {int(r.sum()) for r in c[0, :5]} == {3} and {1, 3} <= {int(r.sum()) for r in c[3, :13]}
    d = np.diff(c[2, :9], axis=0)
    assert np.any((d == 1).sum(axis=1) == 1) and np.any((d == 1).sum(axis=1) == 3)  # hop's touchdowns
    s, tr = solved(prob)
    x = perturbed(tr["Xbar"][:, 0], 5, seed=26)
    ref = R.simulate(prob, tr, x, n)
    ref2 = R.simulate(prob, tr, x * (1 + 1e-15), n)
    assert np.all(ref["status"] == 0)
    g = flat(s.simulate_policy(x, n, trajectories=True))
    s.close()
    check(g, ref, ref2, n, "odd masks")


# ---- 3. fp32 handle: the downloaded (widened) gains ---------------------------------------------
def test_fp32_handle_matches_helper():
    prob = syn.make_batch(2, 3, 4, "trot")
    s, tr = solved(prob, riccati_fp32=True)
    assert np.array_equal(tr["K"], tr["K"].astype(np.float32))
    x = perturbed(tr["Xbar"][:, 0], 3, seed=23)
    ref = R.simulate(prob, tr, x, 12)
    ref2 = R.simulate(prob, tr, x * (1 + 1e-15), 12)
    g = flat(s.simulate_policy(x, 12, trajectories=True))
    s.close()
    check(g, ref, ref2, 12, "fp32")


# ---- 3b. a handle with its own weights and constraint parameters ---------------------------------
def test_nondefault_parameters_match_helper():
    """solver_params.WEIGHTS / CPARAMS: the running and terminal costs by these weights (z foot terms
    included), min_grf by mu = 0.4, max_td against ground = 0.02."""
    import solver_params as SP
    prob = syn.make_batch(3, 3, 4, "trot")
    s, tr = solved(prob, weights=SP.hsddp_weights(), cparams=SP.hsddp_cparams())
    x = perturbed(tr["Xbar"][:, 0], 5, seed=25)
    kw = dict(mu=SP.CPARAMS["mu_fric"], ground=SP.CPARAMS["ground_height"], weights=SP.WEIGHTS)
    ref = R.simulate(prob, tr, x, 12, **kw)
    ref2 = R.simulate(prob, tr, x * (1 + 1e-15), 12, **kw)
    assert np.all(ref["status"] == 0)
    for n in (4, 12):  # a phase end (the touchdown heights enter max_td), the whole horizon
        g = flat(s.simulate_policy(x, n, trajectories=True))
        check(g, ref, ref2, n, "parameters")
    s.close()


# ---- 4. divergence is an outcome, not a fault ---------------------------------------------------
def test_diverged_samples_stop_alone():
    """Sample 1 starts beyond the 1e6 bound and sample 2 carries a NaN: arithmetic only.  Both stop
    at knot 0 with their initial state; their neighbours in the wave are not disturbed."""
    prob = syn.make_batch(2, 3, 4, "trot")
    s, tr = solved(prob)
    x = perturbed(tr["Xbar"][:, 0], 4, seed=24)
    x[:, 1, 3] = 3e6
    x[:, 2, 7] = np.nan
    g = flat(s.simulate_policy(x, 12, trajectories=True))
    s.close()
    for m in (1, 2):
        assert np.all(g["status"][:, m] == 1) and np.all(g["steps"][:, m] == 0) and np.all(g["cost"][:, m] == 0)
        assert np.all(np.isinf(g["min_grf"][:, m])) and np.all(g["max_td"][:, m] == 0)
        assert np.array_equal(g["x_end"][:, m], x[:, m], equal_nan=True)
        assert np.array_equal(g["X"][:, m, 0], x[:, m], equal_nan=True)  # the break knot's own row
        assert np.all(g["X"][:, m, 1:] == 0) and np.all(g["U"][:, m, 1:] == 0)
    keep = [0, 3]
    ref = R.simulate(prob, tr, x[:, keep], 12)
    ref2 = R.simulate(prob, tr, x[:, keep] * (1 + 1e-15), 12)
    check({k: v[:, keep] for k, v in g.items()}, ref, ref2, 12, "neighbours")


# ---- 5. refusals leave the handle usable --------------------------------------------------------
def _table(names=("trot",)):
    tabs, dt = [], None
    for n in names:
        t, dt = hsddp.load_quad_reference(os.path.join(GOLD, f"ref_{n}.csv"))
        tabs.append(t)
    return tabs, dt


def _x0(B, seed=3):
    rng = np.random.default_rng(seed)
    x0 = np.zeros((B, 24))
    x0[:, 5] = 0.25
    x0[:, 12:] = np.float32([.2, -.14, 0, .2, .14, 0, -.2, -.14, 0, -.2, .14, 0])
    x0[:, :3] += rng.uniform(-.05, .05, (B, 3))
    x0[:, 6:12] += rng.uniform(-.2, .2, (B, 6))
    return x0


def test_simulate_refusals():
    B, P, N = 3, 3, 4
    sc = Scenario(["trot", "pace", "bound"], P, N)
    prob = syn.make_batch(B, P, N, "trot")
    inp = sc.inputs(prob["x0"])
    prob.update(inp)
    prob["Xbar"] = inp["ref_x"].copy()
    s = hsddp.Solver(prob, hsddp.load_settings(**FIXED))
    s.solve()
    for kw in (dict(n_steps=0), dict(n_steps=s.Kc + 1), dict(n_steps=1, n_samples=0)):
        with pytest.raises(hsddp.HSDDPError):
            s.simulate_policy(None, **kw)
    s.shift(sc.step(1))
    with pytest.raises(hsddp.HSDDPError):  # the shift awaits update_problem
        s.simulate_policy(None, 1)
    inp = sc.inputs(prob["x0"])
    s.update_problem(inp["contacts"], inp["x0"], inp["ref_x"], inp["ref_u"], inp["ref_foot"])
    assert np.all(s.simulate_policy(None, 2)["summary"]["steps"] == 2)
    s.solve()
    assert np.all(np.isfinite(s.trajectory()["Xbar"]))
    s.close()


def test_update_problem_simulated_refusals():
    (tab,), dt = _table()
    B = 2
    x0 = _x0(B)
    s = hsddp.Solver(hsddp.reference_problem(tab, dt, [0], x0), hsddp.load_settings(**TICK))
    s.solve()

    def refused(sample=0):
        with pytest.raises(hsddp.HSDDPError):
            s.update_problem_simulated(sample)

    s.advance(None, 1)
    refused()                      # no simulation held
    s.update_problem(None, x0)
    s.solve()
    s.simulate_policy(None, 1)
    s.solve()                      # a new policy: the simulation is stale
    s.advance(None, 1)
    refused()
    s.update_problem(None, x0)
    s.solve()
    s.simulate_policy(None, 2)
    s.advance(None, 1)             # one step advanced, two simulated
    refused()
    s.update_problem(None, x0)
    s.solve()
    out = s.simulate_policy(None, 1, n_samples=2)
    refused()                      # no step advanced yet
    s.advance(None, 1)
    refused(2)                     # sample = M
    refused(-1)
    s.update_problem_simulated(1)
    s.solve()
    assert np.all(np.isfinite(s.trajectory()["Xbar"])) and np.all(out["summary"]["status"] == 0)
    s.close()


# ---- 6. no side effects -------------------------------------------------------------------------
def _state(s, it, feet):
    st = {**s.trajectory(), **s.working(), **s.constraint_params(), **s.constraint_values(), **s.element_info()}
    cmd = s.extract_commands(1, 0.01 * it, 0.01, s.phase_info()["durations"], feet, 0.5)
    for f in cmd.dtype.names:  # field by field (the record has padding bytes nothing writes)
        st["cmd_" + f] = cmd[f]
    return st


def test_simulation_has_no_side_effects():
    (tab,), dt = _table()
    B = 3
    p = hsddp.reference_problem(tab, dt, [0], _x0(B))
    a, b = (hsddp.Solver(p, hsddp.load_settings(**TICK)) for _ in range(2))
    a.solve(); b.solve()
    feet = np.random.default_rng(6).standard_normal((B, 12)).astype(np.float32)
    for it in range(2):
        x = perturbed(a.trajectory()["Xbar"][:, 0], 3, seed=30 + it)
        out = a.simulate_policy(x, 3, trajectories=True)
        assert np.all(out["summary"]["steps"] == 3)
        xt = _x0(B, 100 + it)
        fa, fb = a.advance(xt, 1), b.advance(xt, 1)
        assert fa == fb
        a.solve(); b.solve()
        sa, sb = _state(a, it, feet), _state(b, it, feet)
        for f in sa:
            assert np.array_equal(sa[f], sb[f], equal_nan=True), (it, f)
    a.close(); b.close()


# ---- 7. the closed loop on the device equals the one through the host ---------------------------
def _closed_loop(p, B, ticks=6, n=2):
    a, b = (hsddp.Solver(p, hsddp.load_settings()) for _ in range(2))
    a.solve(); b.solve()
    for s in (a, b):
        s.set_options(hsddp.load_settings(**TICK))
    feet = np.random.default_rng(8).standard_normal((B, 12)).astype(np.float32)
    changes, differ = 0, 0
    for it in range(ticks):
        x = np.repeat(a.trajectory()["Xbar"][:, None, 0, :], 2, axis=1)
        x[:, 1] = perturbed(x[:, 1], 1, seed=40 + it)[:, 0]
        ra, rb = a.simulate_policy(x, n), b.simulate_policy(x, n)
        assert np.array_equal(ra["x_end"], rb["x_end"]) and np.all(ra["summary"]["status"] == 0)
        fa = a.advance(None, n)
        a.update_problem_simulated(1)
        fb = b.advance(np.ascontiguousarray(rb["x_end"][:, 1]), n)
        assert fa == fb
        changes += sum(fa)
        lay = a.element_layouts()["horizons"]
        differ += any(h != lay[0] for h in lay)
        a.solve(); b.solve()
        sa, sb = _state(a, it, feet), _state(b, it, feet)
        for f in sa:
            assert np.array_equal(sa[f], sb[f], equal_nan=True), (it, f)
    a.close(); b.close()
    return changes, differ


def test_closed_loop_equals_host_path():
    (tab,), dt = _table(("flytrot",))
    B = 3
    changes, _ = _closed_loop(hsddp.reference_problem(tab, dt, [6], _x0(B)), B)
    assert changes >= 1  # some tick crossed a contact change


def test_closed_loop_with_per_element_windows():
    """Windows into the trot and the flytrot file in one handle: the elements' contact-change
    flags differ, so the ticks run on per-element layouts."""
    (ta, tb), dt = _table(("trot", "flytrot"))
    B = 4
    starts = [0 if b % 2 == 0 else len(ta) + 2 for b in range(B)]
    p = hsddp.reference_problem(np.concatenate([ta, tb]), dt, starts, _x0(B))
    changes, differ = _closed_loop(p, B)
    assert changes >= 1 and differ >= 1
