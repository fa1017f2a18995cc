"""hsddp_upload_constraint_params: the state a handle carries between C-ABI calls.

The caller sees a touchdown constraint as its leg mask (td_legs, 4 bits); the device keeps two more
bits of its own in td_mask — TD_PENDING (legs decided by the next contact rows) and TD_STALE (the
stored residual was never computed since the constraint was registered: it reads 0, as a new
TConstrData's h, not the phase end's term_h, which holds whatever an earlier solve left).  A caller
that keeps its constraint objects itself (the C++ facade's MultiPhaseDDP::solve: upload_problem,
warm start, upload_constraint_params, solve) downloads and uploads leg masks only, so the upload
must not lose what the device knows about slots whose legs it does not change:

  * a download followed by an upload of the same arrays changes nothing — on a reused handle whose
    new problem's initial rollout breaks (the phases past the break never compute a residual and
    term_h still holds the previous problem's), inside the MPC loop (constraints the shift
    appended), with per-element layouts and in the fp32 mode;
  * the facade's call order with host copies of a new problem's values solves that new problem;
  * uploaded ReB / AL parameters are the ones the solve reads, against the oracle started from them;
  * the uniform-ReB shortcut (every knot still at the initial pair: the kernels read two scalars)
    survives partial uploads only while it is true;
  * a slot whose legs change is a new constraint: its residual reads 0 until a rollout reaches it.
"""
import functools
import os
import sys

import numpy as np
import pytest

import divergence_case as DC
import hsddp
import oracle_lib as O
from hsddp import synthetic as syn
from test_gpu_divergence import MPC_T3, _close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import mpc_oracle as M  # noqa: E402

pytestmark = pytest.mark.gpu

PARAMS = ("reb_delta", "reb_eps", "td_mask", "al_sigma", "al_lambda")


def _all(s):
    return {**s.trajectory(), **s.working(), **s.element_info(), **s.constraint_params(), **s.constraint_values()}


def _same(g, c, where=""):
    assert set(g) == set(c)
    for f in g:
        assert np.array_equal(g[f], c[f]), (where, f)


def _rel(a, b):
    return float(np.max(np.abs(a - b)) / max(1e-300, np.max(np.abs(b))))


def _new_problem(s, prob):
    """a new problem on a live handle, as Solver.__init__ uploads it"""
    s.upload_problem(prob["contacts"], prob["x0"], prob["ref_x"], prob["ref_u"], prob["ref_foot"])
    s.warm_start(prob.get("Xbar"), prob.get("Ubar"), prob.get("K"))


# ---- a new problem on a reused handle whose initial rollout breaks --------------------------------
INIT_CASE = ("trot", 4, 12, 8)
INIT_KW = [dict(no_early_exit=1, max_AL_iter=2, max_DDP_iter=3), {}]


@functools.lru_cache(maxsize=None)
def _init_case():
    prob, breaks, T, es = DC.make_init(*INIT_CASE)
    gait, P, N, B = INIT_CASE
    # the same batch untranslated (per-element references, as the handle's): no rollout breaks
    clean = DC._translated(syn.make_batch(B, P, N, gait), np.zeros(B), es)
    return prob, breaks, T, es, clean


@functools.lru_cache(maxsize=None)
def _init_oracle(ikw):
    prob = _init_case()[0]
    kw = INIT_KW[ikw]
    r = O.solve_batch(prob, O.default_options(**kw), n_threads=8)
    p2 = dict(prob); p2["x0"] = prob["x0"] * (1 + 1e-15)
    return r, O.solve_batch(p2, O.default_options(**kw), n_threads=8)


def _dirty_handle(kw):
    """a handle that has solved the untranslated batch: every phase end's residual computed and
    stored (term_h), no constraint stale.  Returns (solver, td_h after that solve)."""
    clean = _init_case()[4]
    s = hsddp.Solver(clean, hsddp.load_settings(**kw))
    s.solve()
    return s, s.constraint_values()["td_h"]


def _check_init_against_oracle(g, ikw):
    """tests/test_gpu_divergence.py::test_new_problem_initial_rollout_diverges' checks"""
    prob, breaks, T, es, _ = _init_case()
    r, r2 = _init_oracle(ikw)
    for b, j in enumerate(breaks):
        assert r["diverged_init"][b] == (j >= 0), b
    assert any(r["diverged_init"])
    most = max(len(DC.stale_knots(prob, r["U"], r["grf_g"], b)) for b in range(8))
    assert most > 8, most
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], r[f]), f
    for f in ("Xbar", "X"):
        err, tol = _close(DC.untranslate(g[f], T, es), DC.untranslate(r[f], T, es), DC.untranslate(r2[f], T, es))
        assert err <= tol, (f, err, tol)
    for f in ("Ubar", "U", "K", "dU", "cost", "feas", "merit", "max_tconstr", "max_pconstr",
              "reb_delta", "reb_eps", "al_sigma", "al_lambda", "grf_g", "td_h"):
        err, tol = _close(g[f], r[f], r2[f])
        assert err <= tol, (f, err, tol)
    for b in range(8):
        assert DC.stale_knots(prob, g["U"], g["grf_g"], b) == DC.stale_knots(prob, r["U"], r["grf_g"], b), b


def _assert_dirty_past_the_breaks(td_h):
    """some touchdown residual the dirtying solve stored belongs to a phase at or after a break
    phase of the new problem — a phase whose residual the new problem never computes"""
    breaks = _init_case()[1]
    N = INIT_CASE[2]
    assert any(j >= 0 and td_h[b, j // N:].any() for b, j in enumerate(breaks)), breaks


@pytest.mark.parametrize("ikw", [0, 1])
def test_round_trip_is_a_noop_on_a_reused_handle(ikw):
    kw = INIT_KW[ikw]
    prob = _init_case()[0]
    out = []
    for round_trip in (False, True):
        s, dirty = _dirty_handle(kw)
        _assert_dirty_past_the_breaks(dirty)
        _new_problem(s, prob)
        if round_trip:
            s.upload_constraint_params(**s.constraint_params())
        s.solve()
        out.append(_all(s))
        s.close()
    _same(out[1], out[0])
    _check_init_against_oracle(out[1], ikw)


def test_facade_call_order_on_a_reused_handle():
    """MultiPhaseDDP::solve of the C++ facade: upload_problem, warm start (Xbar, Ubar, K), the five
    parameter arrays from the caller's own (new) constraint objects, solve."""
    ikw = 0
    prob, _, _, _, _ = _init_case()
    fresh = hsddp.Solver(prob, hsddp.load_settings(**INIT_KW[ikw]))
    own = fresh.constraint_params()  # a new problem's values, held by the caller
    fresh.close()
    s, dirty = _dirty_handle(INIT_KW[ikw])
    _assert_dirty_past_the_breaks(dirty)
    s.upload_problem(prob["contacts"], prob["x0"], prob["ref_x"], prob["ref_u"], prob["ref_foot"])
    s.warm_start(prob["Xbar"], prob["Ubar"], np.zeros((prob["batch"], prob["Kc"], 24, 24)))
    s.upload_constraint_params(**own)
    s.solve()
    g = _all(s)
    s.close()
    _check_init_against_oracle(g, ikw)


# ---- inside the MPC loop ---------------------------------------------------------------------
@pytest.mark.parametrize("ms", [1, 0])
def test_round_trip_inside_the_mpc_loop(ms):
    """tests/test_gpu_divergence.py::test_mpc_tick_initial_rollout_diverges' loop with a download /
    upload of the constraint parameters between update_problem and solve of every tick.  (In this
    loop the only element whose rollout breaks, pronk element 3, has no touchdown legs in the slots
    the shift appends, and every other element's rollout recomputes its residuals before they are
    read — so an upload that dropped TD_STALE passed here too.  What the loop pins is that the
    merge leaves shifted, appended and resolved slots, and everything solved from them, as the
    oracle has them at every tick.)"""
    B, P, N, ticks = 8, 4, 5, 8
    T = np.zeros(B); T[3], first = MPC_T3[ms]
    prob, r0, out = DC.mpc_loop_oracle(B, P, N, T, ticks, ms=ms)
    _, r0p, outp = DC.mpc_loop_oracle(B, P, N, T, ticks, ms=ms, perturb=1e-15)
    div = [t["r"]["diverged_init"][3] for t in out]
    assert r0["diverged_init"][3] == 0 and not any(div[:first]) and all(div[first:]), div
    s = hsddp.Solver(prob, hsddp.load_settings(MS=ms))
    s.solve()
    g = {**s.trajectory(), **s.element_info()}
    for f in ("n_ls_trials", "status"):
        assert np.array_equal(g[f], r0[f]), f
    s.set_options(hsddp.load_settings(max_AL_iter=2, max_DDP_iter=1, MS=ms))
    appended_while_broken = 0
    for it, (t, tp) in enumerate(zip(out, outp)):
        last_before = (s.constraint_params()["td_mask"][:, -1] != 0).sum(axis=1)
        lay = s.shift(t["flags"])
        inp = t["inp"]
        s.update_problem(inp["contacts"], inp["x0"], inp["ref_x"], inp["ref_u"], inp["ref_foot"])
        cp = s.constraint_params()
        # the step pushed a knot onto the last phase (no new phase) and registered one more
        # touchdown constraint on it (k_shift_params): that phase's count grows
        grew = bool(lay["reach_end"][-1]) and np.any((cp["td_mask"][:, -1] != 0).sum(axis=1) > last_before)
        appended_while_broken += bool(grew and div[it])
        s.upload_constraint_params(**cp)
        s.solve()
        g = _all(s)
        r, r2 = t["r"], tp["r"]
        hz = t["prob"]["horizons"]
        es = np.stack([DC.direction_of(inp["contacts"][b], hz) for b in range(B)])
        for f in ("iters", "status", "n_ls_trials"):
            assert np.array_equal(g[f], r[f]), (it, f)
        assert np.array_equal(g["td_mask"], r["td_mask"]), it
        for f in ("Xbar", "X"):
            err, tol = _close(DC.untranslate(g[f], T, es), DC.untranslate(r[f], T, es), DC.untranslate(r2[f], T, es))
            assert err <= tol, (it, f, err, tol)
        for f in ("Ubar", "U", "K", "cost", "feas", "merit", "max_tconstr", "max_pconstr",
                  "reb_delta", "reb_eps", "al_sigma", "al_lambda", "grf_g", "td_h"):
            err, tol = _close(g[f], r[f], r2[f])
            assert err <= tol, (it, f, err, tol)
        assert DC.stale_knots(t["prob"], g["U"], g["grf_g"], 3) == DC.stale_knots(t["prob"], r["U"], r["grf_g"], 3), it
    s.close()
    assert appended_while_broken >= 1


# ---- the uploaded parameters are the ones solved with -----------------------------------------
@pytest.mark.parametrize("gait,P,N", [("trot", 2, 10), ("jump", 8, 4)])
def test_uploaded_parameters_are_solved_with(gait, P, N):
    B = 5
    prob = syn.make_batch(B, P, N, gait)
    kw = dict(max_AL_iter=2, max_DDP_iter=3)
    s = hsddp.Solver(prob, hsddp.load_settings(**kw))
    cp = s.constraint_params()
    rng = np.random.default_rng(P * 100 + N)
    up = {"reb_delta": cp["reb_delta"] * rng.uniform(0.5, 2.0, cp["reb_delta"].shape),
          "reb_eps": cp["reb_eps"] * rng.uniform(0.5, 2.0, cp["reb_eps"].shape),
          "al_sigma": cp["al_sigma"] * rng.uniform(0.5, 2.0, cp["al_sigma"].shape),
          "al_lambda": rng.uniform(-2.0, 2.0, cp["al_lambda"].shape), "td_mask": cp["td_mask"]}
    s.upload_constraint_params(**up)
    back = s.constraint_params()
    for f in PARAMS:
        assert np.array_equal(back[f], up[f]), f
    s.solve()
    g = _all(s)
    s.close()
    r = O.solve_batch(prob, O.default_options(**kw), n_threads=B, constraints=up)
    plain = O.solve_batch(prob, O.default_options(**kw), n_threads=B)
    assert _rel(plain["Xbar"], r["Xbar"]) > 1e-6  # the parameters matter to this solve
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], r[f]), f
    assert np.array_equal(g["td_mask"], r["td_mask"])
    for f in ("Xbar", "X", "Ubar", "U", "K", "cost", "reb_delta", "reb_eps", "al_sigma", "al_lambda"):
        assert _rel(g[f], r[f]) < 1e-9, (f, _rel(g[f], r[f]))


# ---- the uniform-ReB shortcut under partial uploads -------------------------------------------
def test_partial_reb_uploads_keep_the_shortcut_honest():
    """With the shipped schedule (update_ReB = update_relax = 1) the kernels read the two initial
    scalars instead of the per-knot arrays while every knot still holds the initial pair.  A partial
    upload that equals the initial value says nothing about the other field on the device."""
    B = 5
    prob = syn.make_batch(B, 2, 10, "trot")
    opt = lambda: hsddp.load_settings(max_AL_iter=2, max_DDP_iter=3)  # noqa: E731

    def run(*uploads):
        s = hsddp.Solver(prob, opt())
        for u in uploads:
            s.upload_constraint_params(**u)
        s.solve()
        out = _all(s)
        s.close()
        return out

    s = hsddp.Solver(prob, opt())
    init = s.constraint_params()
    s.close()
    rng = np.random.default_rng(17)
    eps = init["reb_eps"] * rng.uniform(0.5, 2.0, init["reb_eps"].shape)
    delta = init["reb_delta"] * rng.uniform(0.5, 2.0, init["reb_delta"].shape)
    d0, e0 = init["reb_delta"], init["reb_eps"]
    assert len(np.unique(d0)) == 1 and len(np.unique(e0)) == 1
    fresh = run()
    # (a) non-uniform eps, then delta alone at its initial value: the eps must still be read
    full = run(dict(reb_delta=d0, reb_eps=eps))
    assert not np.array_equal(full["Xbar"], fresh["Xbar"])
    _same(run(dict(reb_eps=eps), dict(reb_delta=d0)), full, "a")
    # (b) then both at their initial values: a fresh new problem
    _same(run(dict(reb_eps=eps), dict(reb_delta=d0), dict(reb_delta=d0, reb_eps=e0)), fresh, "b")
    # (c) eps alone at its initial value onto a non-uniform delta
    full = run(dict(reb_delta=delta, reb_eps=e0))
    assert not np.array_equal(full["Xbar"], fresh["Xbar"])
    _same(run(dict(reb_delta=delta), dict(reb_eps=e0)), full, "c")


# ---- changed legs ---------------------------------------------------------------------------------
def test_a_slot_with_new_legs_is_a_new_constraint():
    B, P, N = 5, 4, 6
    prob = syn.make_batch(B, P, N, "trot")
    kw = dict(no_early_exit=1, max_AL_iter=2, max_DDP_iter=2)
    s = hsddp.Solver(prob, hsddp.load_settings(**kw))
    s.solve()
    b, i = 2, 1
    legs = M.td_bits(prob["contacts"][b][i], prob["contacts"][b][i + 1])
    cp, before = s.constraint_params(), s.constraint_values()["td_h"]
    assert legs and cp["td_mask"][b, i, 0] == legs and cp["td_mask"][b, i, 1] == 0
    assert before[b, i, 0].any()  # the phase end's residual is stored and is not zero
    mask = cp["td_mask"].copy()
    mask[b, i, 1] = legs
    s.upload_constraint_params(td_mask=mask)
    assert np.array_equal(s.constraint_params()["td_mask"], mask)
    after = s.constraint_values()["td_h"]
    assert not after[b, i, 1].any()  # no rollout has reached the new constraint
    after[b, i, 1] = before[b, i, 1]
    assert np.array_equal(after, before)  # every other constraint keeps its residual
    # the same mask on a new problem (every residual zero), against the oracle started from it
    _new_problem(s, prob)
    cp = s.constraint_params()
    mask = cp["td_mask"].copy()
    mask[b, i, 1] = legs
    s.upload_constraint_params(td_mask=mask)
    assert not s.constraint_values()["td_h"].any()
    s.solve()
    g = _all(s)
    s.close()
    cons = dict(cp, td_mask=mask)
    r = O.solve_batch(prob, O.default_options(**kw), n_threads=B, constraints=cons)
    plain = O.solve_batch(prob, O.default_options(**kw), n_threads=B)
    assert _rel(plain["Xbar"][b], r["Xbar"][b]) > 1e-9  # the second constraint's AL terms are in the solve
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], r[f]), f
    assert np.array_equal(g["td_mask"], r["td_mask"])
    for f in ("Xbar", "X", "Ubar", "U", "K", "cost", "al_sigma", "al_lambda", "td_h"):
        assert _rel(g[f], r[f]) < 1e-9, (f, _rel(g[f], r[f]))


# ---- per-element layouts, fp32 ------------------------------------------------------------------
def _mixed7():
    """tests/test_gpu_layouts.py's mixed handle, B = 7: trot-like gaits on 4 x 10 beside jumps on 8 x 5"""
    names = ["trot", "jump", "pace", "jump", "bound", "pronk", "jump"]
    return syn.make_layout_batch([(g, 8, 5) if g == "jump" else (g, 4, 10) for g in names])


@pytest.mark.parametrize("which", ["layouts", "fp32"])
def test_round_trip_is_a_noop_with_layouts_and_fp32(which):
    prob = _mixed7() if which == "layouts" else syn.make_batch(6, 4, 10, "trot", mixed=True)
    out = []
    for round_trip in (False, True):
        s = hsddp.Solver(prob, hsddp.load_settings(no_early_exit=1, max_AL_iter=2, max_DDP_iter=2),
                         riccati_fp32=(which == "fp32"))
        s.solve()  # a used handle: stored residuals, no stale constraint
        _new_problem(s, prob)
        if round_trip:
            s.upload_constraint_params(**s.constraint_params())
        s.solve()
        out.append(_all(s))
        s.close()
    _same(out[1], out[0], which)
