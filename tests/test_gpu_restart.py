"""GPU checks of hsddp_restart_elements (HKDProblem::initialization for a subset of a live batch):

T1  a restarted element equals, bit for bit, the same element of a twin handle on which it was a
    new problem at that window from the start, and every other element equals, bit for bit, the
    same handle run without the restart call — trajectory, working rows, search direction, element
    info, solver-info history, constraint parameters and stored values, layouts, phase info and
    references (tests/restart_case.py: snapshot / same_element).
T5  the refusals leave the handle as it was.

Batches: tests/restart_case.py (B = 6, Kc = 20 on the trot and flytrot files).  Every case runs three
MPC ticks (hsddp_advance + solve with max_AL_iter = 2, max_DDP_iter = 1), then the tick with the
restart: advance -> restart -> x0 -> solve ("tick"), or the restart with its x0 and a solve
("direct").  The cases: the restart keeps the batch's largest phase count ("base"), raises it
("up") or lowers it ("down") — the per-phase and per-slot strides change and the other elements'
rows move; B = 5 with the restarted element one half of a sweep pair whose partner is kept
("pair"); B = 1 ("single": shared references); every element, onto their own layouts ("all") and
onto one layout ("all_one": the handle returns to the shared layout); no element ("none").
"""
import os
import sys

import numpy as np
import pytest

import hsddp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import restart_case as RC  # noqa: E402

pytestmark = pytest.mark.gpu

T = 130  # samples of the trot file: flytrot's sample k is table sample T + k
# name -> (initial window starts, {restarted element: its new window start})
CASES = {
    "base": ([0, 3, T + 0, T + 6, 12, T + 12], {1: 21, 4: T + 27}),
    "up": ([0, 2, T + 6, T + 21, 31, T + 31], {1: 20, 4: T + 14}),
    "down": ([0, 17, T + 6, T + 21, T + 12, T + 31], {1: 1, 4: T + 22}),
    "pair": ([3, 3, T + 6, 12, T + 12], {1: 21}),
    "single": ([3], {0: 21}),
    "all": ([0, 3, T + 0, T + 6, 12, T + 12], {0: 40, 1: 21, 2: T + 3, 3: T + 27, 4: 5, 5: T + 40}),
    "all_one": ([0, 3, T + 0, T + 6, 12, T + 12], {b: 21 for b in range(6)}),
    "none": ([0, 3, T + 0, T + 6, 12, T + 12], {}),
}


def _trials(alpha):
    n, eps = 0, 1.0
    while eps > 1e-3:
        n, eps = n + 1, eps * alpha
    return n


def _translate_warm_start(s, elems, by=2e6):
    """the warm start of `elems` moved along x beyond the rollout's 1e6 bound (every state slot's
    body position; uploaded as a new warm start, for every element alike): the initial rollout of
    the next solve breaks at these elements' first knot, and so does every line-search trial"""
    tr = s.trajectory()
    for b in elems:
        tr["Xbar"][b, :, 3] += by
    s.warm_start(tr["Xbar"], tr["Ubar"], tr["K"])


def _run(case, how="tick", fp32=False, ms=1, diverged=False):
    starts, restart = CASES[case]
    tab, dt, n_trot = RC.table()
    assert n_trot == T
    B = len(starts)
    opts = dict(RC.TICK, MS=ms)
    A, C = (RC.solver(tab, dt, starts, RC.x0(B), fp32, **opts) for _ in range(2))
    for s in (A, C):
        s.solve()
    for it in range(3):
        x = RC.x0(B, 100 + it)
        for s in (A, C):
            s.advance(None, 1, RC.PLAN)
            s.update_problem(None, x)
            if diverged and it == 2:
                _translate_warm_start(s, restart)
            s.solve()
    if diverged:  # the solve before the restart broke for the restarted elements: the sweep on the broken
        # rollout's model failed (status), or every trial of every line search was rejected
        e = A.element_info()
        for b in restart:
            assert e["status"][b] != 0 or e["n_ls_trials"][b] == e["iters"][b] * _trials(A.options.alpha), \
                (b, e["status"], e["iters"], e["n_ls_trials"])
    mask = np.zeros(B, np.int32)
    ws = np.full(B, -12345, np.int32)  # entries outside the mask are not read
    x = RC.x0(B, 200)
    xr = np.full((B, 24), np.nan)
    for b, w in restart.items():
        mask[b], ws[b], xr[b] = 1, w, x[b]
    if how == "tick":
        for s in (A, C):
            s.advance(None, 1, RC.PLAN)
        A.restart_elements(mask, ws, None, RC.PLAN)
        for s in (A, C):
            s.update_problem(None, x)
    else:
        A.restart_elements(mask, ws, xr, RC.PLAN)
    for s in (A, C):
        s.solve()
    a, c = RC.snapshot(A), RC.snapshot(C)
    # (every element is compared before anything is asserted: one run shows all that differs)
    bad = {("kept", b): RC.differences(a, c, b, shared_refs=B == 1) for b in range(B) if b not in restart}
    if restart:
        st = [restart.get(b, starts[b]) for b in range(B)]
        xt = RC.x0(B, 7)
        for b in restart:
            xt[b] = x[b]
        Tw = RC.solver(tab, dt, st, xt, fp32, **opts)
        Tw.solve()
        t = RC.snapshot(Tw)
        for b in restart:
            bad["restarted", b] = RC.differences(a, t, b, shared_refs=B == 1)
            assert a["reach_end"][b] == [0] * len(a["horizons"][b])
        Tw.close()
    A.close(); C.close()
    assert not any(bad.values()), {k: v for k, v in bad.items() if v}
    return a, c


@pytest.mark.parametrize("case", list(CASES))
def test_restart_equals_new_problem_and_leaves_the_rest(case):
    a, c = _run(case)
    P0, P1 = c["_P"], a["_P"]
    if case == "base":  # the restarted elements' layouts differ from every neighbour's
        assert P0 == P1 == 3
        for b in (1, 4):
            assert all(a["horizons"][b] != a["horizons"][o] for o in range(6) if o != b)
    if case == "up":
        assert (P0, P1) == (2, 3)
    if case == "down":
        assert (P0, P1) == (3, 2)
    if case == "all_one":
        assert all(h == a["horizons"][0] for h in a["horizons"])


@pytest.mark.parametrize("case", ["base", "up", "pair", "single", "all", "none"])
def test_restart_with_x0_then_solve(case):
    """the restart takes the restarted elements' x0 itself; no advance before it"""
    _run(case, how="direct")


@pytest.mark.parametrize("case", ["base", "down", "pair", "single", "all", "none"])
def test_restart_fp32(case):
    _run(case, fp32=True)


@pytest.mark.parametrize("case", ["base", "up", "pair", "single", "all", "none"])
def test_restart_single_shooting(case):
    _run(case, ms=0)


@pytest.mark.parametrize("case,how", [("base", "tick"), ("up", "tick"), ("pair", "direct"), ("single", "tick"),
                                      ("all", "tick"), ("none", "tick")])
def test_restart_after_a_diverged_tick(case, how):
    """the solve before the restart broke the rollout's bound for the restarted elements, from the
    initial rollout on: their stored constraint values (cf_u, TD_STALE) and working rows are those
    of a broken solve"""
    _run(case, how=how, diverged=case != "none")


# ---- T5: arguments ------------------------------------------------------------------------------
def _refused(s, code, *args):
    rc = hsddp.lib().hsddp_restart_elements(s._h, *args)
    assert rc == code, (rc, hsddp.lib().hsddp_last_error())


def test_restart_refusals_leave_the_handle_unchanged():
    from hsddp._lib import ip
    import re
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "hsddp.h")).read()
    E = {k: int(v) for k, v in re.findall(r"\b(HSDDP_ERR_[A-Z]+)\s*=\s*(-?\d+)", hdr)}
    tab, dt, _ = RC.table()
    starts = CASES["base"][0]
    B = len(starts)
    A, C = (RC.solver(tab, dt, starts, RC.x0(B), **RC.TICK) for _ in range(2))
    one = np.array([0, 1, 0, 0, 0, 0], np.int32)
    ws = np.array(starts, np.int32) + 9
    for bad in (len(tab), len(tab) + 40, -1):  # a window start beyond (or before) the table
        w = ws.copy(); w[1] = bad
        _refused(A, E["HSDDP_ERR_ARG"], ip(one), ip(w), 0.2, 0.01, None)
    _refused(A, E["HSDDP_ERR_ARG"], None, ip(ws), 0.2, 0.01, None)   # NULL mask
    _refused(A, E["HSDDP_ERR_ARG"], ip(one), None, 0.2, 0.01, None)  # NULL window starts
    _refused(A, E["HSDDP_ERR_ARG"], ip(one), ip(ws), 0.6, 0.01, None)  # a plan that is not the handle's Kc
    for s in (A, C):
        s.solve()
    a, c = RC.snapshot(A), RC.snapshot(C)
    for b in range(B):
        RC.same_element(a, c, b)
    A.close(); C.close()
    # shared references: a partial mask, or window starts that differ
    S = RC.solver(tab, dt, [3], RC.x0(4), **RC.TICK)
    S2 = RC.solver(tab, dt, [3], RC.x0(4), **RC.TICK)
    part, every = np.array([0, 1, 0, 0], np.int32), np.ones(4, np.int32)
    _refused(S, E["HSDDP_ERR_UNSUPPORTED"], ip(part), ip(np.full(4, 21, np.int32)), 0.2, 0.01, None)
    _refused(S, E["HSDDP_ERR_UNSUPPORTED"], ip(every), ip(np.array([21, 21, 22, 21], np.int32)), 0.2, 0.01, None)
    for s in (S, S2):
        s.solve()
    a, c = RC.snapshot(S), RC.snapshot(S2)
    for b in range(4):
        RC.same_element(a, c, b, shared_refs=True)
    # ... and every element at one window start is a restart of the whole batch
    S.restart_elements(every, np.full(4, 21), RC.x0(4, 5), RC.PLAN)
    S.solve()
    W = RC.solver(tab, dt, [21], RC.x0(4, 5), **RC.TICK)
    W.solve()
    a, w = RC.snapshot(S), RC.snapshot(W)
    for b in range(4):
        RC.same_element(a, w, b, shared_refs=True)
    S.close(); S2.close(); W.close()
    # references uploaded from the host, not built from a table
    from hsddp import synthetic as syn
    H = hsddp.Solver(syn.make_batch(4, 2, 10, "trot"), hsddp.load_settings(**RC.TICK))
    _refused(H, E["HSDDP_ERR_UNSUPPORTED"], ip(every), ip(np.zeros(4, np.int32)), 0.2, 0.01, None)
    H.solve()
    H.close()


# ---- T2: the restarted elements against the oracle ------------------------------------------------
DT = float(np.float32(0.01))  # HKDProblem's float dt_sim widened to double (hsddp.reference_problem)


def _oracle_element(ref, dt, tk, x0_b, r_prev, lay_prev, flags, O, M, R):
    """One solve of the oracle for one element (B = 1): a new problem at the tracker's window
    (r_prev None), or the tick after r_prev — warm start, working rows and constraint objects
    shifted by the step flags (mpc_oracle), as tests/divergence_case.mpc_loop_oracle carries them."""
    hz = list(tk.horizons)
    rx, ru, rf = (a[None] for a in R.reference_slots(ref, tk.start, RC.N_WIN, dt, hz, 0.01))
    rows = tk.contact_rows()[None]
    p = {"batch": 1, "horizons": hz, "shooting": list(tk.shooting), "dt": DT, "S": sum(n + 1 for n in hz),
         "Kc": sum(hz), "x0": x0_b[None], "contacts": rows, "ref_x": rx, "ref_u": ru, "ref_foot": rf}
    opts = O.default_options(**RC.TICK)
    if r_prev is None:
        p.update(Xbar=rx.copy(), Ubar=np.zeros((1, p["Kc"], 24)))
        return O.solve_batch(p, opts)
    hz0, ss0, re0 = lay_prev
    op, _ = O.default_problem(hz0, DT)
    sh = M.shift(hz0, ss0, re0, r_prev["Xbar"][0], r_prev["X"][0], r_prev["Ubar"][0], r_prev["K"][0], flags)
    wk = M.shift_working(hz0, re0, r_prev["X"][0], r_prev["U"][0], r_prev["Defect"][0], flags)
    cons = M.shift_constraints(hz0, re0, {k: r_prev[k][0] for k in O.CONSTRAINT_FIELDS + ("grf_g", "td_h")}, flags,
                               op.grf_delta, op.grf_eps, op.td_sigma, op.td_lambda)
    cons = M.resolve_td(cons, rows[0])
    assert list(sh[0]) == hz and list(sh[1]) == list(tk.shooting)
    p.update(Xbar=sh[3][None], Ubar=sh[4][None], K=sh[5][None])
    state = {"X": wk[0][None], "U": wk[1][None], "Defect": wk[2][None], "grf_g": cons["grf_g"][None],
             "td_h": cons["td_h"][None]}
    return O.solve_batch(p, opts, constraints={k: cons[k][None] for k in O.CONSTRAINT_FIELDS}, state=state)


@pytest.mark.parametrize("case", ["base", "up", "pair", "single", "all"])
def test_restarted_elements_match_the_oracle(case):
    """After the restart the restarted elements run three more ticks; the restart's solve and every
    tick equal an oracle run started at that window (ProblemTracker + mpc_oracle), by
    tests/test_gpu_mpc.py::test_mpc_loop_matches_oracle's rule: Xbar, Ubar, X, K within 1e-8 and the
    cost and the ReB / AL parameters within 1e-9 of the largest entry (its _rel), td_mask and
    n_ls_trials exactly.  The layouts after each tick equal the tracker's."""
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
    import mpc_oracle as M
    import oracle_lib as O
    import ref_oracle as R
    from test_gpu_mpc import _rel
    starts, restart = CASES[case]
    tab, dt, _ = RC.table()
    ref = R.load_quad_reference(os.path.join(RC.GOLD, "ref_trot.csv"))[0] + \
        R.load_quad_reference(os.path.join(RC.GOLD, "ref_flytrot.csv"))[0]
    B = len(starts)
    A = RC.solver(tab, dt, starts, RC.x0(B), **RC.TICK)
    A.solve()
    for it in range(3):
        A.advance(RC.x0(B, 100 + it), 1, RC.PLAN)
        A.solve()
    mask, ws = np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b, w in restart.items():
        mask[b], ws[b] = 1, w
    x = RC.x0(B, 200)
    A.advance(None, 1, RC.PLAN)
    A.restart_elements(mask, ws, None, RC.PLAN)
    A.update_problem(None, x)
    A.solve()
    tks = {b: R.ProblemTracker(ref, w, dt, plan_duration=RC.PLAN) for b, w in restart.items()}
    rs = {b: _oracle_element(ref, dt, tks[b], x[b], None, None, None, O, M, R) for b in restart}

    def check(where):
        g = RC.snapshot(A)
        for b in restart:
            r, tk = rs[b], tks[b]
            assert list(g["horizons"][b]) == tk.horizons and list(g["shooting"][b]) == tk.shooting, (where, b)
            assert list(g["reach_end"][b]) == tk.reach_end, (where, b)
            P, S = len(tk.horizons), sum(n + 1 for n in tk.horizons)
            assert np.array_equal(g["contacts"][b][:P + 1], tk.contact_rows()), (where, b)
            assert np.array_equal(g["durations"][b][:P], np.array(tk.durations)), (where, b)
            assert np.array_equal(g["td_mask"][b][:P], r["td_mask"][0]), (where, b)
            for f in ("al_sigma", "al_lambda"):
                assert _rel(g[f][b][:P], r[f][0]) < 1e-9, (where, b, f)
            for f in ("reb_delta", "reb_eps"):
                assert _rel(g[f][b], r[f][0]) < 1e-9, (where, b, f)
            for f in ("Xbar", "X"):
                assert _rel(g[f][b][:S], r[f][0]) < 1e-8, (where, b, f)
            for f in ("Ubar", "K"):
                assert _rel(g[f][b], r[f][0]) < 1e-8, (where, b, f)
            assert g["n_ls_trials"][b] == r["n_ls_trials"][0], (where, b)
            assert _rel(g["cost"][b], r["cost"][0]) < 1e-9, (where, b)

    check("restart")
    for it in range(3):
        xt = RC.x0(B, 300 + it)
        A.advance(xt, 1, RC.PLAN)
        A.solve()
        for b in restart:
            tk = tks[b]
            lay = (list(tk.horizons), list(tk.shooting), list(tk.reach_end))
            flags = tk.update(1)
            rs[b] = _oracle_element(ref, dt, tk, xt[b], rs[b], lay, flags, O, M, R)
        check(it)
    A.close()
