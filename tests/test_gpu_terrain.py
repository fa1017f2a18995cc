"""Per-phase terrain (hsddp_set_terrain): each robot's friction coefficient and touchdown ground
height, phase by phase, against the unmodified oracle — which takes one (mu_fric, ground_height) per
problem, so it is run per robot, or per knot and phase end (oracle_lib.knot_eval).

Shapes (terrain_case.py): Kc = 40, the shared layout 4 x 10 with B = 5 and a mix of 4 x 10 and 8 x 5
layouts with B = 6, at solver_params.WEIGHTS / CPARAMS from warm-start controls with pyramid rows on
both sides of delta; fixed small iteration budgets; multiple and single shooting.
"""
import os
import sys

import numpy as np
import pytest

import hsddp
import oracle_lib as O
from hsddp import model
import solver_params as SP
import terrain_case as TC

pytestmark = pytest.mark.gpu

FIXED = {"no_early_exit": 1, "max_AL_iter": 3, "max_DDP_iter": 2, **SP.SCHEDULE}


def _compare_robots(g, r, r2, where):
    """test_gpu_parameters.compare's rule, and the stored constraint values at the parameters' 1e-9"""
    for f in TC.ARRAYS + TC.SCALARS:
        e, tol = TC.rel(g[f], r[f]), max(1e-9, 10 * TC.rel(r2[f], r[f]))
        print(f"{where} {f}: rel {e:.3e} (bound {tol:.3e})")
        assert e < tol, (where, f, e, tol)
    for f in TC.DECISIONS:
        assert np.array_equal(g[f], r[f]), (where, f, g[f], r[f])
    assert np.array_equal(g["p_td_mask"], r["td_mask"]), where
    for f in TC.PARAMS:
        e = TC.rel(g["p_" + f], r[f])
        print(f"{where} {f}: rel {e:.3e}")
        assert e < 1e-9, (where, f, e)
    for f in ("grf_g", "td_h"):
        e, tol = TC.rel(g["v_" + f], r[f]), max(1e-9, 10 * TC.rel(r2[f], r[f]))
        print(f"{where} {f}: rel {e:.3e} (bound {tol:.3e})")
        assert e < tol, (where, f, e, tol)


# ---- 1. per robot against the oracle ----------------------------------------------------------------
@pytest.mark.parametrize("ms", [1, 0])
@pytest.mark.parametrize("shape", list(TC.PROBLEMS))
def test_robot_terrain_matches_oracle_per_robot(shape, ms):
    """Robot b on (MU, GROUND)[b mod 5], uniform over its phases: everything the solve leaves equals
    the oracle's solve of that robot alone with cparams {mu_fric: mu_b, ground_height: ground_b}."""
    prob = TC.PROBLEMS[shape]()
    opts = {**FIXED, "MS": ms}
    mu, gr = TC.robot_terrain(prob)
    r = TC.oracle_robots(prob, opts, mu[:, 0], gr[:, 0])
    r2 = TC.oracle_robots(prob, opts, mu[:, 0], gr[:, 0], 1 + 1e-15)
    for f in TC.DECISIONS:
        assert np.array_equal(r[f], r2[f]), f  # (nothing to screen)
    s = TC.gpu_solver(prob, opts)
    s.set_terrain(mu, gr)
    t = s.terrain()
    for b, hz in enumerate(TC.phases_of(prob)):  # (rows past a robot's phases read back as the cparams pair)
        assert np.array_equal(t["mu"][b, :len(hz)], mu[b, :len(hz)]) and np.array_equal(t["ground"][b, :len(hz)], gr[b, :len(hz)])
        assert np.all(t["mu"][b, len(hz):] == SP.CPARAMS["mu_fric"]) and np.all(t["ground"][b, len(hz):] == SP.CPARAMS["ground_height"])
    s.solve()
    g = TC.mask_padding(prob, TC.downloads(s))
    s.close()
    _compare_robots(g, r, r2, f"{shape} MS={ms}")


# ---- 2. every consumer, per phase ------------------------------------------------------------------
def _knot_refs(prob, b, W1, W2, mu, gr, opts):
    """oracle_lib.knot_eval over robot b's knots and phase ends with (mu, gr)[i] of each phase i: the
    LQ pieces at the rows W1 the last LQ_approximation saw, the costs and constraint values at the
    rows W2 of the last compute_cost (the downloaded working rows)."""
    hz = TC.phases_of(prob)[b]
    rb = 0 if prob["ref_x"].shape[0] == 1 else b
    out = {"l": [], "lu": [], "luu": [], "Phi": [], "Phix": [], "Phixx": [], "grf_g": [], "td_h": []}
    s = kc = 0
    o = O.default_options(**opts)
    for i, n in enumerate(hz):
        c, cn = prob["contacts"][b, i], prob["contacts"][b, i + 1]
        cp = SP.oracle_cparams(mu_fric=float(mu[i]), ground_height=float(gr[i]))
        kw = dict(options=o, dt=prob["dt"], weights=SP.WEIGHTS, cparams=cp)
        for k in range(n):
            ref = (prob["ref_x"][rb, s + k], prob["ref_u"][rb, s + k], prob["ref_foot"][rb, s + k])
            e1 = O.knot_eval(c, cn, W1["X"][b, s + k], W1["U"][b, kc], *ref, **kw)
            e2 = O.knot_eval(c, cn, W2["X"][b, s + k], W2["U"][b, kc], *ref, **kw)
            out["lu"].append(e1["lu"]); out["luu"].append(e1["luu"]); out["l"].append(e2["l"])
            g = np.zeros(20)
            for leg in range(4):
                if c[leg]:
                    f = W2["U"][b, kc, 3 * leg:3 * leg + 3]
                    m = float(mu[i])
                    g[5 * leg:5 * leg + 5] = [f[2], -f[0] + m * f[2], f[0] + m * f[2], -f[1] + m * f[2], f[1] + m * f[2]]
            out["grf_g"].append(g)
            kc += 1
        end = (prob["ref_x"][rb, s + n], prob["ref_foot"][rb, s + n])
        z = np.zeros(24)
        e1 = O.knot_eval(c, cn, z, z, z, z, np.zeros(12), W1["X"][b, s + n], *end, **kw)
        e2 = O.knot_eval(c, cn, z, z, z, z, np.zeros(12), W2["X"][b, s + n], *end, **kw)
        out["Phix"].append(e1["Phix"]); out["Phixx"].append(e1["Phixx"]); out["Phi"].append(e2["Phi"])
        s += n + 1
    return {k: np.array(v) for k, v in out.items()}


def _stance_and_touchdown(prob, b):
    hz = TC.phases_of(prob)[b]
    st = [bool(prob["contacts"][b, i].any()) for i in range(len(hz))]
    td = [bool(((prob["contacts"][b, i] == 0) & (prob["contacts"][b, i + 1] == 1)).any()) for i in range(len(hz))]
    return hz, st, td


@pytest.mark.parametrize("shape", list(TC.PROBLEMS))
def test_every_consumer_reads_its_phase(shape):
    """A distinct (mu, ground) per (robot, phase).  Two inner iterations through the split solve: the
    downloaded LQ pieces (l, lu, luu), terminal pieces (Phi, Phix, Phixx) and stored constraint values
    equal the oracle's knot evaluation with that phase's values at 1e-12 (the LQ-export tests'
    tolerance) — and the same comparison with the handle-wide cparams misses it at every stance phase
    (mu) and every touchdown phase (ground), so no site can pass while ignoring the table."""
    prob = TC.PROBLEMS[shape]()
    opts = {"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 2}
    mu, gr = TC.phase_terrain(prob)
    s = TC.gpu_solver(prob, opts)
    s.set_terrain(mu, gr)
    s.begin()
    s.iterate(1)
    W1, info1 = s.working(), s.element_info()
    s.iterate(1)
    W2, lq, tm, val = s.working(), s.lq(), s.terminal(), s.constraint_values()
    s.close()
    assert np.all(info1["n_ls_trials"] >= 1) and not np.array_equal(W1["U"], prob["Ubar"])  # (a step was taken)
    wide = (np.full_like(mu, SP.CPARAMS["mu_fric"]), np.full_like(gr, SP.CPARAMS["ground_height"]))
    for b in range(prob["batch"]):
        hz, stance, touch = _stance_and_touchdown(prob, b)
        k0 = np.cumsum([0] + hz)
        ref = _knot_refs(prob, b, W1, W2, mu[b], gr[b], opts)
        off = _knot_refs(prob, b, W1, W2, wide[0][b], wide[1][b], opts)
        for i, n in enumerate(hz):
            ks = slice(k0[i], k0[i + 1])
            got = {"l": lq["l"][b, ks], "lu": lq["lu"][b, ks], "luu": lq["luu"][b, ks], "grf_g": val["grf_g"][b, ks]}
            for f, a in got.items():
                e = TC.rel(a, ref[f][ks]) if np.abs(ref[f][ks]).max() > 0 else float(np.abs(a).max())
                assert e < 1e-12, (b, i, f, e)
                if stance[i]:
                    assert TC.rel(a, off[f][ks]) > 1e-12, ("the handle-wide mu passes", b, i, f)
            tgot = {"Phi": tm["Phi"][b, i], "Phix": tm["Phix"][b, i], "Phixx": tm["Phixx"][b, i]}
            for f, a in tgot.items():
                assert TC.rel(a, ref[f][i]) < 1e-12, (b, i, f)
                if touch[i]:
                    assert TC.rel(a, off[f][i]) > 1e-12, ("the handle-wide ground passes", b, i, f)
            # the stored touchdown residuals: foot height at the working X_i[N] above the phase's ground
            if touch[i]:
                c, cn = prob["contacts"][b, i], prob["contacts"][b, i + 1]
                legs = np.flatnonzero((c == 0) & (cn == 1))
                h = val["td_h"][b, i, 0, legs]
                x_end = W2["X"][b, k0[i] + i + n]
                want = model.touchdown_constraint(x_end, c, cn, ground=float(gr[b, i]))[0][0, :len(legs)]
                wide_h = model.touchdown_constraint(x_end, c, cn, ground=SP.CPARAMS["ground_height"])[0][0, :len(legs)]
                assert np.all(np.abs(h - want) <= 1e-12), (b, i, h, want)
                assert np.all(np.abs(h - wide_h) > 1e-12), ("the handle-wide ground passes", b, i)


def test_reb_update_relaxes_the_rows_below_threshold_at_the_phase_mu():
    """k_reb_update: after each of two outer iterations (two solves of one, the parameters carried)
    the rows whose (delta, eps) moved are those whose stored g — compared above with the phase's mu
    — lies at or below -pconstr_thresh, and some rows do move."""
    prob = TC.mixed_problem()
    opts = {"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 1, **SP.SCHEDULE}
    mu, gr = TC.phase_terrain(prob)
    s = TC.gpu_solver(prob, opts)
    s.set_terrain(mu, gr)
    thr = s.options.pconstr_thresh
    eps = np.full((prob["batch"], prob["Kc"], 20), SP.CPARAMS["grf_eps"])
    moved = 0
    for _ in range(2):
        s.solve()
        g, p = s.constraint_values()["grf_g"], s.constraint_params()
        stance = np.repeat(_stance_rows(prob), 5, axis=2).reshape(g.shape)
        below = (g <= -thr) & stance
        assert np.array_equal(p["reb_eps"] != eps, below)
        moved += int(below.sum())
        eps = p["reb_eps"]
    s.close()
    assert moved > 0


def _stance_rows(prob):
    """[B][Kc][4]: leg l stands at knot kc"""
    out = np.zeros((prob["batch"], prob["Kc"], 4), bool)
    for b, hz in enumerate(TC.phases_of(prob)):
        kc = 0
        for i, n in enumerate(hz):
            out[b, kc:kc + n] = prob["contacts"][b, i] != 0
            kc += n
    return out


# ---- 3. a uniform table is the handle, bit for bit --------------------------------------------------
def _solve_all(prob, opts, cparams, fp32, table):
    s = TC.gpu_solver(prob, opts, cparams, fp32)
    if table is not None:
        s.set_terrain(*table)
    s.solve()
    out = TC.downloads(s)
    s.close()
    return out


@pytest.mark.parametrize("ms", [1, 0])
@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("shape", list(TC.PROBLEMS))
def test_uniform_table_equals_no_table_bit_for_bit(shape, fp32, ms):
    """3a: a table filled with the handle's own cparams values gives byte-identical downloads to the
    handle without a table.  3b: a handle whose cparams keep the library's mu_fric / ground_height
    with a table of CPARAMS' 0.4 / 0.02 against the handle created with them."""
    prob = TC.PROBLEMS[shape]()
    opts = {**FIXED, "MS": ms}
    B, P = prob["batch"], TC.stride_P(prob)
    v = (np.full((B, P), SP.CPARAMS["mu_fric"]), np.full((B, P), SP.CPARAMS["ground_height"]))
    plain = _solve_all(prob, opts, None, fp32, None)
    same = _solve_all(prob, opts, None, fp32, v)
    for f in plain:
        assert np.array_equal(plain[f], same[f]), ("3a", f)
    other = _solve_all(prob, opts, SP.oracle_cparams(mu_fric=0.7, ground_height=0.0), fp32, v)
    for f in plain:
        assert np.array_equal(plain[f], other[f]), ("3b", f)


def test_slot_costs_recomputed_after_set_terrain():
    """hsddp_set_terrain clears slots_fresh: the next k_lq forms the slot costs itself (its SLOTS
    instantiation, with the table) and the iteration equals the one whose rollout formed them."""
    prob = TC.mixed_problem()
    opts = {"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 1}
    mu, gr = TC.phase_terrain(prob)
    outs = []
    for again in (False, True):
        s = TC.gpu_solver(prob, opts)
        s.set_terrain(mu, gr)
        s.begin()
        if again:
            s.set_terrain(mu, gr)
        s.iterate(1)
        outs.append(TC.downloads(s))
        s.close()
    for f in outs[0]:
        assert np.array_equal(outs[0][f], outs[1][f]), f


# ---- 4. graph and freshness ----------------------------------------------------------------------
@pytest.mark.parametrize("graph", [True, False])
def test_terrain_between_solves_on_the_graph_path(monkeypatch, graph):
    """Early exits on (the replayed inner iteration): solve, set_terrain, solve — the second solve
    continues from the first one's state and equals the oracle doing the same per robot.  Then
    set_terrain(None, None): a twin handle that never had terrain takes every robot as it stands
    (hsddp_copy_elements), and the next solve of the two is equal bit for bit.  The same with
    HSDDP_NO_GRAPH=1."""
    if not graph:
        monkeypatch.setenv("HSDDP_NO_GRAPH", "1")
    prob = TC.shared_problem()
    B = prob["batch"]
    for k in ("ref_x", "ref_u", "ref_foot"):  # per-element references (the twin receives elements)
        prob[k] = np.ascontiguousarray(np.repeat(prob[k], B, axis=0))
    opts = {"max_AL_iter": 2, "max_DDP_iter": 3, **SP.SCHEDULE}
    mu, gr = TC.robot_terrain(prob)
    s, twin = TC.gpu_solver(prob, opts), TC.gpu_solver(prob, opts)
    s.solve()
    first = TC.downloads(s)
    s.set_terrain(mu, gr)
    s.solve()
    g = TC.downloads(s)
    # the oracle: the second solve from the first one's trajectories, parameters and stored values
    cont = dict(prob, Xbar=first["Xbar"], Ubar=first["Ubar"], K=first["K"])
    cons = {f: first["p_" + f] for f in O.CONSTRAINT_FIELDS}
    state = {"X": first["X"], "U": first["U"], "Defect": first["Defect"], "grf_g": first["v_grf_g"],
             "td_h": first["v_td_h"], "dX": first["dX"], "dU": first["dU"]}
    r, r2 = (_continue(cont, opts, mu[:, 0], gr[:, 0], cons, state, sc) for sc in (1.0, 1 + 1e-15))
    for f in TC.DECISIONS:
        assert np.array_equal(r[f], r2[f]), f  # (the oracle repeats its exits under the perturbation)
    _compare_robots(g, r, r2, f"second solve, graph={graph}")
    s.set_terrain(None, None)
    every = np.arange(B)
    twin.copy_elements(s, every, every)
    s.solve()
    twin.solve()
    a, b = TC.downloads(s), TC.downloads(twin)
    s.close()
    twin.close()
    for f in a:
        assert np.array_equal(a[f], b[f]), f


def _continue(prob, opts, mu, gr, cons, state, scale):
    out = {}
    B = prob["batch"]
    p = dict(prob)
    if scale != 1.0:
        p["x0"] = p["x0"] * scale
    for b in range(B):
        cp = SP.oracle_cparams(mu_fric=float(mu[b]), ground_height=float(gr[b]))
        r = O.solve_batch(p, O.default_options(**opts), elements=[b], weights=SP.WEIGHTS, cparams=cp,
                          constraints=cons, state=state)
        for k, v in r.items():
            if k != "solver_info":
                out.setdefault(k, []).append(np.asarray(v)[0])
    return {k: np.array(v) for k, v in out.items()}


# ---- ABI ------------------------------------------------------------------------------------------
def test_refused_terrain_leaves_the_handle_unchanged():
    prob = TC.mixed_problem()
    mu, gr = TC.phase_terrain(prob)
    s = TC.gpu_solver(prob, {"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 1})
    s.set_terrain(mu, gr)
    lens = [len(h) for h in TC.phases_of(prob)]
    for bad_mu, bad_gr in ((0.0, None), (-0.1, None), (np.nan, None), (np.inf, None), (None, np.nan)):
        m2, g2 = mu.copy(), gr.copy()
        if bad_mu is not None:
            m2[2, 1] = bad_mu
        if bad_gr is not None:
            g2[2, 1] = bad_gr
        with pytest.raises(hsddp.HSDDPError):
            s.set_terrain(m2, g2)
        t = s.terrain()
        for b, n in enumerate(lens):
            assert np.array_equal(t["mu"][b, :n], mu[b, :n]) and np.array_equal(t["ground"][b, :n], gr[b, :n])
    # rows past a robot's own phases are not read (robot 0: 4 of the stride's 8 phases) and read back as cparams
    m2 = mu.copy()
    m2[0, lens[0]:] = np.nan
    s.set_terrain(m2, None)
    t = s.terrain()
    assert np.all(t["mu"][0, lens[0]:] == SP.CPARAMS["mu_fric"]) and np.all(t["ground"] == SP.CPARAMS["ground_height"])
    s.set_terrain(None, None)
    t = s.terrain()
    assert np.all(t["mu"] == SP.CPARAMS["mu_fric"]) and np.all(t["ground"] == SP.CPARAMS["ground_height"])
    s.close()


# ---- 5. ticks ----------------------------------------------------------------------------------------
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
PLAN = 0.4  # Kc = 40 on the trot file
STARTS = [0, 4, 9, 15]  # within 16 ticks every robot drops a first phase and appends a last one, at its own ticks


def _tick_batch(copies, ms=1):
    import restart_case as RC
    tab, dt = hsddp.load_quad_reference(os.path.join(HERE, "golden", "ref_trot.csv"))
    out = []
    for _ in range(copies):
        p = hsddp.reference_problem(tab, dt, STARTS, RC.x0(len(STARTS), 40), plan_duration=PLAN)
        assert p["Kc"] == 40
        out.append(hsddp.Solver(p, hsddp.load_settings(**dict(RC.TICK, MS=ms))))
    return out


class _Rows:
    """the restatement: ref_oracle.ProblemTracker's phases with each robot's rows riding on them"""

    def __init__(self, rows, fill):
        import ref_oracle as R
        ref, dt = R.load_quad_reference(os.path.join(HERE, "golden", "ref_trot.csv"))
        self.R, self.ref, self.dt = R, ref, dt
        self.tk = [R.ProblemTracker(ref, w, dt, plan_duration=PLAN) for w in STARTS]
        self.rows, self.fill = [[list(q) for q in r[:len(t.horizons)]] for r, t in zip(rows, self.tk)], list(fill)
        self.events = [set() for _ in STARTS]

    def step(self):
        for b, t in enumerate(self.tk):
            n0, pop = len(t.horizons), t.horizons[0] <= 1
            t.step()
            app = len(t.horizons) - (n0 - pop)
            src = list(range(int(pop), n0)) + [-1] * app
            self.rows[b] = TC.move_rows(self.rows[b], src, self.fill)
            self.events[b] |= ({"pop"} if pop else set()) | ({"append"} if app else set())

    def restart(self, b, start):
        self.tk[b] = self.R.ProblemTracker(self.ref, start, self.dt, plan_duration=PLAN)
        self.rows[b] = [list(self.fill) for _ in self.tk[b].horizons]

    def arrays(self):
        P = max(len(r) for r in self.rows)
        a = np.array([r + [self.fill] * (P - len(r)) for r in self.rows])
        return np.ascontiguousarray(a[..., 0]), np.ascontiguousarray(a[..., 1])


@pytest.mark.parametrize("ms", [1, 0])
def test_terrain_rides_the_phases_through_ticks(ms):
    """Per-phase terrain set once on handle A; handle B is given the whole expected table (the
    restatement's) after every advance, while its inputs are pending.  hsddp_get_terrain of A shows
    the moved and inherited rows after every advance, and A and B are equal bit for bit every tick.
    Mid-way robot 2 of A and B restarts: cparams rows for it, and every bit of the other robots as in
    the twin C, which runs the same ticks without the restart."""
    import restart_case as RC
    A, Bh, Ct = _tick_batch(3, ms)
    lib_cp = hsddp.ConstraintParams()
    hsddp.lib().hsddp_default_constraint_params(__import__("ctypes").byref(lib_cp))
    fill = (lib_cp.mu_fric, lib_cp.ground_height)
    P0 = A.P
    q = np.arange(4 * P0).reshape(4, P0)
    mu0, gr0 = 0.3 + 0.6 * ((q * 7) % (4 * P0)) / (4 * P0), -0.03 + 0.06 * ((q * 5 + 3) % (4 * P0)) / (4 * P0)
    rows = _Rows(np.stack([mu0, gr0], -1), fill)
    mu0, gr0 = rows.arrays()  # (rows past a robot's phases: the cparams values, as they read back)
    for s in (A, Bh, Ct):
        s.set_terrain(mu0, gr0)
        s.solve()
    for it in range(16):
        x = RC.x0(4, 60 + it)
        rows.step()
        mu, gr = rows.arrays()
        for s in (A, Bh, Ct):
            s.advance(None, 1, PLAN)
        if it == 8:
            rows.restart(2, 30)
            mu, gr = rows.arrays()
            ws = np.array([0, 0, 30, 0], np.int32)
            for s in (A, Bh):
                s.restart_elements([0, 0, 1, 0], ws, None, PLAN)
        t = A.terrain()
        assert t["mu"].shape == mu.shape and np.array_equal(t["mu"], mu) and np.array_equal(t["ground"], gr), it
        Bh.set_terrain(mu, gr)
        for s in (A, Bh, Ct):
            s.update_problem(None, x)
            s.solve()
        a, b, c = RC.snapshot(A), RC.snapshot(Bh), RC.snapshot(Ct)
        assert [list(h) for h in a["horizons"]] == [t.horizons for t in rows.tk], it
        for e in range(4):
            RC.same_element(a, b, e)
        for e in (0, 1, 3):  # the restart of robot 2 left the others' bits alone
            RC.same_element(a, c, e)
        if it >= 8:
            assert RC.differences(a, c, 2), it
    assert all(ev == {"pop", "append"} for ev in rows.events), rows.events
    A.close(); Bh.close(); Ct.close()


def test_ticks_match_the_oracle_per_robot():
    """5a: robot b on (MU, GROUND)[b], uniform over its phases, set once before the first tick.  The
    initial solve with the shipped settings and sixteen ticks of hsddp_advance + re-solve (max_AL_iter
    = 2, max_DDP_iter = 1) — every robot drops a first phase and appends a last one, at its own ticks
    — equal, tick by tick and robot by robot, the oracle doing the same with cparams {mu_fric: mu_b,
    ground_height: ground_b} and the restated bookkeeping (mpc_oracle.shift / shift_constraints,
    ref_oracle.ProblemTracker and reference_slots), as test_gpu_reference.test_advance_loop_matches_oracle
    does for a handle-wide pair and with its tolerances.  A kernel that read another phase's row
    after an advance (a stale stride, a row not moved) would solve some robot on another robot's or
    the handle's values."""
    import mpc_oracle as M
    import ref_oracle as R
    import restart_case as RC
    path = os.path.join(HERE, "golden", "ref_trot.csv")
    tab, dt = hsddp.load_quad_reference(path)
    ref, _ = R.load_quad_reference(path)
    B = len(STARTS)
    mu, gr = np.array(TC.MU[:B]), np.array(TC.GROUND[:B])
    x0 = RC.x0(B, 40)
    p = hsddp.reference_problem(tab, dt, STARTS, x0, plan_duration=PLAN)
    assert p["Kc"] == 40 and p.get("layouts") is not None
    n_win = int(p["window_len"])
    dev = hsddp.Solver(p, hsddp.load_settings())
    dev.set_terrain(mu, gr)
    dev.solve()
    tks = [R.ProblemTracker(ref, w, dt, plan_duration=PLAN) for w in STARTS]
    cps = [{"mu_fric": float(mu[b]), "ground_height": float(gr[b])} for b in range(B)]

    def problem_of(tk, x, Xbar=None, Ubar=None, K=None):
        rx, ru, rf = R.reference_slots(ref, int(tk.start), n_win, dt, tk.horizons, 0.01, None)
        hz = list(tk.horizons)
        return {"batch": 1, "horizons": hz, "shooting": list(tk.shooting), "dt": p["dt"], "S": sum(n + 1 for n in hz),
                "Kc": sum(hz), "x0": np.ascontiguousarray(x[None]), "contacts": np.ascontiguousarray(tk.contact_rows()[None]),
                "ref_x": rx[None], "ref_u": ru[None], "ref_foot": rf[None],
                "Xbar": (rx if Xbar is None else Xbar)[None].copy(),
                "Ubar": (np.zeros((sum(hz), 24)) if Ubar is None else Ubar)[None].copy(), "K": None if K is None else K[None].copy()}

    def compare(r, where):
        g = {**dev.trajectory(), **dev.working(), **dev.element_info()}
        dc = dev.constraint_params()
        lay = dev.element_layouts()
        for b, tk in enumerate(tks):
            hz = list(tk.horizons)
            S, P = sum(n + 1 for n in hz), len(hz)
            assert [int(v) for v in lay["horizons"][b][:P]] == hz, (where, b)
            assert np.array_equal(dc["td_mask"][b, :P], r[b]["td_mask"][0]), (where, b)
            for f in ("al_sigma", "al_lambda"):
                assert np.max(np.abs(dc[f][b, :P] - r[b][f][0])) <= 1e-9 * max(1.0, np.max(np.abs(r[b][f]))), (where, b, f)
            for f in ("reb_delta", "reb_eps"):
                assert np.max(np.abs(dc[f][b] - r[b][f][0])) <= 1e-9 * max(1.0, np.max(np.abs(r[b][f]))), (where, b, f)
            for f in ("Xbar", "Ubar", "X", "K"):
                a = g[f][b, :S] if f in ("Xbar", "X") else g[f][b]
                e = np.max(np.abs(a - r[b][f][0])) / np.max(np.abs(r[b][f]))
                assert e <= 1e-8, (where, b, f, e)
            assert g["n_ls_trials"][b] == r[b]["n_ls_trials"][0], (where, b)

    r = [O.solve_batch(problem_of(tks[b], x0[b]), O.default_options(), cparams=cps[b]) for b in range(B)]
    compare(r, "initial")
    # the robots are on different ground: with the handle-wide pair robot 0's solve is another one
    r_wide = O.solve_batch(problem_of(tks[0], x0[0]), O.default_options())
    assert TC.rel(r_wide["Ubar"], r[0]["Ubar"]) > 1e-6
    kw = dict(max_AL_iter=2, max_DDP_iter=1)
    dev.set_options(hsddp.load_settings(**kw))
    op, _ = O.default_problem(p["horizons"], p["dt"])
    events = [set() for _ in tks]
    for it in range(16):
        x = RC.x0(B, 60 + it)
        dev.advance(x, 1, PLAN)
        for b, tk in enumerate(tks):
            hz0, ss0, re0 = list(tk.horizons), list(tk.shooting), list(tk.reach_end)
            flags = tk.update(1)
            events[b] |= ({"pop"} if hz0[0] <= 1 else set()) | ({"append"} if len(tk.horizons) > len(hz0) - (hz0[0] <= 1) else set())
            sh = M.shift(hz0, ss0, re0, r[b]["Xbar"][0], r[b]["X"][0], r[b]["Ubar"][0], r[b]["K"][0], flags)
            cons = M.resolve_td(M.shift_constraints(hz0, re0, {k: r[b][k][0] for k in O.CONSTRAINT_FIELDS}, flags,
                                                    op.grf_delta, op.grf_eps, op.td_sigma, op.td_lambda), tk.contact_rows())
            cons = {k: np.asarray(cons[k])[None] for k in O.CONSTRAINT_FIELDS}
            r[b] = O.solve_batch(problem_of(tk, x[b], sh[3], sh[4], sh[5]), O.default_options(**kw), constraints=cons,
                                 cparams=cps[b])
        dev.solve()
        compare(r, it)
    assert all(ev == {"pop", "append"} for ev in events), events
    dev.close()


# ---- 6. moves ----------------------------------------------------------------------------------------
def test_terrain_travels_with_moved_robots():
    """hsddp_copy_elements into a handle with terrain and into one without (which takes it up, cparams
    rows elsewhere), and hsddp_export_elements / hsddp_import_elements: the moved robot's rows arrive
    with it, its next ticks equal the ticks it runs in place bit for bit, and every other robot of
    the destination keeps every bit.  A record of the previous version is refused."""
    import restart_case as RC
    src, on, off, twin = _tick_batch(4)
    P0 = src.P
    q = np.arange(4 * P0).reshape(4, P0)
    mu0, gr0 = 0.3 + 0.6 * ((q * 7) % (4 * P0)) / (4 * P0), -0.03 + 0.06 * ((q * 5 + 3) % (4 * P0)) / (4 * P0)
    src.set_terrain(mu0, gr0)
    on.set_terrain(mu0[::-1].copy(), gr0[::-1].copy())
    for s in (src, on, off, twin):
        s.solve()
        for it in range(3):
            s.advance(RC.x0(4, 70 + it), 1, PLAN)
            s.solve()
    t_src, t_on = src.terrain(), on.terrain()
    s0, off0, on0 = RC.snapshot(src), RC.snapshot(off), RC.snapshot(on)
    n1, n3 = len(s0["horizons"][1]), len(s0["horizons"][3])
    on.copy_elements(src, [0], [1])
    off.copy_elements(src, [2], [3])
    rec = src.export_elements([1])
    imp = twin  # (a handle without terrain that receives the record)
    imp.import_elements([3], rec)
    old = rec.copy()
    old[0, :4] = np.frombuffer(np.uint32(0x48454c31).tobytes(), np.uint8)  # "HEL1"
    with pytest.raises(hsddp.HSDDPError, match="version"):
        imp.import_elements([0], old)
    # a record is outside input: its rows pass hsddp_set_terrain's checks (the header holds robot 1's
    # first friction coefficient once; a copy with it negated, and one with it NaN, are refused)
    head = rec[0, :4096].tobytes()
    at = head.find(np.float64(t_src["mu"][1, 0]).tobytes())
    assert at >= 0 and head.find(np.float64(t_src["mu"][1, 0]).tobytes(), at + 1) < 0
    for v in (-t_src["mu"][1, 0], np.nan):
        bad = rec.copy()
        bad[0, at:at + 8] = np.frombuffer(np.float64(v).tobytes(), np.uint8)
        before = RC.snapshot(imp), imp.terrain()
        with pytest.raises(hsddp.HSDDPError, match="terrain"):
            imp.import_elements([0], bad)
        after = RC.snapshot(imp), imp.terrain()
        for e in range(4):
            RC.same_element(after[0], before[0], e)
        assert np.array_equal(after[1]["mu"], before[1]["mu"])
    cp = hsddp.ConstraintParams()
    hsddp.lib().hsddp_default_constraint_params(__import__("ctypes").byref(cp))
    # the rows: the moved robot's own, the others' kept (on) or the cparams pair (off, imp)
    t = on.terrain()
    assert np.array_equal(t["mu"][0, :n1], t_src["mu"][1, :n1]) and np.array_equal(t["ground"][0, :n1], t_src["ground"][1, :n1])
    for e in (1, 2, 3):
        n = len(on0["horizons"][e])
        assert np.array_equal(t["mu"][e, :n], t_on["mu"][e, :n]) and np.array_equal(t["ground"][e, :n], t_on["ground"][e, :n])
    t = off.terrain()
    assert np.array_equal(t["mu"][2, :n3], t_src["mu"][3, :n3]) and np.array_equal(t["ground"][2, :n3], t_src["ground"][3, :n3])
    assert np.all(t["mu"][[0, 1, 3]] == cp.mu_fric) and np.all(t["ground"][[0, 1, 3]] == cp.ground_height)
    t = imp.terrain()
    assert np.array_equal(t["mu"][3, :n1], t_src["mu"][1, :n1]) and np.all(t["mu"][:3] == cp.mu_fric)
    RC.same_element(RC.snapshot(on), s0, 0, 1)
    RC.same_element(RC.snapshot(off), s0, 2, 3)
    for e in (0, 1, 3):
        RC.same_element(RC.snapshot(off), off0, e)
    # the ticks that follow: each robot given the same x0 wherever it lives
    for it in range(3):
        xs = RC.x0(4, 90 + it)
        xo, xf, xi = RC.x0(4, 100 + it), RC.x0(4, 110 + it), RC.x0(4, 110 + it)
        xo[0], xf[2], xi[3] = xs[1], xs[3], xs[1]
        for s, x in ((src, xs), (on, xo), (off, xf), (imp, xi)):
            s.advance(x, 1, PLAN)
            s.solve()
        a = RC.snapshot(src)
        RC.same_element(RC.snapshot(on), a, 0, 1)
        RC.same_element(RC.snapshot(off), a, 2, 3)
        RC.same_element(RC.snapshot(imp), a, 3, 1)
        f, i = RC.snapshot(off), RC.snapshot(imp)
        for e in (0, 1):  # robots 0 and 1 of off and imp never had terrain and got the same x0
            RC.same_element(f, i, e)
    for s in (src, on, off, twin):
        s.close()


# ---- 7. simulation -------------------------------------------------------------------------------------
def test_simulation_margins_follow_the_phase():
    """hsddp_simulate_policy with per-phase terrain: from the X, U rows it returns, min_grf is the
    minimum of the GRF rows with the knot's phase's mu over the simulated stance knots and max_td the
    largest |foot height - the phase's ground| at the phase ends reached — exactly.  M = 70 (a second
    chunk of 6 live lanes), 21 knots (past two phase ends of every layout)."""
    prob = TC.mixed_problem()
    B, M, n = prob["batch"], 70, 21
    mu, gr = TC.phase_terrain(prob)
    s = TC.gpu_solver(prob, {"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 2})
    s.set_terrain(mu, gr)
    s.solve()
    tr = s.trajectory()
    rng = np.random.default_rng(7)
    x = tr["Xbar"][:, None, 0, :] + 1e-3 * rng.standard_normal((B, M, 24))
    out = s.simulate_policy(x, n, trajectories=True)
    s.close()
    sm = out["summary"]
    assert np.all(sm["status"] == 0) and np.all(sm["steps"] == n)
    wide_differs = False
    for b, hz in enumerate(TC.phases_of(prob)):
        want_g = {True: np.full(M, np.inf), False: np.full(M, np.inf)}
        want_h = {True: np.zeros(M), False: np.zeros(M)}
        kc = 0
        for i, N in enumerate(hz):
            c, cn = prob["contacts"][b, i], prob["contacts"][b, i + 1]
            ks = [k for k in range(kc, kc + N) if k < n]
            kc += N
            if not ks:
                break
            for table in (True, False):
                m_i = float(mu[b, i]) if table else SP.CPARAMS["mu_fric"]
                g_i = float(gr[b, i]) if table else SP.CPARAMS["ground_height"]
                if c.any():
                    g = model.grf_constraint(out["U"][b][:, ks].reshape(-1, 24), c, mu=m_i)[0][:, :5 * int(c.sum())]
                    want_g[table] = np.minimum(want_g[table], g.reshape(M, -1).min(axis=1))
                ntd = int(((c == 0) & (cn == 1)).sum())
                if ks[-1] == kc - 1 and ntd:  # the phase end was reached: X_i[N] = the step from its last knot
                    xe = model.dynamics(out["X"][b][:, ks[-1]], out["U"][b][:, ks[-1]], np.tile(c.astype(float), (M, 1)), prob["dt"])
                    h = model.touchdown_constraint(xe, c, cn, ground=g_i)[0][:, :ntd]
                    want_h[table] = np.maximum(want_h[table], np.abs(h).max(axis=1))
        print(f"robot {b}: min_grf max diff {np.max(np.abs(sm['min_grf'][b] - want_g[True])):.3e}, "
              f"max_td max diff {np.max(np.abs(sm['max_td'][b] - want_h[True])):.3e}")
        assert np.array_equal(sm["min_grf"][b], want_g[True]), b
        assert np.array_equal(sm["max_td"][b], want_h[True]), b
        wide_differs = wide_differs or (not np.array_equal(want_g[True], want_g[False]) and
                                        not np.array_equal(want_h[True], want_h[False]))
    assert wide_differs


# ---- 8. facade -------------------------------------------------------------------------------------------
def test_facade_solves_with_per_phase_terrain():
    """tests/drivers/terrain_facade device: MultiPhaseDDP::solve of a problem whose phases differ in mu
    and ground equals, byte for byte over three ticks, the C ABI with describe()'s arrays and
    hsddp_set_terrain — and differs from the same calls without hsddp_set_terrain."""
    import subprocess
    drivers = os.path.join(HERE, "drivers")
    r = subprocess.run(["make", "-C", drivers, "-f", "terrain.mk", "terrain_facade"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(drivers, "terrain_facade"), "device"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "terrain_facade device ok" in r.stdout, r.stdout + r.stderr
