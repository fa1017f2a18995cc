"""Per-phase cost weights (hsddp_set_phase_weights): a row of HKD weights for single phases of single
robots, against the unmodified oracle (which takes one set per problem: rows that differ only in
fields their phase's contact multiplies by zero), against the oracle's knot evaluation with each
phase's row and a dense numpy sweep over those terms, and bit for bit against the per-robot table and
the plain handle.

Shapes (terrain_case.py): Kc = 40, the shared layout 4 x 10 with B = 5 and a mix of 4 x 10 and 8 x 5
layouts with B = 6, at solver_params.WEIGHTS / CPARAMS from warm-start controls with pyramid rows on
both sides of delta; fixed small iteration budgets; multiple and single shooting.
"""
import os
import sys

import numpy as np
import pytest

import hsddp
import element_weights_case as EW
import phase_weights_case as PW
import solver_params as SP
import terrain_case as TC
import tiled_case as TT
from test_gpu_terrain import FIXED, _compare_robots

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))


def _same(a, b, where):
    for f in a:
        assert np.array_equal(a[f], b[f]), (where, f)


# ---- 1. fields the contact masks out, full solve against the oracle ---------------------------------
@pytest.mark.parametrize("ms", [1, 0])
def test_masked_fields_match_the_oracle_per_robot(ms):
    """A pronk (phases alternate 1111 / 0000), robot b on weight set b: its stance phases carry the
    set with other q_qJ and qf_scale[12..23], its flight phases the set with other foot weights —
    fields those phases multiply by zero.  Everything the solve leaves equals the oracle's solve of
    that robot alone with the set, by test_gpu_terrain._compare_robots' rule; a site that read the
    other phase's row would pick up a replaced value where it is not masked.  Control: with the
    replacements swapped between stance and flight rows the solve is another one."""
    prob = PW.pronk_problem()
    opts = {**FIXED, "MS": ms}
    sets = EW.robot_sets(prob["batch"])
    r = EW.oracle_robots(prob, opts, sets)
    r2 = EW.oracle_robots(prob, opts, sets, 1 + 1e-15)
    for f in TC.DECISIONS:
        assert np.array_equal(r[f], r2[f]), f  # (nothing to screen)
    outs = {}
    for swap in (False, True):
        s = EW.gpu_solver(prob, opts)
        rows = PW.table(prob, PW.masked_rows(prob, sets, swap))
        s.set_phase_weights(rows)
        back, flags = s.phase_weights()
        assert np.array_equal(back, rows) and np.all(flags == 1)
        s.solve()
        outs[swap] = TC.mask_padding(prob, TC.downloads(s))
        s.close()
    _compare_robots(outs[False], r, r2, f"pronk MS={ms}")
    e = TC.rel(outs[True]["K"], r["K"])
    print(f"control (swapped rows) K: rel {e:.3e}")
    assert e > 1e-6, e


# ---- 2. every consumer reads its phase ---------------------------------------------------------------
@pytest.mark.parametrize("shape", list(TC.PROBLEMS))
def test_every_consumer_reads_its_phase(shape):
    """A distinct row for every (robot, phase), each field within 30 % of SP.WEIGHTS.  Two inner
    iterations through the split solve: the LQ terms of the second (A, B, lx, lu, lxx, luu, Phix,
    Phixx) equal the oracle's knot evaluation with the phase's row at 1e-12; the value function at
    each phase start, the gains, the feed-forward and the linear rollout's dX equal a dense numpy
    sweep over the oracle's terms at 1e-9 (test_gpu_parity's tolerances for these quantities); and the
    accepted cost equals the sum of the oracle's knot and terminal costs at the working rows, at
    test_new_rows_on_a_warm_handle_against_oracle_knot_costs' 1e-12.  With the robot's first phase's
    row on every phase the LQ terms miss."""
    prob = TC.PROBLEMS[shape]()
    opts = {"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 2}
    rows = PW.phase_rows(prob)
    s = EW.gpu_solver(prob, opts)
    s.set_value_export(True)
    s.set_phase_weights(PW.table(prob, rows), PW.own_mask(prob))
    s.begin()
    s.iterate(1)
    W1, info1 = s.working(), s.element_info()
    s.iterate(1)
    W2, lq, tm, val, tr, info2 = s.working(), s.lq(), s.terminal(), s.value(), s.trajectory(), s.element_info()
    s.close()
    assert np.all(info1["n_ls_trials"] >= 1) and not np.array_equal(W1["U"], prob["Ubar"])  # (a step was taken)
    costs_checked = 0
    for b in range(prob["batch"]):
        hz = TC.phases_of(prob)[b]
        S, Kc, P = sum(n + 1 for n in hz), sum(hz), len(hz)
        T1 = PW.knot_terms(prob, b, W1, rows[b], opts)
        for f in ("A", "B", "lx", "lu", "lxx", "luu"):
            e = TC.rel(lq[f][b, :Kc], T1[f])
            print(f"{shape} robot {b} {f}: rel {e:.3e}")
            assert e < 1e-12, (b, f, e)
        for f in ("Phix", "Phixx"):
            e = TC.rel(tm[f][b, :P], T1[f])
            print(f"{shape} robot {b} {f}: rel {e:.3e}")
            assert e < 1e-12, (b, f, e)
        wrong = PW.knot_terms(prob, b, W1, [rows[b][0]] * P, opts)
        assert TC.rel(lq["lxx"][b, :Kc], wrong["lxx"]) > 1e-6 and TC.rel(tm["Phixx"][b, :P], wrong["Phixx"]) > 1e-6, b
        ref = PW.dense_sweep(hz, T1, W1["Defect"][b])
        got = {"G": val["G"][b, :P], "H": val["H"][b, :P], "K": tr["K"][b], "dU": W2["dU"][b], "dX": W2["dX"][b, :S]}
        for f, a in got.items():
            e = TC.rel(a, ref[f])
            print(f"{shape} robot {b} {f}: rel {e:.3e}")
            assert e < 1e-9, (b, f, e)
        if info2["n_ls_trials"][b] < 4:  # accepted: the last trial's slot costs are the robot's cost
            T2 = PW.knot_terms(prob, b, W2, rows[b], opts)
            total = T2["l"].sum() + T2["Phi"].sum()
            e = abs(info2["cost"][b] - total) / abs(total)
            print(f"{shape} robot {b} cost: rel {e:.3e}")
            assert e < 1e-12, (b, e)
            costs_checked += 1
    assert costs_checked >= 1, "no robot accepted a step: the cost comparison checked nothing"


# ---- 3. bit-for-bit equalities -----------------------------------------------------------------------
def _solve(prob, opts, fp32, how):
    s = EW.gpu_solver(prob, opts, None, fp32)
    sets = EW.robot_sets(prob["batch"])
    per_phase = [[sets[b]] * len(hz) for b, hz in enumerate(TC.phases_of(prob))]
    if how in ("robot", "robot_and_equal"):
        s.set_element_weights(EW.rows(sets))
    if how == "equal":  # (a) on a handle without a per-robot table: the handle's weights as every override
        s.set_phase_weights(PW.table(prob, [[SP.WEIGHTS] * len(hz) for hz in TC.phases_of(prob)]))
    if how in ("robot_and_equal", "phase"):  # (a) over the per-robot rows; (b) in their place
        s.set_phase_weights(PW.table(prob, per_phase))
    if how == "on_off":  # (c)
        s.set_phase_weights(PW.table(prob, PW.phase_rows(prob)), PW.own_mask(prob))
        s.set_phase_weights(None)
        back, flags = s.phase_weights()
        assert not flags.any() and np.array_equal(back, np.tile(PW.vec(SP.WEIGHTS), back.shape[:2] + (1,)))
    s.solve()
    out = TC.downloads(s)
    s.close()
    return out


@pytest.mark.parametrize("ms", [1, 0])
@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("shape", list(TC.PROBLEMS))
def test_overrides_equal_the_coarser_levels_bit_for_bit(shape, fp32, ms):
    """(a) overrides that all equal the robot's effective row give the bytes of no overrides, on a
    plain handle and over per-robot rows; (b) robot b's every phase on set b mod 5 gives the bytes
    of hsddp_set_element_weights with those sets; (c) set, then w = NULL, gives the bytes of a
    handle that never called it.  Every expression keeps its form: only where a weight comes from
    changes."""
    prob = TC.PROBLEMS[shape]()
    opts = {**FIXED, "MS": ms}
    plain, robot = _solve(prob, opts, fp32, None), _solve(prob, opts, fp32, "robot")
    assert not np.array_equal(plain["K"], robot["K"])
    _same(plain, _solve(prob, opts, fp32, "equal"), "(a) the handle's weights as overrides")
    _same(robot, _solve(prob, opts, fp32, "robot_and_equal"), "(a) the robots' rows as overrides")
    _same(robot, _solve(prob, opts, fp32, "phase"), "(b) overrides in place of the per-robot table")
    _same(plain, _solve(prob, opts, fp32, "on_off"), "(c) set, then NULL")


# ---- 4. every sweep kernel ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """the trot problem's five robots on test 2's rows, in a B = 5 handle: the small-handle copies"""
    prob = TC.shared_problem()
    rows = PW.phase_rows(prob)
    s = EW.gpu_solver(prob, FIXED)
    s.set_phase_weights(PW.table(prob, rows))
    s.solve()
    out = TC.downloads(s)
    s.close()
    return prob, rows, out


@pytest.mark.parametrize("B,split", [(6, "0"), (6, None), (520, None)], ids=["B6_one_wave", "B6_column_split", "B520_two_pairs"])
def test_every_sweep_kernel_reads_the_rows(small, monkeypatch, B, split):
    """Test 2's rows tiled (tiled_case): the one-wave sweep with one pair per workgroup (B = 6,
    HSDDP_SWEEP_SPLIT=0), the column split (B = 6) and two pairs per workgroup (B = 520).  Every
    element equals its small-handle copy bit for bit."""
    if split is not None:
        monkeypatch.setenv("HSDDP_SWEEP_SPLIT", split)
    prob, rows, ref = small
    for index in TT.draws(5, B, 3)[:2]:
        tiled = TT.tile(prob, index)
        s = EW.gpu_solver(tiled, FIXED)
        s.set_phase_weights(PW.table(tiled, [rows[i] for i in index]))
        s.solve()
        g = TC.downloads(s)
        s.close()
        for f in g:
            assert np.array_equal(np.asarray(g[f]), np.asarray(ref[f])[np.asarray(index)]), (B, split, f)


def test_a_retry_row_in_one_phase(monkeypatch):
    """Robot 1 of solver_params' retry case carries r_qJd = -0.5 in its second phase only, so its
    first sweep fails the PSD test there and k_riccati_retry runs the schedule with the rows: the
    parallel retry equals HSDDP_SEQUENTIAL_RETRY=1 bit for bit, the robot's solve depends on
    update_regularization (it retried) where the others' does not, and it differs from a handle whose
    robot carries the row in all phases."""
    case = SP.CASES["retries"]
    prob = SP.shape_batch(*SP.SHAPES[0], dt=case["dt"])
    opts = case["options"]
    hz = TC.phases_of(prob)
    bad = {**SP.WEIGHTS, "r_qJd": -0.5}

    def run(o, rows):
        s = EW.gpu_solver(prob, o)
        s.set_phase_weights(PW.table(prob, rows))
        s.solve()
        out = {**s.trajectory(), **s.working(), **s.element_info()}
        s.close()
        return out

    one = [[bad if (b, i) == (1, 1) else SP.WEIGHTS for i in range(len(hz[b]))] for b in range(prob["batch"])]
    every = [[bad if b == 1 else SP.WEIGHTS for i in range(len(hz[b]))] for b in range(prob["batch"])]
    g, g5, ga = run(opts, one), run({**opts, "update_regularization": 5.0}, one), run(opts, every)
    assert [b for b in range(prob["batch"]) if not np.array_equal(g["K"][b], g5["K"][b])] == [1]
    assert not np.array_equal(g["K"][1], ga["K"][1])
    for b in range(prob["batch"]):
        if b != 1:
            assert np.array_equal(g["K"][b], ga["K"][b]), b
    monkeypatch.setenv("HSDDP_SEQUENTIAL_RETRY", "1")
    q = run(opts, one)
    for f in TC.ARRAYS + TC.SCALARS + TC.DECISIONS:
        assert np.array_equal(g[f], q[f]), f


def test_retried_sweep_against_the_restatement_at_the_retried_mu():
    """The same rows (robot 1 of the retry case with r_qJd = -0.5 in its second phase only), one inner
    iteration through the split solve.  The restatement: oracle_lib.knot_eval's LQ terms at the
    initial rollout with each phase's row, and phase_weights_case.dense_sweep at every mu of the
    reference's schedule (0, then max(3 mu, 1e-3) up to 1e2).  By the reference's rule (Quu - 1e-9 I
    positive definite at every knot) the first admissible mu is a retried one (> 0) for robot 1 and 0
    for the others; the device's gains, feed-forward, dX and value function equal the restatement at
    that mu at test 2's 1e-9 and miss it at every other mu of the schedule — so k_riccati_retry read
    the one-phase row, at the retried mu.  With the row on all phases, or on none, the restatement
    misses."""
    case = SP.CASES["retries"]
    prob = SP.shape_batch(*SP.SHAPES[0], dt=case["dt"])
    opts = {**case["options"], "max_DDP_iter": 1}
    hz = TC.phases_of(prob)
    bad = {**SP.WEIGHTS, "r_qJd": -0.5}
    one = [[bad if (b, i) == (1, 1) else SP.WEIGHTS for i in range(len(hz[b]))] for b in range(prob["batch"])]
    s = EW.gpu_solver(prob, opts)
    s.set_value_export(True)
    s.set_phase_weights(PW.table(prob, one))
    s.begin()
    W0 = s.working()
    s.iterate(1)
    W1, tr, val = s.working(), s.trajectory(), s.value()
    s.close()
    mus = [0.0]
    while mus[-1] <= 1e2:
        mus.append(max(mus[-1] * opts["update_regularization"], 1e-3))
    for b in (0, 1, 2):
        P, S = len(hz[b]), sum(n + 1 for n in hz[b])
        T = PW.knot_terms(prob, b, W0, one[b], opts)
        refs = [PW.dense_sweep(hz[b], T, W0["Defect"][b], reg=mu) for mu in mus]
        first = next(k for k, r in enumerate(refs) if r["min_eig"] > 1e-9)
        assert (first > 0) == (b == 1), (b, mus[first])
        got = {"K": tr["K"][b], "dU": W1["dU"][b], "dX": W1["dX"][b, :S], "G": val["G"][b, :P], "H": val["H"][b, :P]}
        for f, a in got.items():
            e = TC.rel(a, refs[first][f])
            print(f"robot {b} mu {mus[first]:g} {f}: rel {e:.3e}")
            assert e < 1e-9, (b, f, e)
        for k, r in enumerate(refs):
            if k != first:
                assert TC.rel(got["K"], r["K"]) > 1e-6, ("another mu passes", b, mus[k])
        if b == 1:
            for rows in ([bad] * P, [SP.WEIGHTS] * P):
                Tw = PW.knot_terms(prob, b, W0, rows, opts)
                assert all(TC.rel(got["K"], PW.dense_sweep(hz[b], Tw, W0["Defect"][b], reg=mu)["K"]) > 1e-6 for mu in mus)


# ---- 5. ticks ----------------------------------------------------------------------------------------
PLAN = 0.4  # Kc = 40 on the trot file
STARTS = [8, 10, 13, 19]  # within five ticks robots 0 and 1 drop a first phase and robots 2 and 3 append a last one


def _tick_batch(copies, ms=1):
    import restart_case as RC
    tab, dt = hsddp.load_quad_reference(os.path.join(HERE, "golden", "ref_trot.csv"))
    out = []
    for _ in range(copies):
        p = hsddp.reference_problem(tab, dt, STARTS, RC.x0(len(STARTS), 40), plan_duration=PLAN)
        assert p["Kc"] == 40
        out.append(hsddp.Solver(p, hsddp.load_settings(**dict(RC.TICK, MS=ms)), cparams=SP.hsddp_cparams(), weights=SP.hsddp_weights()))
    return out


class _Rows:
    """the restatement: ref_oracle.ProblemTracker's phases with each robot's overrides riding on them
    (None: no override — an appended phase, a restarted robot's phases)"""

    def __init__(self, rows):
        import ref_oracle as R
        ref, dt = R.load_quad_reference(os.path.join(HERE, "golden", "ref_trot.csv"))
        self.R, self.ref, self.dt = R, ref, dt
        self.tk = [R.ProblemTracker(ref, w, dt, plan_duration=PLAN) for w in STARTS]
        self.rows = [list(r[:len(t.horizons)]) for r, t in zip(rows, self.tk)]
        self.events = [set() for _ in STARTS]

    def step(self):
        for b, t in enumerate(self.tk):
            n0, pop = len(t.horizons), t.horizons[0] <= 1
            t.step()
            app = len(t.horizons) - (n0 - pop)
            self.rows[b] = self.rows[b][int(pop):] + [None] * app
            self.events[b] |= ({"pop"} if pop else set()) | ({"append"} if app else set())

    def restart(self, b, start):
        self.tk[b] = self.R.ProblemTracker(self.ref, start, self.dt, plan_duration=PLAN)
        self.rows[b] = [None for _ in self.tk[b].horizons]

    def arrays(self, robot_rows):
        """the effective table [B][P][46] and the flags [B][P]"""
        P = max(len(r) for r in self.rows)
        t = np.array([[PW.vec(robot_rows[b])] * P for b in range(len(self.rows))])
        f = np.zeros((len(self.rows), P), np.int32)
        for b, r in enumerate(self.rows):
            for i, w in enumerate(r):
                if w is not None:
                    t[b, i], f[b, i] = PW.vec(w), 1
        return np.ascontiguousarray(t), f


@pytest.mark.parametrize("ms", [1, 0])
def test_overrides_ride_the_phases_through_ticks(ms):
    """Overrides set once on handle A (on a per-robot table, so a phase without one reads its robot's
    row); handle B is given the whole expected table and flags (the restatement's) after every
    advance, while its inputs are pending.  phase_weights() of A shows the moved rows and the
    appended phases without one after every advance, and A and B are equal bit for bit every tick.
    In the fourth tick robot 2 of A and B restarts: no overrides for it, its per-robot row kept."""
    import restart_case as RC
    A, Bh = _tick_batch(2, ms)
    n = len(STARTS)
    sets = EW.robot_sets(n)
    P0 = A.P
    rng = np.random.default_rng(3)
    first = [[{**EW.weight_set(b + i), "r_grf": SP.WEIGHTS["r_grf"] * (0.7 + 0.6 * rng.random())} if (b + i) % 3 else None
              for i in range(P0)] for b in range(n)]
    rows = _Rows(first)
    t0, f0 = rows.arrays(sets)
    for s in (A, Bh):
        s.set_element_weights(EW.rows(sets))
        s.set_phase_weights(t0, f0)
        s.solve()
    for it in range(5):
        x = RC.x0(n, 60 + it)
        rows.step()
        for s in (A, Bh):
            s.advance(None, 1, PLAN)
        if it == 3:
            rows.restart(2, 30)
            ws = np.array([0, 0, 30, 0], np.int32)
            for s in (A, Bh):
                s.restart_elements([0, 0, 1, 0], ws, None, PLAN)
        t, f = rows.arrays(sets)
        got, flags = A.phase_weights()
        assert got.shape == t.shape and np.array_equal(flags, f) and np.array_equal(got, t), it
        Bh.set_phase_weights(t, f)
        assert [EW.as_bytes(w) for w in A.element_weights()] == [EW.as_bytes(w) for w in EW.rows(sets)], it
        for s in (A, Bh):
            s.update_problem(None, x)
            s.solve()
        a, b = RC.snapshot(A), RC.snapshot(Bh)
        assert [list(h) for h in a["horizons"]] == [tk.horizons for tk in rows.tk], it
        for e in range(n):
            RC.same_element(a, b, e)
    assert {"pop"} <= rows.events[0] | rows.events[1] and {"append"} <= rows.events[2] | rows.events[3], rows.events
    A.close(); Bh.close()


def test_uniform_overrides_ticks_match_the_oracle_per_robot():
    """Robot b's every phase on weight set b (and its per-robot row on the same set, which the phases
    the ticks append read), set once before the first tick.  The initial solve with the shipped
    settings and five ticks of hsddp_advance + re-solve (max_AL_iter = 2, max_DDP_iter = 1) — phases
    leave and enter at different ticks, the stride changes, the table goes up again at the new stride —
    equal, tick by tick and robot by robot, the oracle doing the same with that robot's weights and the
    restated bookkeeping, as test_gpu_terrain.test_ticks_match_the_oracle_per_robot does for terrain
    and with its tolerances.  The per-phase instantiations run throughout (overrides remain), and an
    appended phase has none.  A kernel that read another robot's row after an advance (a stale stride,
    a row not moved) would solve some robot on another robot's weights."""
    import mpc_oracle as M
    import oracle_lib as O
    import ref_oracle as R
    import restart_case as RC
    path = os.path.join(HERE, "golden", "ref_trot.csv")
    tab, dt = hsddp.load_quad_reference(path)
    ref, _ = R.load_quad_reference(path)
    B = len(STARTS)
    sets = EW.robot_sets(B)
    x0 = RC.x0(B, 40)
    p = hsddp.reference_problem(tab, dt, STARTS, x0, plan_duration=PLAN)
    assert p["Kc"] == 40 and p.get("layouts") is not None
    n_win = int(p["window_len"])
    dev = hsddp.Solver(p, hsddp.load_settings())
    dev.set_element_weights(EW.rows(sets))
    dev.set_phase_weights(np.ascontiguousarray(np.array([[PW.vec(sets[b])] * dev.P for b in range(B)])))
    dev.solve()
    tks = [R.ProblemTracker(ref, w, dt, plan_duration=PLAN) for w in STARTS]

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
                print(f"{where} robot {b} {f}: rel {e:.3e}")
                assert e <= 1e-8, (where, b, f, e)
            assert g["n_ls_trials"][b] == r[b]["n_ls_trials"][0], (where, b)

    r = [O.solve_batch(problem_of(tks[b], x0[b]), O.default_options(), weights=sets[b]) for b in range(B)]
    compare(r, "initial")
    # the robots are weighted differently: with robot 1's set robot 0's solve is another one
    r_other = O.solve_batch(problem_of(tks[0], x0[0]), O.default_options(), weights=sets[1])
    assert TC.rel(r_other["Ubar"], r[0]["Ubar"]) > 1e-6
    kw = dict(max_AL_iter=2, max_DDP_iter=1)
    dev.set_options(hsddp.load_settings(**kw))
    op, _ = O.default_problem(p["horizons"], p["dt"])
    events = [set() for _ in tks]
    strides = {dev.P}
    for it in range(5):
        x = RC.x0(B, 60 + it)
        dev.advance(x, 1, PLAN)
        strides.add(dev.P)
        for b, tk in enumerate(tks):
            hz0, ss0, re0 = list(tk.horizons), list(tk.shooting), list(tk.reach_end)
            flags = tk.update(1)
            events[b] |= ({"pop"} if hz0[0] <= 1 else set()) | ({"append"} if len(tk.horizons) > len(hz0) - (hz0[0] <= 1) else set())
            sh = M.shift(hz0, ss0, re0, r[b]["Xbar"][0], r[b]["X"][0], r[b]["Ubar"][0], r[b]["K"][0], flags)
            cons = M.resolve_td(M.shift_constraints(hz0, re0, {k: r[b][k][0] for k in O.CONSTRAINT_FIELDS}, flags,
                                                    op.grf_delta, op.grf_eps, op.td_sigma, op.td_lambda), tk.contact_rows())
            cons = {k: np.asarray(cons[k])[None] for k in O.CONSTRAINT_FIELDS}
            r[b] = O.solve_batch(problem_of(tk, x[b], sh[3], sh[4], sh[5]), O.default_options(**kw), constraints=cons,
                                 weights=sets[b])
        rows, is_set = dev.phase_weights()
        assert is_set.any(), it  # (the per-phase instantiations run)
        for b, tk in enumerate(tks):
            assert np.array_equal(rows[b, :len(tk.horizons)], np.array([PW.vec(sets[b])] * len(tk.horizons))), (it, b)
        dev.solve()
        compare(r, it)
    for b, tk in enumerate(tks):  # an appended phase has no override of its own
        if "append" in events[b]:
            assert not is_set[b, len(tk.horizons) - 1], b
    assert "pop" in events[0] | events[1] and "append" in events[2] | events[3] and len(strides) > 1, (events, strides)
    dev.close()


# ---- 6. remaining behaviour --------------------------------------------------------------------------
def _per_element_refs(prob):
    prob = dict(prob)
    for k in ("ref_x", "ref_u", "ref_foot"):
        prob[k] = np.ascontiguousarray(np.repeat(prob[k], prob["batch"], axis=0))
    return prob


def test_overrides_travel_with_moved_robots():
    """hsddp_copy_elements and hsddp_export_elements / hsddp_import_elements of a robot with overrides
    into a handle without any (which takes them up) and into one with some: flags and rows arrive
    with the robot, its next solve equals the one it runs in place bit for bit, the residents' equals
    a twin's that received nothing.  A record whose version word reads "HEL3", and one with a NaN in
    an override, are refused with the handle unchanged."""
    prob = _per_element_refs(TC.shared_problem())
    opts = {"max_AL_iter": 2, "max_DDP_iter": 3, **SP.SCHEDULE}
    src, cp, imp, plain, twin = (EW.gpu_solver(prob, opts) for _ in range(5))
    rows = PW.phase_rows(prob)
    mask = PW.own_mask(prob)
    mask[:, 1] = 0  # (every robot's second phase without an override)
    src.set_phase_weights(PW.table(prob, rows), mask)
    other = PW.table(prob, PW.phase_rows(prob, seed=12))
    for h in (imp, twin):
        h.set_phase_weights(other, mask[::-1].copy())
    for h in (src, cp, imp, plain, twin):
        h.solve()
    cp.copy_elements(src, [0], [2])
    rec = src.export_elements([4])
    old = rec.copy()
    old[0, :4] = np.frombuffer(np.uint32(0x48454c33).tobytes(), np.uint8)  # "HEL3"
    bad = rec.copy()
    head = rec[0, :16384].tobytes()
    at = head.find(np.float64(rows[4][2]["q_qJ"]).tobytes())
    assert at >= 0
    bad[0, at:at + 8] = np.frombuffer(np.float64(np.nan).tobytes(), np.uint8)
    before = imp.phase_weights()
    for r, why in ((old, "version"), (bad, "weight")):
        with pytest.raises(hsddp.HSDDPError, match=why):
            imp.import_elements([1], r)
        after = imp.phase_weights()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    imp.import_elements([1], rec)
    st, sf = src.phase_weights()
    ct, cf = cp.phase_weights()
    it_, if_ = imp.phase_weights()
    own = PW.vec(SP.WEIGHTS)
    assert np.array_equal(cf[0], sf[2]) and np.array_equal(ct[0], st[2]) and not cf[1:].any() and np.all(ct[1:] == own)
    assert np.array_equal(if_[1], sf[4]) and np.array_equal(it_[1], st[4])
    assert np.array_equal(if_[[0, 2, 3, 4]], before[1][[0, 2, 3, 4]]) and np.array_equal(it_[[0, 2, 3, 4]], before[0][[0, 2, 3, 4]])
    for h in (src, cp, imp, plain, twin):
        h.solve()
    a, b, c, d, e = (TC.downloads(h) for h in (src, cp, imp, plain, twin))
    for h in (src, cp, imp, plain, twin):
        h.close()
    for f in a:
        assert np.array_equal(a[f][2], b[f][0]), ("copied robot", f)
        assert np.array_equal(a[f][4], c[f][1]), ("imported robot", f)
        assert np.array_equal(b[f][1:], d[f][1:]), ("copy's residents", f)
        assert np.array_equal(c[f][[0, 2, 3, 4]], e[f][[0, 2, 3, 4]]), ("import's residents", f)


def test_element_weights_beneath_overrides_change_only_the_phases_without_one():
    """Robots 1 and 3 have overrides on phases 0 and 2.  hsddp_set_element_weights then changes what
    their phases 1 and 3 read, and nothing else: phase_weights() shows it, and the solve equals, bit
    for bit, a handle given the whole effective table as overrides."""
    prob = TC.shared_problem()
    rows = PW.phase_rows(prob)
    mask = np.zeros((5, 4), np.int32)
    mask[[1, 3], 0] = mask[[1, 3], 2] = 1
    sets = EW.robot_sets(5)
    s, t = EW.gpu_solver(prob, FIXED), EW.gpu_solver(prob, FIXED)
    s.set_phase_weights(PW.table(prob, rows), mask)
    s.set_element_weights(EW.rows(sets))
    got, flags = s.phase_weights()
    assert np.array_equal(flags, mask)
    want = PW.table(prob, [[rows[b][i] if mask[b, i] else sets[b] for i in range(4)] for b in range(5)])
    assert np.array_equal(got, want)
    t.set_phase_weights(want)
    for h in (s, t):
        h.solve()
    _same(TC.downloads(s), TC.downloads(t), "effective table")
    s.close(); t.close()


def test_new_rows_on_a_warm_handle_recompute_the_slot_costs():
    """Solve, give robots 1 and 3 overrides in phases 1 and 2, begin(); iterate(1).  The slot costs the
    iteration starts from (lq()["l"]) are the new rows': they equal a twin's that set the same
    overrides after begin() (slots_fresh cleared: k_lq's SLOTS instantiation forms them), and differ
    from the untouched handle's in exactly those phases' knots; robots 0, 2 and 4 continue bit for
    bit as in the handle never touched."""
    prob = TC.shared_problem()
    opts = {"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 2, **SP.SCHEDULE}
    rows = PW.phase_rows(prob)
    mask = np.zeros((5, 4), np.int32)
    mask[[1, 3], 1] = mask[[1, 3], 2] = 1
    outs = {}
    for name in ("never", "set", "set_after_begin"):
        s = EW.gpu_solver(prob, opts)
        s.solve()
        if name == "set":
            s.set_phase_weights(PW.table(prob, rows), mask)
        s.begin()
        if name == "set_after_begin":
            s.set_phase_weights(PW.table(prob, rows), mask)
        s.iterate(1)
        outs[name] = TC.downloads(s)
        s.close()
    _same(outs["set"], outs["set_after_begin"], "slot costs by k_lq")
    for f in outs["set"]:
        for b in (0, 2, 4):
            assert np.array_equal(outs["set"][f][b], outs["never"][f][b]), ("untouched robot", b, f)
    for b in (1, 3):
        l, l0 = outs["set"]["lq_l"][b], outs["never"]["lq_l"][b]
        assert np.all(l[10:30] != l0[10:30]), b
        assert not np.array_equal(outs["set"]["K"][b], outs["never"]["K"][b]), b


def test_simulate_policy_costs_follow_the_knots_phase():
    """k_simulate_policy as the first consumer of a changed table: after a solve, robot 0 gets overrides
    in its second and third phase and hsddp_simulate_policy runs at once over 12 knots of 3 x 4.  The
    per-sample costs equal tests/sim_reference.py's helper summed phase by phase with each phase's
    weights (costs of a prefix are sums over knots, so a run with phase i's weights minus the run
    before it gives the phase's part), at test_gpu_simulate's tolerance; robots 1 and 2 keep their
    costs bit for bit."""
    import sim_reference as R
    import test_gpu_simulate as TS
    from hsddp import synthetic as syn
    prob = syn.make_batch(3, 3, 4, "trot")
    s = hsddp.Solver(prob, hsddp.load_settings(**TS.FIXED), weights=SP.hsddp_weights())
    s.solve()
    tr = s.trajectory()
    x = TS.perturbed(tr["Xbar"][:, 0], 70, seed=23)
    n = 12
    g0 = TS.flat(s.simulate_policy(x, n))
    rows = [[SP.WEIGHTS, EW.weight_set(1), EW.weight_set(3)]] + [[SP.WEIGHTS] * 3] * 2
    mask = np.array([[0, 1, 1], [0, 0, 0], [0, 0, 0]], np.int32)
    s.set_phase_weights(PW.table(prob, rows), mask)
    g = TS.flat(s.simulate_policy(x, n))
    s.close()
    assert np.array_equal(g["cost"][1:], g0["cost"][1:])
    # phase i's part of the cost: its knots' running costs and its terminal cost, under its weights;
    # the helper's prefix of k knots holds the phases that end within them
    def cost(w, k, scale=1.0):
        return R.prefix(R.simulate(prob, tr, x * scale, k, weights=w), k)["cost"][0] if k else 0.0
    want = want2 = 0.0
    for i, w in enumerate(rows[0]):
        want = want + cost(w, 4 * (i + 1)) - cost(w, 4 * i)
        want2 = want2 + cost(w, 4 * (i + 1), 1 + 1e-15) - cost(w, 4 * i, 1 + 1e-15)
    e, tol = TS.rel(g["cost"][0], want), max(1e-9, 10 * TS.rel(want2, want))
    print(f"simulate robot 0 cost: rel {e:.3e} (bound {tol:.3e})")
    assert e < tol, (e, tol)
    assert TS.rel(g["cost"][0], g0["cost"][0]) > 1e-6


def test_graph_replayed_solve_equals_the_split_solve(monkeypatch):
    """B = 1 at the shipped settings (early exits: the inner iteration replayed from a graph keyed on
    the table pointer): a full solve with overrides differs from the plain handle's and equals the
    same solve through the split launches (HSDDP_NO_GRAPH=1) bit for bit; so does the second solve
    after w = NULL, which replays the graphs of a handle without overrides."""
    prob = TC.shared_problem()
    one = TT.tile(prob, [2])
    table = PW.table(one, [PW.phase_rows(prob)[2]])
    outs = {}
    for graph in (True, False):
        if not graph:
            monkeypatch.setenv("HSDDP_NO_GRAPH", "1")
        s = EW.gpu_solver(one, {})
        s.set_phase_weights(table)
        s.solve()
        first = TC.downloads(s)
        s.set_phase_weights(None)
        assert not s.phase_weights()[1].any()
        s.solve()
        outs[graph] = (first, TC.downloads(s))
        s.close()
    monkeypatch.delenv("HSDDP_NO_GRAPH")
    p = EW.gpu_solver(one, {})
    p.solve()
    assert not np.array_equal(outs[True][0]["K"], TC.downloads(p)["K"])
    p.close()
    _same(outs[True][0], outs[False][0], "graph against split launches")
    _same(outs[True][1], outs[False][1], "after w = NULL")


def test_argument_checks():
    """No problem uploaded: refused.  A NaN in a masked row: refused, every download unchanged.  A NaN
    in an unmasked row or past a robot's phases: not read.  Negative weights stay legal."""
    import ctypes as C
    L = hsddp.lib()
    prob = TC.mixed_problem()
    s = EW.gpu_solver(prob, FIXED)
    rows = PW.table(prob, PW.phase_rows(prob))
    s.set_phase_weights(rows, PW.own_mask(prob))
    s.solve()
    before, (t0, f0) = TC.downloads(s), s.phase_weights()
    bad = rows.copy()
    bad[3, 2, 17] = np.nan
    with pytest.raises(hsddp.HSDDPError, match="finite"):
        s.set_phase_weights(bad)
    t1, f1 = s.phase_weights()
    assert np.array_equal(t0, t1) and np.array_equal(f0, f1)
    _same(before, TC.downloads(s), "refused call")
    m = PW.own_mask(prob)
    m[3, 2] = 0
    s.set_phase_weights(bad, m)  # (the NaN row is not read)
    past = rows.copy()
    assert len(TC.phases_of(prob)[0]) == 4 and rows.shape[1] == 8
    past[0, 5, 3] = np.nan  # (robot 0 has four phases)
    s.set_phase_weights(past)
    t2, f2 = s.phase_weights()
    assert np.array_equal(f2, PW.own_mask(prob)) and np.isfinite(t2).all()
    at = int(np.flatnonzero(PW.vec({**SP.WEIGHTS, "r_qJd": -0.5}) != PW.vec(SP.WEIGHTS))[0])
    neg = rows.copy()
    neg[:, :, at] = -0.5  # r_qJd
    s.set_phase_weights(neg)
    assert s.phase_weights()[0][2, 1, at] == -0.5
    s.close()
    desc = hsddp.ProblemDesc()
    desc.device, desc.batch, desc.n_phases, desc.dt, desc.ref_per_element = 0, 5, 4, float(prob["dt"]), 0
    for i in range(4):
        desc.horizons[i] = 10
    L.hsddp_default_weights(C.byref(desc.weights))
    L.hsddp_default_constraint_params(C.byref(desc.cparams))
    h = C.c_void_p()
    assert L.hsddp_create(C.byref(desc), C.byref(h)) == 0
    arr = (hsddp.Weights * 20)()
    flags = (C.c_int * 20)()
    assert L.hsddp_set_phase_weights(h, C.addressof(arr), None) == -1
    assert L.hsddp_set_phase_weights(h, None, None) == -1
    assert L.hsddp_get_phase_weights(h, C.addressof(arr), C.addressof(flags)) == -1
    L.hsddp_destroy(h)


# ---- 7. the facade -----------------------------------------------------------------------------------
def test_facade_solves_with_per_phase_cost_objects():
    """tests/drivers/phase_weights_facade device: MultiPhaseDDP::solve of a problem whose phases' cost
    objects differ, through the hkd:: terms and through diagonals alone, over three ticks: everything
    it writes back equals the C ABI given describe()'s arrays and hsddp_set_phase_weights byte for
    byte, and differs without the overrides."""
    import subprocess
    drivers = os.path.join(HERE, "drivers")
    r = subprocess.run(["make", "-C", drivers, "-f", "phase_weights.mk", "phase_weights_facade"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(drivers, "phase_weights_facade"), "device"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "phase_weights_facade device ok" in r.stdout, r.stdout + r.stderr
