"""Per-robot cost weights (hsddp_set_element_weights): a row of HKD weights for each robot of a batch,
against the unmodified oracle — which takes one set of weights per problem, so it is run per robot —
and bit for bit against handles created with a robot's row as their handle-wide weights.

Shapes (terrain_case.py): Kc = 40, the shared layout 4 x 10 with B = 5 and a mix of 4 x 10 and 8 x 5
layouts with B = 6, at solver_params.WEIGHTS / CPARAMS from warm-start controls with pyramid rows on
both sides of delta; fixed small iteration budgets; multiple and single shooting.
"""
import ctypes as C

import numpy as np
import pytest

import hsddp
import element_weights_case as EW
import solver_params as SP
import terrain_case as TC
import tiled_case as TT
from test_gpu_terrain import FIXED, _compare_robots

pytestmark = pytest.mark.gpu


def _same(a, b, where):
    for f in a:
        assert np.array_equal(a[f], b[f]), (where, f)


# ---- 1. per robot against the oracle ----------------------------------------------------------------
@pytest.mark.parametrize("ms", [1, 0])
@pytest.mark.parametrize("shape", list(TC.PROBLEMS))
def test_robot_weights_match_oracle_per_robot(shape, ms):
    """Robot b on weight set b mod 5 (each differs from the handle's SP.WEIGHTS in every field
    group): everything the solve leaves equals the oracle's solve of that robot alone with those
    weights, by test_gpu_terrain._compare_robots' rule."""
    prob = TC.PROBLEMS[shape]()
    opts = {**FIXED, "MS": ms}
    sets = EW.robot_sets(prob["batch"])
    r = EW.oracle_robots(prob, opts, sets)
    r2 = EW.oracle_robots(prob, opts, sets, 1 + 1e-15)
    for f in TC.DECISIONS:
        assert np.array_equal(r[f], r2[f]), f  # (nothing to screen)
    s = EW.gpu_solver(prob, opts)
    rows = EW.rows(sets)
    s.set_element_weights(rows)
    back = s.element_weights()
    assert [EW.as_bytes(w) for w in back] == [EW.as_bytes(w) for w in rows]
    s.solve()
    g = TC.mask_padding(prob, TC.downloads(s))
    s.close()
    _compare_robots(g, r, r2, f"{shape} MS={ms}")


# ---- 2. one field group at a time, bit for bit ------------------------------------------------------
def _run(s, full):
    if full:
        s.solve()
    else:
        s.begin()
        s.iterate(2)
    out = TC.downloads(s)
    out.update({"val_" + k: v for k, v in s.value().items()})
    return out


@pytest.mark.parametrize("full", [False, True], ids=["begin_iterate2", "solve"])
def test_one_field_group_at_a_time_bit_for_bit(full):
    """13 copies of one robot of the shared problem; copy g < 12 differs from the handle's weights in
    one field group only, copy 12 is left unset.  Every download of copy g equals, bit for bit, that
    of a B = 1 handle created with copy g's weights, and differs from copy 12's in the gains or the
    costs — so no site can pass while ignoring the table."""
    base = TC.shared_problem()
    prob = TT.tile(base, [1] * 13)
    one = TT.tile(base, [1])
    sets = EW.group_sets()
    s = EW.gpu_solver(prob, FIXED)
    s.set_value_export(True)
    mask = np.ones(13, np.int32)
    mask[12] = 0
    rows = EW.rows(sets)
    rows[12] = SP.hsddp_weights(EW.weight_set(0))  # (masked out: never read)
    s.set_element_weights(rows, mask)
    assert EW.as_bytes(s.element_weights()[12]) == EW.as_bytes(SP.hsddp_weights())
    g = _run(s, full)
    s.close()
    bad = []
    for b in range(13):
        t = EW.gpu_solver(one, FIXED, sets[b])
        t.set_value_export(True)
        ref = _run(t, full)
        t.close()
        for f in g:
            x, y = np.asarray(g[f])[b], np.asarray(ref[f])[0]
            if not np.array_equal(x, y):
                at = np.argwhere(np.atleast_1d(x != y))
                print(f"robot {b} {f}: {len(at)} of {x.size} entries differ, first at {at[0].tolist()}, max |diff| {np.max(np.abs(np.atleast_1d(x - y))):.3e}")
                bad.append((b, EW.GROUPS[b] if b < 12 else "unset", f))
        if b < 12:
            moved = [f for f in ("K", "cost", "lq_l", "lq_lx", "lq_lu", "tm_Phi", "tm_Phix") if not np.array_equal(g[f][b], g[f][12])]
            assert moved, ("the group changes nothing", EW.GROUPS[b])
    assert not bad, bad


# ---- 3. a table equal to the handle's weights changes nothing ---------------------------------------
def _solve_all(prob, opts, fp32, table):
    s = EW.gpu_solver(prob, opts, None, fp32)
    if table == "on":
        s.set_element_weights([SP.hsddp_weights()] * prob["batch"])
    elif table == "on_off":
        s.set_element_weights(EW.rows(EW.robot_sets(prob["batch"])))
        s.set_element_weights(None)
        assert [EW.as_bytes(w) for w in s.element_weights()] == [EW.as_bytes(SP.hsddp_weights())] * prob["batch"]
    s.solve()
    out = TC.downloads(s)
    s.close()
    return out


@pytest.mark.parametrize("ms", [1, 0])
@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("shape", list(TC.PROBLEMS))
def test_table_of_the_handles_weights_equals_no_table_bit_for_bit(shape, fp32, ms):
    """Rows that all equal the handle's weights give byte-identical downloads to the handle without a
    table (every expression keeps its form; only where a weight comes from changes), and turning the
    table off again (w = NULL) restores the off path."""
    prob = TC.PROBLEMS[shape]()
    opts = {**FIXED, "MS": ms}
    plain = _solve_all(prob, opts, fp32, None)
    _same(plain, _solve_all(prob, opts, fp32, "on"), "table on")
    _same(plain, _solve_all(prob, opts, fp32, "on_off"), "table on, then off")


# ---- 4. every sweep kernel --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    """the trot problem's five robots on the five sets, in a B = 5 handle: the small-handle copies"""
    prob = TC.shared_problem()
    s = EW.gpu_solver(prob, FIXED)
    s.set_element_weights(EW.rows(EW.robot_sets(5)))
    s.solve()
    out = TC.downloads(s)
    s.close()
    return prob, out


@pytest.mark.parametrize("B,split", [(6, "0"), (6, None), (520, None)], ids=["B6_one_wave", "B6_column_split", "B520_two_pairs"])
def test_every_sweep_kernel_reads_the_rows(small, monkeypatch, B, split):
    """The sets of test 1 tiled (tiled_case): the one-wave sweep with one pair per workgroup (B = 6,
    HSDDP_SWEEP_SPLIT=0), the column split (B = 6) and two pairs per workgroup (B = 520), on a trot
    problem (the masked knot loops).  Every element equals its small-handle copy bit for bit."""
    if split is not None:
        monkeypatch.setenv("HSDDP_SWEEP_SPLIT", split)
    prob, ref = small
    sets = EW.robot_sets(5)
    for index in TT.draws(5, B, 3)[:2]:
        tiled = TT.tile(prob, index)
        s = EW.gpu_solver(tiled, FIXED)
        s.set_element_weights(EW.rows([sets[i] for i in index]))
        s.solve()
        g = TC.downloads(s)
        s.close()
        for f in g:
            assert np.array_equal(np.asarray(g[f]), np.asarray(ref[f])[np.asarray(index)]), (B, split, f)


def test_graph_replayed_solve_equals_a_handle_created_with_the_row():
    """B = 1 at the shipped settings (early exits: the inner iteration replayed from a graph keyed on
    the table pointer): a full solve with a row equals the solve of a handle created with that row,
    and a second solve after turning the table off equals the plain handle's second solve."""
    one = TT.tile(TC.shared_problem(), [2])
    w = EW.weight_set(3)
    s, t, p = EW.gpu_solver(one, {}), EW.gpu_solver(one, {}, w), EW.gpu_solver(one, {})
    s.set_element_weights(EW.rows([w]))
    for h in (s, t, p):
        h.solve()
    a, b, c = TC.downloads(s), TC.downloads(t), TC.downloads(p)
    _same(a, b, "row against created")
    assert not np.array_equal(a["K"], c["K"])
    s.close()
    t.close()
    p.close()


# ---- 6. changing weights on a warm handle -----------------------------------------------------------
def test_new_rows_on_a_warm_handle_recompute_the_slot_costs():
    """Solve, give robots 1 and 3 new rows, begin(); iterate(1).  The slot costs k_lq stores for the
    iteration (lq()["l"], the cost the iteration starts from) are those of the new rows — they equal
    a twin handle's that had the rows from the start of that second solve and so formed them in its
    rollout — and differ from the untouched handle's; robots 0, 2 and 4 continue bit for bit as in
    the handle never touched.  Setting the same rows again after begin() (slots_fresh cleared: k_lq's
    SLOTS instantiation forms the costs) changes nothing."""
    prob = TC.shared_problem()
    opts = {"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 2, **SP.SCHEDULE}
    sets = [dict(SP.WEIGHTS) for _ in range(5)]
    sets[1], sets[3] = EW.weight_set(1), EW.weight_set(3)
    outs = {}
    for name in ("never", "set", "set_again"):
        s = EW.gpu_solver(prob, opts)
        s.solve()
        if name != "never":
            mask = np.array([0, 1, 0, 1, 0], np.int32)
            s.set_element_weights(EW.rows(sets), mask)
        s.begin()
        if name == "set_again":
            s.set_element_weights(EW.rows(sets), mask)
        s.iterate(1)
        outs[name] = TC.downloads(s)
        s.close()
    _same(outs["set"], outs["set_again"], "slot costs by k_lq")
    for f in outs["set"]:
        for b in (0, 2, 4):
            assert np.array_equal(outs["set"][f][b], outs["never"][f][b]), ("untouched robot", b, f)
    for b in (1, 3):
        assert TC.rel(outs["set"]["lq_l"][b], outs["never"]["lq_l"][b]) > 1e-6, b
        assert not np.array_equal(outs["set"]["K"][b], outs["never"]["K"][b]), b


# ---- 7. moves ---------------------------------------------------------------------------------------
def _per_element_refs(prob):
    prob = dict(prob)
    for k in ("ref_x", "ref_u", "ref_foot"):
        prob[k] = np.ascontiguousarray(np.repeat(prob[k], prob["batch"], axis=0))
    return prob


def test_rows_travel_with_moved_robots():
    """hsddp_copy_elements and hsddp_export_elements / hsddp_import_elements of a robot with a row
    into handles with the table off: the destination's table turns on with the robot's row and the
    handle's weights elsewhere, the robot's next solve equals the one it runs in place bit for bit,
    the residents' equals a handle's that received nothing.  A record whose version word reads "HEL2",
    and one with a NaN in its row, are refused with the handle unchanged."""
    prob = _per_element_refs(TC.shared_problem())
    opts = {"max_AL_iter": 2, "max_DDP_iter": 3, **SP.SCHEDULE}
    src, cp, imp, plain = (EW.gpu_solver(prob, opts) for _ in range(4))
    sets = EW.robot_sets(5)
    src.set_element_weights(EW.rows(sets))
    for h in (src, cp, imp, plain):
        h.solve()
    cp.copy_elements(src, [0], [2])
    rec = src.export_elements([4])
    old = rec.copy()
    old[0, :4] = np.frombuffer(np.uint32(0x48454c32).tobytes(), np.uint8)  # "HEL2"
    bad = rec.copy()
    head = rec[0, :8192].tobytes()
    at = head.find(np.float64(sets[4]["q_qJ"]).tobytes())
    assert at >= 0
    bad[0, at:at + 8] = np.frombuffer(np.float64(np.nan).tobytes(), np.uint8)
    for r, why in ((old, "version"), (bad, "weight")):
        with pytest.raises(hsddp.HSDDPError, match=why):
            imp.import_elements([1], r)
        assert [EW.as_bytes(w) for w in imp.element_weights()] == [EW.as_bytes(SP.hsddp_weights())] * 5
    imp.import_elements([1], rec)
    own = EW.as_bytes(SP.hsddp_weights())
    assert [EW.as_bytes(w) for w in cp.element_weights()] == [EW.as_bytes(SP.hsddp_weights(sets[2]))] + [own] * 4
    assert [EW.as_bytes(w) for w in imp.element_weights()] == [own, EW.as_bytes(SP.hsddp_weights(sets[4]))] + [own] * 3
    for h in (src, cp, imp, plain):
        h.solve()
    a, b, c, d = (TC.downloads(h) for h in (src, cp, imp, plain))
    for h in (src, cp, imp, plain):
        h.close()
    for f in a:
        assert np.array_equal(a[f][2], b[f][0]), ("copied robot", f)
        assert np.array_equal(a[f][4], c[f][1]), ("imported robot", f)
        assert np.array_equal(b[f][1:], d[f][1:]), ("copy's residents", f)
        assert np.array_equal(c[f][[0, 2, 3, 4]], d[f][[0, 2, 3, 4]]), ("import's residents", f)


# ---- 9. argument checks -----------------------------------------------------------------------------
def test_argument_checks():
    """No problem uploaded: refused.  A NaN in a masked row: refused, nothing changed.  A NaN in an
    unmasked row: ignored.  Negative weights stay legal."""
    L = hsddp.lib()
    prob = TC.shared_problem()
    s = EW.gpu_solver(prob, FIXED)
    rows = EW.rows(EW.robot_sets(5))
    s.set_element_weights(rows)
    before = [EW.as_bytes(w) for w in s.element_weights()]
    bad = EW.rows(EW.robot_sets(5)[::-1])
    bad[3].qf_scale[7] = float("nan")
    with pytest.raises(hsddp.HSDDPError, match="finite"):
        s.set_element_weights(bad)
    assert [EW.as_bytes(w) for w in s.element_weights()] == before
    s.set_element_weights(bad, np.array([1, 0, 0, 0, 0], np.int32))  # (the NaN row is not read)
    after = [EW.as_bytes(w) for w in s.element_weights()]
    assert after == [EW.as_bytes(bad[0])] + before[1:]
    neg = EW.rows([{**SP.WEIGHTS, "r_qJd": -0.5}] * 5)
    s.set_element_weights(neg)
    assert s.element_weights()[2].r_qJd == -0.5
    s.close()
    # a handle without a problem
    desc = hsddp.ProblemDesc()
    desc.device, desc.batch, desc.n_phases, desc.dt, desc.ref_per_element = 0, 5, 4, float(prob["dt"]), 0
    for i in range(4):
        desc.horizons[i] = 10
    L.hsddp_default_weights(C.byref(desc.weights))
    L.hsddp_default_constraint_params(C.byref(desc.cparams))
    h = C.c_void_p()
    assert L.hsddp_create(C.byref(desc), C.byref(h)) == 0
    arr = (hsddp.Weights * 5)()
    assert L.hsddp_set_element_weights(h, C.addressof(arr), None) == -1
    assert L.hsddp_set_element_weights(h, None, None) == -1
    assert L.hsddp_get_element_weights(h, C.addressof(arr)) == -1
    L.hsddp_destroy(h)


# ---- 5. retries for some robots only ----------------------------------------------------------------
RETRY_ROBOTS = (1, 4)


def _retry_sets():
    return [{**SP.WEIGHTS, "r_qJd": -0.5} if b in RETRY_ROBOTS else dict(SP.WEIGHTS) for b in range(SP.BATCH)]


def _oracle_each(prob, opts, sets, x0_scale=1.0):
    import oracle_lib as O
    p = dict(prob)
    if x0_scale != 1.0:
        p["x0"] = p["x0"] * x0_scale
    out = {}
    for b in range(prob["batch"]):
        r = O.solve_batch(p, O.default_options(**opts), elements=[b], weights=sets[b], cparams=SP.oracle_cparams())
        for k, v in r.items():
            if k != "solver_info":
                out.setdefault(k, []).append(np.asarray(v)[0])
    return {k: np.array(v) for k, v in out.items()}


def _gpu_rows_solve(prob, opts, sets):
    s = EW.gpu_solver(prob, opts)
    s.set_element_weights(EW.rows(sets))
    s.solve()
    out = {**s.trajectory(), **s.working(), **s.element_info()}
    s.close()
    return out


def test_retries_for_some_robots_only(monkeypatch):
    """Robots 1 and 4 of six carry r_qJd = -0.5 in their rows (solver_params' retry case): their first
    sweeps fail the PSD test and run the schedule mu = 1e-3, 3e-3, 9e-3 ..., the others' do not.  A
    robot retries exactly when its solve depends on update_regularization (3 against 5; the first
    retry's mu is 1e-3 under both): checked on the oracle first, then on the device.  Statuses,
    iteration and trial counts equal the oracle's per robot, the arrays within test 1's rule, and the
    parallel retry (k_riccati_retry with rows) equals HSDDP_SEQUENTIAL_RETRY=1 bit for bit."""
    case = SP.CASES["retries"]
    prob = SP.shape_batch(*SP.SHAPES[0], dt=case["dt"])
    opts, sets = case["options"], _retry_sets()
    other = {**opts, "update_regularization": 5.0}
    r, r2, r5 = _oracle_each(prob, opts, sets), _oracle_each(prob, opts, sets, 1 + 1e-15), _oracle_each(prob, other, sets)
    for f in TC.DECISIONS:
        assert np.array_equal(r[f], r2[f]), f  # (nothing to screen)
    assert np.all(r["status"] == 0)
    retried = [b for b in range(SP.BATCH) if not np.array_equal(r["K"][b], r5["K"][b])]
    assert retried == list(RETRY_ROBOTS), retried  # (the oracle retries for exactly those two)
    g = _gpu_rows_solve(prob, opts, sets)
    for f in TC.DECISIONS:
        assert np.array_equal(g[f], r[f]), (f, g[f], r[f])
    for f in TC.ARRAYS + TC.SCALARS:
        e, tol = TC.rel(g[f], r[f]), max(1e-9, 10 * TC.rel(r2[f], r[f]))
        print(f"retries {f}: rel {e:.3e} (bound {tol:.3e})")
        assert e < tol, (f, e, tol)
    g5 = _gpu_rows_solve(prob, other, sets)
    assert [b for b in range(SP.BATCH) if not np.array_equal(g["K"][b], g5["K"][b])] == list(RETRY_ROBOTS)
    monkeypatch.setenv("HSDDP_SEQUENTIAL_RETRY", "1")
    q = _gpu_rows_solve(prob, opts, sets)
    for f in TC.ARRAYS + TC.SCALARS + TC.DECISIONS:
        assert np.array_equal(g[f], q[f]), f


# ---- 6. against the oracle's knot costs -------------------------------------------------------------
def _knot_cost(prob, b, W, weights, opts):
    """the sum of oracle_lib.knot_eval's running costs over robot b's knots and terminal costs over its
    phase ends at the rows W, under `weights` (no AL / ReB terms: opts turns them off)"""
    import oracle_lib as O
    hz = TC.phases_of(prob)[b]
    rb = 0 if prob["ref_x"].shape[0] == 1 else b
    o = O.default_options(**opts)
    kw = dict(options=o, dt=prob["dt"], weights=weights, cparams=SP.oracle_cparams())
    z, tot, s, kc = np.zeros(24), 0.0, 0, 0
    for i, n in enumerate(hz):
        c, cn = prob["contacts"][b, i], prob["contacts"][b, i + 1]
        for k in range(n):
            tot += float(O.knot_eval(c, cn, W["X"][b, s + k], W["U"][b, kc], prob["ref_x"][rb, s + k], prob["ref_u"][rb, s + k],
                                     prob["ref_foot"][rb, s + k], **kw)["l"])
            kc += 1
        tot += float(O.knot_eval(c, cn, z, z, z, z, np.zeros(12), W["X"][b, s + n], prob["ref_x"][rb, s + n],
                                 prob["ref_foot"][rb, s + n], **kw)["Phi"])
        s += n + 1
    return tot


@pytest.mark.parametrize("when", ["before_begin", "after_begin"])
def test_new_rows_on_a_warm_handle_against_oracle_knot_costs(when):
    """Solve, give robots 1 and 3 new rows, begin(); iterate(1) with a line search that rejects every
    trial (gamma = 1e6), so the element's cost stays the one the iteration started from: for robots 1
    and 3 it equals the sum of the oracle's knot and terminal costs of the working rows downloaded
    after begin() under the new rows at 1e-12 relative, and misses it under the old weights.  The
    costs are formed by begin()'s rollout (rows set before it) or by k_lq's SLOTS instantiation
    (rows set after it: the call clears slots_fresh).  AL and ReB are off: the cost is the weights'.
    The untouched robots' cost is the old weights' sum."""
    prob = TC.shared_problem()
    opts = {"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 2, "AL_active": 0, "ReB_active": 0}
    rej = {**opts, "alpha": 0.5, "gamma": 1e6}
    sets = [dict(SP.WEIGHTS) for _ in range(5)]
    sets[1], sets[3] = EW.weight_set(1), EW.weight_set(3)
    mask = np.array([0, 1, 0, 1, 0], np.int32)
    s = EW.gpu_solver(prob, opts)
    s.solve()
    s.set_options(hsddp.load_settings(**rej))
    if when == "before_begin":
        s.set_element_weights(EW.rows(sets), mask)
    s.begin()
    W = s.working()
    if when == "after_begin":
        s.set_element_weights(EW.rows(sets), mask)
    s.iterate(1)
    info = s.element_info()
    s.close()
    assert np.all(info["n_ls_trials"] >= 1)
    for b in range(5):
        new, old = _knot_cost(prob, b, W, sets[b], rej), _knot_cost(prob, b, W, SP.WEIGHTS, rej)
        e_new, e_old = abs(info["cost"][b] - new) / abs(new), abs(info["cost"][b] - old) / abs(old)
        print(f"{when} robot {b}: cost {info['cost'][b]:.17g}, oracle new {new:.17g} (rel {e_new:.3e}), old {old:.17g} (rel {e_old:.3e})")
        assert e_new < 1e-12, (b, e_new)
        if mask[b]:
            assert e_old > 1e-12, ("the old weights pass", b, e_old)


# ---- 7. through the MPC steps -----------------------------------------------------------------------
def test_rows_stay_with_the_robots_through_the_mpc_steps():
    """Five ticks of advance -> update_problem -> solve on robots with their own reference windows, a
    restart_elements of robot 1 in the third: element_weights() reads back unchanged after every call
    (a restarted robot keeps its row), and every robot equals, bit for bit, a B = 1 handle created with
    its row and driven through the same calls."""
    import restart_case as RC
    tab, dt, n_trot = RC.table()
    starts = [0, 7, n_trot + 3, 12]
    B = len(starts)
    x = RC.x0(B, 40)
    sets = EW.robot_sets(B)

    def make(idx, weights):
        p = hsddp.reference_problem(tab, dt, [starts[b] for b in idx], x[idx], plan_duration=RC.PLAN)
        return hsddp.Solver(p, hsddp.load_settings(**RC.TICK), weights=SP.hsddp_weights(weights))

    s = make(list(range(B)), None)
    ones = [make([b], sets[b]) for b in range(B)]
    rows = EW.rows(sets)
    s.set_element_weights(rows)
    want = [EW.as_bytes(w) for w in rows]
    for h in [s] + ones:
        h.solve()
    for it in range(5):
        xt = RC.x0(B, 50 + it)
        for h, idx in [(s, list(range(B)))] + [(ones[b], [b]) for b in range(B)]:
            h.advance(None, 1, RC.PLAN)
            if it == 2:
                mask = np.array([1 if b == 1 else 0 for b in idx], np.int32)
                h.restart_elements(mask, np.array([starts[b] + 20 for b in idx], np.int32), None, RC.PLAN)
            if h is s:
                assert [EW.as_bytes(w) for w in s.element_weights()] == want, it
            h.update_problem(None, xt[idx])
            h.solve()
        snap = RC.snapshot(s)
        for b in range(B):
            RC.same_element(snap, RC.snapshot(ones[b]), b, 0)
        assert [EW.as_bytes(w) for w in s.element_weights()] == want, it
    for h in [s] + ones:
        h.close()


# ---- 8. simulate_policy -----------------------------------------------------------------------------
def test_simulate_policy_costs_under_each_robots_row():
    """k_simulate_policy with rows, as the first consumer of a changed table: after a solve, robots 0
    and 2 get new rows and hsddp_simulate_policy runs at once.  Each robot's rollouts, per-sample costs
    and summaries equal test_gpu_simulate.py's helper (tests/sim_reference.py) evaluated with that
    robot's weights, at that file's tolerance; robot 2's costs miss the helper's under robot 0's row."""
    import sim_reference as R
    import test_gpu_simulate as TS
    from hsddp import synthetic as syn
    prob = syn.make_batch(3, 3, 4, "trot")
    first = [EW.weight_set(4), EW.weight_set(1), EW.weight_set(2)]
    sets = [EW.weight_set(0), EW.weight_set(1), EW.weight_set(3)]
    s = hsddp.Solver(prob, hsddp.load_settings(**TS.FIXED), weights=SP.hsddp_weights())
    s.set_element_weights(EW.rows(first))
    s.solve()
    tr = s.trajectory()
    assert np.any(tr["K"] != 0)
    x = TS.perturbed(tr["Xbar"][:, 0], 70, seed=23)
    s.set_element_weights(EW.rows(sets), np.array([1, 0, 1], np.int32))
    n = 12
    g = TS.flat(s.simulate_policy(x, n, trajectories=True))
    s.close()
    refs = [(R.simulate(prob, tr, x, n, weights=sets[b]), R.simulate(prob, tr, x * (1 + 1e-15), n, weights=sets[b])) for b in range(3)]
    for b in range(3):
        ref, ref2 = (R.prefix(q, n) for q in refs[b])
        assert np.all(ref["status"][b] == 0)
        assert np.array_equal(g["steps"][b], ref["steps"][b]) and np.array_equal(g["status"][b], ref["status"][b]), b
        for f in TS.FIELDS:
            e, tol = TS.rel(g[f][b], ref[f][b]), max(1e-9, 10 * TS.rel(ref2[f][b], ref[f][b]))
            print(f"simulate robot {b} {f}: rel {e:.3e} (bound {tol:.3e})")
            assert e < tol, (b, f, e, tol)
    wrong = R.prefix(refs[0][0], n)
    assert TS.rel(g["cost"][2], wrong["cost"][2]) > 1e-6


# ---- the running cost's rounding, pinned -------------------------------------------------------------
def test_slot_costs_do_not_depend_on_the_kernel_variant(monkeypatch):
    """cost_combine forms dt lt + dt lf as fma(lt, dt, lf dt) in every kernel (left to the compiler's
    contraction, the instantiations disagreed by an ulp): on a handle without a table the slot costs
    the fused-decide rollout stores (B <= 16) equal the plain rollout's (HSDDP_NO_FUSED_DECIDE=1) bit
    for bit, as does everything else the solve leaves; and the [B][46] array form of the setter gives
    the rows the structure form gives."""
    prob = TC.shared_problem()
    outs = []
    for fused in (True, False):
        if not fused:
            monkeypatch.setenv("HSDDP_NO_FUSED_DECIDE", "1")
        s = EW.gpu_solver(prob, FIXED)
        s.solve()
        outs.append(TC.downloads(s))
        s.close()
    _same(outs[0], outs[1], "fused against plain rollout")
    monkeypatch.delenv("HSDDP_NO_FUSED_DECIDE")
    rows = EW.rows(EW.robot_sets(5))
    arr = np.array([np.frombuffer(EW.as_bytes(w), np.float64) for w in rows])
    packed = (hsddp.Weights * 5)(*rows)
    got = []
    for form in (rows, arr, packed):
        s = EW.gpu_solver(prob, FIXED)
        s.set_element_weights(form)
        got.append([EW.as_bytes(w) for w in s.element_weights()])
        s.close()
    assert got[0] == got[1] == got[2] == [EW.as_bytes(w) for w in rows]
