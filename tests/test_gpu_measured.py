"""x0 formed on the device from the robots' measured states (hsddp_hkd_state,
hsddp_update_problem_measured, hsddp_extract_commands_measured).

The expected x0 is a numpy restatement of HKDMPC.cpp:119-129 whose foot positions come from
hsddp.model.foot_position — the route a caller had to take before — so every comparison is bit
for bit: the primitive against the restatement, and a solver fed the records against a twin fed
the host-formed x0 (same contacts, references and fixed iteration budget).
"""
import os

import numpy as np
import pytest

import hsddp
from hsddp import model, shard
from hsddp import synthetic as syn

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXED = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=2)  # two inner iterations, no early exit
TICK = dict(max_AL_iter=2, max_DDP_iter=1)
ERR_ARG = "hsddp error -1"


def records(n, seed):
    """[n] ROBOT_STATE near the nominal stance, all float32"""
    rng = np.random.default_rng(seed)
    u = lambda *shape: rng.uniform(-1.0, 1.0, shape)  # noqa: E731
    r = np.zeros(n, dtype=hsddp.ROBOT_STATE)
    r["p"] = np.array([0.0, 0.0, 0.25]) + u(n, 3) * np.array([0.05, 0.05, 0.02])
    rpy = 0.1 * u(n, 3)
    rpy[np.abs(rpy[:, 0] - rpy[:, 2]) < 1e-3, 2] += 0.01  # yaw and roll distinct: a swap shows
    r["rpy"] = rpy
    r["omegaBody"] = 0.3 * u(n, 3)
    r["vWorld"] = 0.3 * u(n, 3)
    r["qJ"] = np.tile([0.0, -0.8, 1.6], 4) + 0.1 * u(n, 12)
    r["foot_placements"] = 0.3 * u(n, 12)
    return r


def expected_x0(rec, c0):
    """x0 [n][24] of HKDMPC.cpp:119-129 with T = double; c0 [n][4] the first phase's contact"""
    n = rec.shape[0]
    x = np.zeros((n, 24))
    x[:, 0:3] = rec["rpy"][:, ::-1]
    x[:, 3:6] = rec["p"]
    x[:, 6:9] = rec["omegaBody"]
    x[:, 9:12] = rec["vWorld"]
    x[:, 12:24] = rec["qJ"]
    rows = x.copy()  # (the joint angles of every leg still in place)
    for l in range(4):
        fp = model.foot_position(rows, l)
        on = np.asarray(c0)[:, l] != 0
        x[on, 12 + 3 * l:15 + 3 * l] = fp[on]
    return x


def state_of(s):
    return {**s.trajectory(), **s.working(), **s.element_info(), **s.constraint_values()}


def assert_same(a, b, what):
    for f in a:
        assert np.array_equal(a[f], b[f], equal_nan=True), (what, f)


# ---- 1. the primitive -----------------------------------------------------------------------------
# the six patterns the first records have always cycled through, then the other ten of the 16 masks
PATTERNS = np.array([[1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 0, 1], [0, 1, 1, 0], [1, 0, 0, 0], [0, 0, 1, 0],
                     [0, 1, 0, 0], [0, 0, 0, 1], [1, 1, 0, 0], [0, 0, 1, 1], [1, 0, 1, 0], [0, 1, 0, 1],
                     [0, 1, 1, 1], [1, 0, 1, 1], [1, 1, 0, 1], [1, 1, 1, 0]], np.int32)
assert len({tuple(r) for r in PATTERNS}) == 16


@pytest.mark.parametrize("n", [1, 5, 67])
def test_primitive_equals_the_restatement(n):
    rec = records(n, 10 + n)
    c = PATTERNS[np.arange(n) % len(PATTERNS)]
    x = model.hkd_state(rec, c)
    assert x.shape == (n, 24) and x.dtype == np.float64
    assert np.array_equal(x, expected_x0(rec, c))
    assert np.array_equal(x[:, 0], rec["rpy"][:, 2].astype(np.float64))  # eul = (yaw, pitch, roll)
    assert np.array_equal(x[:, 2], rec["rpy"][:, 0].astype(np.float64))
    q = x[:, 12:].reshape(n, 4, 3)
    swing = c == 0
    assert np.array_equal(q[swing], rec["qJ"].reshape(n, 4, 3).astype(np.float64)[swing])
    if n > 1:
        assert np.all(np.any(q[~swing] != rec["qJ"].reshape(n, 4, 3).astype(np.float64)[~swing], axis=-1))


# ---- 2. a shared layout with per-element contacts -------------------------------------------------
def _tick_inputs(contacts, hzs, t0):
    """references of each element's layout (hzs[b]) at window start t0, strided by the largest"""
    B = contacts.shape[0]
    S = max(sum(n + 1 for n in hz) for hz in hzs)
    rx = np.zeros((B, S, 24)); ru = np.zeros((B, S, 24)); rf = np.zeros((B, S, 12))
    for b, hz in enumerate(hzs):
        x, u, f = syn._reference_slots([tuple(r) for r in contacts[b, :len(hz) + 1]], hz, syn.DT, t0)
        rx[b, :x.shape[0]], ru[b, :x.shape[0]], rf[b, :x.shape[0]] = x, u, f
    return rx, ru, rf


def test_shared_layout_equals_host_x0():
    B = 5
    prob = syn.make_batch(B, 4, 3, mixed=True)
    contacts = prob["contacts"].copy()
    assert len({tuple(r) for r in contacts[:, 0]}) > 1  # row 0 differs between elements
    opt = hsddp.load_settings(**FIXED)
    a, m = hsddp.Solver(prob, opt), hsddp.Solver(prob, opt)
    a.solve(); m.solve()
    for tick in range(1, 4):
        la, lm = a.shift([0]), m.shift([0])
        assert la == lm
        hz = la["horizons"]
        if len(hz) + 1 < contacts.shape[1]:  # the first phase left: its contact row goes
            contacts = np.ascontiguousarray(contacts[:, 1:])
        rx, ru, rf = _tick_inputs(contacts, [hz] * B, tick)
        rec = records(B, 20 + tick)
        a.update_problem(contacts, expected_x0(rec, contacts[:, 0]), rx, ru, rf)
        m.update_problem_measured(rec, contacts, rx, ru, rf)
        a.solve(); m.solve()
        assert_same(state_of(a), state_of(m), tick)
    assert len(hz) == 3  # the ticks crossed a layout change
    a.close(); m.close()


# ---- 3. per-element layouts: the contact stride is Pmax + 1 ---------------------------------------
def test_per_element_layouts_equal_host_x0():
    lays = [("trot", 4, 3), ("bound", 2, 6), ("pace", 4, 3), ("pronk", 2, 6), ("trot", 4, 3)]
    B = len(lays)
    prob = syn.make_layout_batch(lays)
    opt = hsddp.load_settings(**FIXED)
    a, m = hsddp.Solver(prob, opt), hsddp.Solver(prob, opt)
    a.solve(); m.solve()
    la, lm = a.shift([0]), m.shift([0])
    assert la["horizons"] == lm["horizons"] and len({len(h) for h in la["horizons"]}) == 2
    contacts = prob["contacts"]
    assert contacts.shape[1] == 5
    rx, ru, rf = _tick_inputs(contacts, la["horizons"], 1)
    rec = records(B, 31)
    a.update_problem(contacts, expected_x0(rec, contacts[:, 0]), rx, ru, rf)
    m.update_problem_measured(rec, contacts, rx, ru, rf)
    a.solve(); m.solve()
    assert_same(state_of(a), state_of(m), "layouts")
    a.close(); m.close()


# ---- 4, 5. device-resident records; the commands --------------------------------------------------
@pytest.fixture(scope="module")
def solved_pair():
    """two solvers on one problem with one solve behind them.  Two phases: only the legs that swing
    in phase 0 touch down inside the command's search, so the others keep the records' feet."""
    B = 5
    prob = syn.make_batch(B, 2, 6, mixed=True)
    opt = hsddp.load_settings(**FIXED)
    a, m = hsddp.Solver(prob, opt), hsddp.Solver(prob, opt)
    a.solve(); m.solve()
    yield prob, a, m
    a.close(); m.close()


def _keeps_some_feet(cmd, rec):
    same = cmd["foot_placement"] == rec["foot_placements"]
    return bool(np.any(np.all(same.reshape(-1, 4, 3), axis=-1))) and not bool(np.all(same))


def test_device_records_equal_host_records(solved_pair):
    prob, a, m = solved_pair
    B = prob["batch"]
    rec = records(B, 41)
    dur = np.random.default_rng(42).uniform(0.0, 0.3, (B, a.P, 4))
    dev = model._Dev(rec.nbytes).put(rec)
    refs = (prob["ref_x"], prob["ref_u"], prob["ref_foot"])
    a.update_problem_measured(rec, None, *refs)  # (contacts NULL: the handle's own)
    m.update_problem_measured(None, None, *refs, device_ptr=dev.ptr)
    dev.put(np.zeros_like(rec))  # the handle holds its own copy of the feet
    a.solve(); m.solve()
    assert_same(state_of(a), state_of(m), "device records")
    ca = a.extract_commands_measured(1, 0.02, 0.01, dur, 0.5)
    cm = m.extract_commands_measured(1, 0.02, 0.01, dur, 0.5)
    assert np.array_equal(shard.command_bytes(ca), shard.command_bytes(cm))
    assert _keeps_some_feet(cm, rec)  # (the records' feet, not the zeroed buffer's)


def test_commands_equal_the_host_fed_extraction(solved_pair):
    prob, a, m = solved_pair
    B = prob["batch"]
    rec = records(B, 51)
    dur = np.random.default_rng(52).uniform(0.0, 0.3, (B, a.P, 4))
    feet = np.ascontiguousarray(rec["foot_placements"])
    m.update_problem_measured(rec, None, prob["ref_x"], prob["ref_u"], prob["ref_foot"])
    m.solve()
    got = m.extract_commands_measured(1, 0.03, 0.01, dur, 0.25)
    want = m.extract_commands(1, 0.03, 0.01, dur, feet, 0.25)
    assert np.array_equal(shard.command_bytes(got), shard.command_bytes(want))
    assert _keeps_some_feet(got, rec)
    # into device memory: the same bytes as hsddp_extract_commands_device given D and the feet
    nbytes = B * hsddp.MPC_COMMAND.itemsize
    mine = model._Dev(nbytes).put(np.full(nbytes, 0xAB, np.uint8))
    theirs = model._Dev(nbytes).put(np.full(nbytes, 0x11, np.uint8))
    assert m.extract_commands_measured(1, 0.03, 0.01, dur, 0.25, out_ptr=mine.ptr) is None
    hsddp._lib.check(hsddp._lib.lib().hsddp_extract_commands_device(
        m._h, 1, 0.03, 0.01, dur.ctypes.data, 1, feet.ctypes.data, 1, 0.25, theirs.ptr))
    out = mine.get((nbytes,), np.uint8)
    assert np.array_equal(out, theirs.get((nbytes,), np.uint8))
    assert np.array_equal(out, shard.command_bytes(got))


# ---- 6. the reference-table path ------------------------------------------------------------------
def test_reference_table_ticks_equal_the_host_route():
    B = 3
    a, m = _table_solver(B), _table_solver(B)
    a.solve(); m.solve()
    first = a.phase_info()["contacts"][:, 0].copy()
    changed = False
    for it in range(30):
        rec = records(B, 60 + it)
        fa, fm = a.advance(None), m.advance(None)
        assert fa == fm
        info = a.phase_info()
        a.update_problem(None, expected_x0(rec, info["contacts"][:, 0]))
        m.update_problem_measured(rec)
        a.solve(); m.solve()
        sa, sm = state_of(a), state_of(m)
        for f in ("Xbar", "Ubar", "K", "cost", "feas", "merit", "max_tconstr", "max_pconstr", "iters", "outer_iters",
                  "status", "n_ls_trials"):
            assert np.array_equal(sa[f], sm[f], equal_nan=True), (it, f)
        ca = a.extract_commands(1, 0.01 * it, 0.01, info["durations"], rec["foot_placements"], 0.5)
        cm = m.extract_commands_measured(1, 0.01 * it, 0.01, None, 0.5)  # the handle's own durations
        assert np.array_equal(shard.command_bytes(ca), shard.command_bytes(cm)), it
        changed = changed or not np.array_equal(info["contacts"][:, 0], first)
        if changed and it >= 2:
            break
    assert changed  # the first phase's contact changed: x0's stance legs did too
    a.close(); m.close()


# ---- 7. state rules -------------------------------------------------------------------------------
def _error_of(call):
    with pytest.raises(hsddp.HSDDPError) as e:
        call()
    return str(e.value)


def _table_solver(B):
    tab, dt = hsddp.load_quad_reference(os.path.join(GOLD, "ref_trot.csv"))
    x0 = np.zeros((B, 24))
    x0[:, 5] = 0.25
    x0[:, 12:] = np.float32([.2, -.14, 0, .2, .14, 0, -.2, -.14, 0, -.2, .14, 0])
    return hsddp.Solver(hsddp.reference_problem(tab, dt, [0], x0), hsddp.load_settings(**TICK))


def test_state_rules():
    B = 4
    prob = syn.make_batch(B, 3, 4, mixed=True)
    refs = (prob["ref_x"], prob["ref_u"], prob["ref_foot"])
    opt = hsddp.load_settings(**FIXED)
    a, m = hsddp.Solver(prob, opt), hsddp.Solver(prob, opt)
    rec = records(B, 71)
    L = hsddp._lib.lib()
    # no measured update yet
    assert ERR_ARG in _error_of(lambda: m.extract_commands_measured())
    # argument errors, each with the message hsddp_update_problem gives where it refuses the same
    for r in ((refs[0], refs[1], None), (refs[0], None, None)):  # references: two, one of three
        want = _error_of(lambda: m.update_problem(prob["contacts"], prob["x0"], *r))
        got = _error_of(lambda: m.update_problem_measured(rec, prob["contacts"], *r))
        assert want == got and ERR_ARG in got
    assert ERR_ARG in _error_of(lambda: m.update_problem_measured(None))  # no records, no device_ptr
    assert L.hsddp_update_problem_measured(m._h, None, rec.ctypes.data, 2, None, None, None) == -1
    # nothing was launched: the twin that never saw the refused calls solves to the same bits
    a.solve(); m.solve()
    assert_same(state_of(a), state_of(m), "after refusals")
    # device_bytes grows by the record and feet buffers, once
    b0 = m.device_bytes()
    m.update_problem_measured(rec, prob["contacts"], *refs)
    b1 = m.device_bytes()
    assert b1 - b0 == B * 144 + B * 48
    m.update_problem_measured(rec, prob["contacts"], *refs)
    assert m.device_bytes() == b1
    assert m.extract_commands_measured().shape == (B,)
    # a host-formed x0 afterwards: no measured record belongs to this tick
    m.update_problem(prob["contacts"], prob["x0"], *refs)
    assert ERR_ARG in _error_of(lambda: m.extract_commands_measured())
    # NULL contacts with none derived (a shift leaves none of the new layout on the handle)
    m.solve()
    m.shift([0])
    want = _error_of(lambda: m.update_problem(None, prob["x0"], *refs))
    got = _error_of(lambda: m.update_problem_measured(rec, None, *refs))
    assert want == got and ERR_ARG in got and "contacts" in got
    # no problem uploaded (a layout just set), as hsddp_update_problem refuses
    assert L.hsddp_set_layout(a._h, 3, hsddp._lib.ip(np.array([4, 4, 4], np.int32)), None, None) == 0
    want = _error_of(lambda: a.update_problem(prob["contacts"], prob["x0"], *refs))
    got = _error_of(lambda: a.update_problem_measured(rec, prob["contacts"], *refs))
    assert want == got and ERR_ARG in got
    a.close(); m.close()


def test_simulated_update_clears_the_held_feet():
    B = 3
    t = _table_solver(B)
    t.solve()
    t.advance(None, 1)
    t.update_problem_measured(records(B, 72))
    t.solve()
    assert t.extract_commands_measured().shape == (B,)
    t.simulate_policy(None, 1)
    t.advance(None, 1)
    t.update_problem_simulated(0)
    assert ERR_ARG in _error_of(lambda: t.extract_commands_measured())
    t.close()
