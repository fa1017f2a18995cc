"""GPU checks of hsddp_copy_elements, hsddp_export_elements and hsddp_import_elements: a robot moved
between live batches cannot tell.

Elements are independent of batch, slot and sweep pair in this solver (the restart, split and
pairing tests rely on it), so a moved element equals its original bit for bit — in every field a
caller can read (tests/restart_case.py: snapshot / same_element, whatever the two handles' strides)
and over the MPC ticks that follow, given the same x0 — and every other element of the destination
equals a twin handle that never received anything.  No comparison here has a tolerance.

Batches: tests/restart_case.py's (Kc = 20 on the trot and flytrot files, at most six robots on
different windows, the tick budget TICK).  The layouts the cases rely on (which element has two or
three phases after how many ticks) are asserted where they matter."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import hsddp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import restart_case as RC  # noqa: E402

pytestmark = pytest.mark.gpu

T = 130  # samples of the trot file: flytrot's sample k is table sample T + k
SRC = [0, 3, T + 0, T + 6, 12, T + 12]  # after three ticks: elements 1 and 4 have two phases, 2 and 5 three
DST = [1, T + 14, 20, T + 21]           # after two ticks: elements 1 and 2 have three phases, 0 and 3 two


def _codes():
    hdr = open(os.path.join(os.path.dirname(HERE), "include", "hsddp.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(HSDDP_(?:OK|ERR_[A-Z]+))\s*=\s*(-?\d+)", hdr)}


_TAB = []


def _table():
    if not _TAB:
        _TAB.append(RC.table())
    return _TAB[0]


def _live(starts, ticks, seed, fp32=False, ms=1, copies=1):
    """`copies` equal handles of the batch at `starts` after a solve and `ticks` MPC ticks"""
    tab, dt, n_trot = _table()
    assert n_trot == T
    B = len(starts)
    out = [RC.solver(tab, dt, starts, RC.x0(B, seed), fp32, **dict(RC.TICK, MS=ms)) for _ in range(copies)]
    for s in out:
        s.solve()
        for it in range(ticks):
            s.advance(RC.x0(B, seed + 1 + it), 1, RC.PLAN)
            s.solve()
    return out


def _tick(s, x):
    s.advance(x, 1, RC.PLAN)
    s.solve()


def _phases(snap, b):
    return len(snap["horizons"][b])


def _assert_unchanged(before, after, elems=None):
    B = len(before["horizons"])
    for b in (range(B) if elems is None else elems):
        RC.same_element(after, before, b)
    if elems is None:
        assert (after["_P"], after["_S"]) == (before["_P"], before["_S"])


def _follow(dst, src, twin, moved, kept, ticks, seed):
    """`ticks` more ticks on the three handles, each robot given the same x0 wherever it lives: the
    moved robots (dst slot -> src element) equal their originals and the kept ones the twin's"""
    for it in range(ticks):
        xs = RC.x0(src.B, seed + it)
        xd = RC.x0(dst.B, seed + 50 + it)
        for d, s in moved.items():
            xd[d] = xs[s]
        _tick(src, xs)
        _tick(dst, xd)
        if twin is not None:
            _tick(twin, xd)
        a, b = RC.snapshot(dst), RC.snapshot(src)
        for d, s in moved.items():
            RC.same_element(a, b, d, s)
        if twin is not None:
            t = RC.snapshot(twin)
            for e in kept:
                RC.same_element(a, t, e)


def _copy_case(fp32=False, ms=1):
    src, = _live(SRC, 3, 100, fp32, ms)
    dst, twin = _live(DST, 2, 150, fp32, ms, copies=2)
    s0, d0 = RC.snapshot(src), RC.snapshot(dst)
    assert [_phases(s0, b) for b in range(6)] == [2, 2, 3, 2, 2, 3] and [_phases(d0, b) for b in range(4)] == [2, 3, 3, 2]
    dst.copy_elements(src, [0, 3], [1, 4])
    s1, d1 = RC.snapshot(src), RC.snapshot(dst)
    RC.same_element(d1, s0, 0, 1)
    RC.same_element(d1, s0, 3, 4)
    _assert_unchanged(d0, d1, [1, 2])
    _assert_unchanged(s0, s1)
    _follow(dst, src, twin, {0: 1, 3: 4}, [1, 2], 3, 300)
    for s in (src, dst, twin):
        s.close()


# ---- 1, 6: copy equals source, the rest is untouched; the modes ---------------------------------------
def test_copy_equals_source_and_leaves_the_rest():
    _copy_case()


def test_copy_fp32():
    _copy_case(fp32=True)


def test_copy_single_shooting():
    _copy_case(ms=0)


# ---- 2: same handle, overlapping -----------------------------------------------------------------------
def test_copy_within_one_handle_overlapping():
    A, C_ = _live(SRC, 3, 100, copies=2)
    a0 = RC.snapshot(A)
    A.copy_elements(A, [0, 1, 2], [2, 2, 0])
    a1 = RC.snapshot(A)
    RC.same_element(a1, a0, 0, 2)
    RC.same_element(a1, a0, 1, 2)
    RC.same_element(a1, a0, 2, 0)
    _assert_unchanged(a0, a1, [3, 4, 5])
    for it in range(2):
        xc = RC.x0(6, 300 + it)
        xa = xc.copy()
        xa[0], xa[1], xa[2] = xc[2], xc[2], xc[0]
        _tick(C_, xc)
        _tick(A, xa)
        a, c = RC.snapshot(A), RC.snapshot(C_)
        for d, s in ((0, 2), (1, 2), (2, 0), (3, 3), (4, 4), (5, 5)):
            RC.same_element(a, c, d, s)
    A.close(); C_.close()


# ---- 3: strides ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["up", "down"])
def test_copy_changes_the_strides(case):
    """up: the moved robot has more phases than any in dst; down: the robot holding dst's largest P
    is overwritten by one with fewer.  Every other robot's rows are intact at the new strides, and
    the next tick equals the twin."""
    src, = _live(SRC, 3, 100)
    starts = [0, 1, T + 6, T + 21] if case == "up" else [0, T + 14, T + 6, T + 21]
    dst, twin = _live(starts, 2, 150, copies=2)
    s0, d0 = RC.snapshot(src), RC.snapshot(dst)
    slot, elem, P0, P1 = (2, 2, 2, 3) if case == "up" else (1, 1, 3, 2)
    assert d0["_P"] == P0 and _phases(s0, elem) == P1
    assert all(_phases(d0, b) == 2 for b in range(4) if b != slot) and _phases(d0, slot) == P0
    dst.copy_elements(src, [slot], [elem])
    d1 = RC.snapshot(dst)
    assert d1["_P"] == P1 and dst.P == P1
    RC.same_element(d1, s0, slot, elem)
    kept = [b for b in range(4) if b != slot]
    _assert_unchanged(d0, d1, kept)
    _assert_unchanged(s0, RC.snapshot(src))
    _follow(dst, src, twin, {slot: elem}, kept, 2, 300)
    for s in (src, dst, twin):
        s.close()


# ---- 4: shared to per-element layouts and back ---------------------------------------------------------
def test_shared_layout_to_per_element_and_back():
    src, = _live(SRC, 3, 100)
    dst, twin = _live([1, 1, 1, 1], 2, 150, copies=2)
    s0, d0 = RC.snapshot(src), RC.snapshot(dst)
    assert dst.layout()["horizons"] == list(d0["horizons"][0])  # the shared layout
    assert list(s0["horizons"][1]) != list(d0["horizons"][0])
    dst.copy_elements(src, [2], [1])
    with pytest.raises(hsddp.HSDDPError):  # per-element layouts: hsddp_get_layout refuses
        dst.layout()
    d1 = RC.snapshot(dst)
    RC.same_element(d1, s0, 2, 1)
    _assert_unchanged(d0, d1, [0, 1, 3])
    _follow(dst, src, twin, {2: 1}, [0, 1, 3], 1, 300)
    # every slot replaced by robots of one layout: the shared layout again
    s1 = RC.snapshot(src)
    dst.copy_elements(src, [0, 1, 2, 3], [4, 4, 4, 4])
    assert dst.layout()["horizons"] == list(s1["horizons"][4])
    d2 = RC.snapshot(dst)
    for b in range(4):
        RC.same_element(d2, s1, b, 4)
    _follow(dst, src, None, {b: 4 for b in range(4)}, [], 2, 400)
    for s in (src, dst, twin):
        s.close()


# ---- 5: after a diverged tick --------------------------------------------------------------------------
def test_copy_after_a_diverged_tick():
    """the source's element 1 broke the rollout's bound from the initial rollout on (its warm start
    translated along tests/divergence_case.py's direction): its stored constraint values (cf_u /
    cf_flag, TD_STALE, ovr) and working rows are those of a broken solve"""
    import divergence_case as DC
    src, = _live(SRC, 2, 100)
    src.advance(None, 1, RC.PLAN)
    src.update_problem(None, RC.x0(6, 103))
    lay, info, tr = src.element_layouts(), src.phase_info(), src.trajectory()
    e = DC.direction_of(info["contacts"][1], lay["horizons"][1])
    tr["Xbar"][1, :len(e)] += 2e6 * e
    src.warm_start(tr["Xbar"], tr["Ubar"], tr["K"])
    src.solve()
    ei = src.element_info()
    trials, eps = 0, 1.0
    while eps > 1e-3:
        trials, eps = trials + 1, eps * src.options.alpha
    assert ei["status"][1] != 0 or ei["n_ls_trials"][1] == ei["iters"][1] * trials, (ei["status"], ei["n_ls_trials"])
    dst, twin = _live(DST, 2, 150, copies=2)
    s0 = RC.snapshot(src)
    dst.copy_elements(src, [0], [1])
    d1 = RC.snapshot(dst)
    cd, cs = dst.constraint_values(), src.constraint_values()
    P = _phases(s0, 1)
    assert np.array_equal(cd["grf_g"][0], cs["grf_g"][1], equal_nan=True)
    assert np.array_equal(cd["td_h"][0][:P], cs["td_h"][1][:P], equal_nan=True)
    RC.same_element(d1, s0, 0, 1)
    _follow(dst, src, twin, {0: 1}, [1, 2, 3], 2, 300)
    for s in (src, dst, twin):
        s.close()


# ---- 7: export and import ------------------------------------------------------------------------------
def test_export_then_import_into_the_same_slots_changes_nothing():
    A, C_ = _live(SRC, 3, 100, copies=2)
    a0 = RC.snapshot(A)
    rec = A.export_elements([1, 4, 2])
    assert rec.dtype == np.uint8 and rec.size == 3 * hsddp.lib().hsddp_element_record_bytes(A._h)
    _assert_unchanged(a0, RC.snapshot(A))
    A.import_elements([1, 4, 2], rec)
    _assert_unchanged(a0, RC.snapshot(A))
    x = RC.x0(6, 300)
    _tick(A, x)
    _tick(C_, x)
    _assert_unchanged(RC.snapshot(C_), RC.snapshot(A))
    A.close(); C_.close()


def test_import_into_a_new_handle_equals_copy():
    tab, dt, _ = _table()
    src, = _live(SRC, 3, 100)
    s0 = RC.snapshot(src)
    N1, N2 = (RC.solver(tab, dt, [40, T + 40], RC.x0(2, 9), **RC.TICK) for _ in range(2))
    rec = src.export_elements([1, 2])
    assert len(rec.reshape(-1)) == 2 * src.element_record_bytes()
    N1.import_elements([1, 0], rec)   # record 0 (element 1) into slot 1, record 1 (element 2) into slot 0
    N2.copy_elements(src, [1, 0], [1, 2])
    a, b = RC.snapshot(N1), RC.snapshot(N2)
    for d, s in ((1, 1), (0, 2)):
        RC.same_element(a, s0, d, s)
        RC.same_element(a, b, d, d)
    for it in range(2):
        xs = RC.x0(6, 300 + it)
        xn = np.stack([xs[2], xs[1]])
        _tick(src, xs)
        _tick(N1, xn)
        _tick(N2, xn)
        a, b, s = RC.snapshot(N1), RC.snapshot(N2), RC.snapshot(src)
        for d, e in ((1, 1), (0, 2)):
            RC.same_element(a, s, d, e)
            RC.same_element(b, s, d, e)
    for h in (src, N1, N2):
        h.close()


# ---- 8: refusals leave both handles unchanged ----------------------------------------------------------
def _idx(*v):
    return np.array(v, np.int32)


def test_refusals_leave_both_handles_unchanged():
    from hsddp._lib import ip
    E = _codes()
    L = hsddp.lib()
    tab, dt, _ = _table()
    opts = hsddp.load_settings(**RC.TICK)
    src, = _live(SRC, 1, 100)
    dst, = _live(DST, 1, 150)
    s0, d0 = RC.snapshot(src), RC.snapshot(dst)

    def refused(code, d, s, di, si, what):
        rc = L.hsddp_copy_elements(d._h, s._h, len(di), ip(_idx(*di)), ip(_idx(*si)))
        assert rc == E[code], (what, rc, L.hsddp_last_error())

    def others():
        p = hsddp.reference_problem(tab, dt, SRC, RC.x0(6), plan_duration=0.3)
        assert p["Kc"] == 30
        yield "Kc", "HSDDP_ERR_ARG", hsddp.Solver(p, opts)
        p = hsddp.reference_problem(tab, dt, SRC, RC.x0(6), plan_duration=RC.PLAN)
        p["dt"] = 0.0125
        yield "dt", "HSDDP_ERR_ARG", hsddp.Solver(p, opts)
        w = hsddp._lib.Weights()
        L.hsddp_default_weights(C.byref(w))
        w.r_grf *= 2
        p = hsddp.reference_problem(tab, dt, SRC, RC.x0(6), plan_duration=RC.PLAN)
        yield "weights", "HSDDP_ERR_ARG", hsddp.Solver(p, opts, weights=w)
        yield "precision", "HSDDP_ERR_ARG", RC.solver(tab, dt, SRC, RC.x0(6), True, **RC.TICK)
        tab2 = tab.copy()
        tab2["grf"][T + 60, 2] += 1.0
        yield "tables", "HSDDP_ERR_UNSUPPORTED", RC.solver(tab2, dt, SRC, RC.x0(6), **RC.TICK)

    for what, code, X in others():  # as the source of a move into dst, and as its destination
        x0 = RC.snapshot(X)
        refused(code, dst, X, [0], [1], what)
        refused(code, X, src, [0], [1], what)
        _assert_unchanged(x0, RC.snapshot(X))
        X.close()
    S = RC.solver(tab, dt, [3], RC.x0(4), **RC.TICK)  # shared references
    S.solve()
    sh0 = RC.snapshot(S)
    refused("HSDDP_ERR_UNSUPPORTED", S, src, [0], [1], "shared-reference destination")
    sh1 = RC.snapshot(S)
    for b in range(4):
        RC.same_element(sh1, sh0, b, shared_refs=True)
    S.close()
    refused("HSDDP_ERR_ARG", dst, src, [1, 1], [0, 2], "duplicate destination")
    refused("HSDDP_ERR_ARG", dst, src, [4], [0], "destination out of range")
    refused("HSDDP_ERR_ARG", dst, src, [-1], [0], "destination out of range")
    refused("HSDDP_ERR_ARG", dst, src, [0], [6], "source out of range")
    refused("HSDDP_ERR_ARG", dst, dst, [0, 0], [1, 2], "duplicate destination, one handle")
    rec = src.export_elements([1])
    bad = rec.copy()
    bad[0, 0] ^= 0xFF  # the version word
    rc = L.hsddp_import_elements(dst._h, 1, ip(_idx(0)), bad.ctypes.data)
    assert rc == E["HSDDP_ERR_ARG"], (rc, L.hsddp_last_error())
    two = np.concatenate([rec, rec])
    rc = L.hsddp_import_elements(dst._h, 2, ip(_idx(0, 0)), two.ctypes.data)
    assert rc == E["HSDDP_ERR_ARG"], (rc, L.hsddp_last_error())
    # n = 0: nothing happens
    assert L.hsddp_copy_elements(dst._h, src._h, 0, None, None) == E["HSDDP_OK"]
    assert L.hsddp_export_elements(src._h, 0, None, None) == E["HSDDP_OK"]
    assert L.hsddp_import_elements(dst._h, 0, None, None) == E["HSDDP_OK"]
    _assert_unchanged(s0, RC.snapshot(src))
    _assert_unchanged(d0, RC.snapshot(dst))
    # a source (and a destination) awaiting its inputs after advance(x0 = None)
    W, V = _live(SRC, 1, 100, copies=2)
    W.advance(None, 1, RC.PLAN)
    refused("HSDDP_ERR_ARG", dst, W, [0], [1], "source awaiting inputs")
    refused("HSDDP_ERR_ARG", W, src, [0], [1], "destination awaiting inputs")
    rc = L.hsddp_export_elements(W._h, 1, ip(_idx(1)), rec.ctypes.data)
    assert rc == E["HSDDP_ERR_ARG"], (rc, L.hsddp_last_error())
    _assert_unchanged(d0, RC.snapshot(dst))
    _assert_unchanged(s0, RC.snapshot(src))
    x = RC.x0(6, 300)
    W.update_problem(None, x)
    W.solve()
    _tick(V, x)
    _assert_unchanged(RC.snapshot(V), RC.snapshot(W))
    for h in (src, dst, W, V):
        h.close()


# ---- handles whose references were uploaded, not built from a table ----------------------------------
def test_copy_between_handles_without_a_table():
    """the reference rows travel with the element (no table to rebuild them from): the moved element
    equals its original after the copy and after a further solve of both handles"""
    from hsddp import synthetic as syn

    def make(seed):
        p = syn.make_batch(4, 2, 10, "trot", seed=seed)
        for k in ("ref_x", "ref_u", "ref_foot"):
            p[k] = np.ascontiguousarray(np.repeat(p[k], 4, axis=0)) * (1.0 + 1e-3 * seed)
        s = hsddp.Solver(p, hsddp.load_settings(**RC.TICK))
        s.solve()
        return s

    def state(s):
        out = {**s.trajectory(), **s.working(), **s.element_info(), **s.constraint_params(), **s.constraint_values(),
               **s.references()}
        out.update({"hist_" + k: v for k, v in s.solver_info(16).items()})
        return out

    def same(a, b, ea, eb):
        bad = [f for f in a if not np.array_equal(a[f][ea], b[f][eb], equal_nan=True)]
        assert not bad, (ea, eb, bad)

    src, dst, twin = make(1), make(2), make(2)
    s0, d0 = state(src), state(dst)
    dst.copy_elements(src, [1], [2])
    d1 = state(dst)
    same(d1, s0, 1, 2)
    for b in (0, 2, 3):
        same(d1, d0, b, b)
    for h in (src, dst, twin):
        h.solve()
    d2, s2, t2 = state(dst), state(src), state(twin)
    same(d2, s2, 1, 2)
    for b in (0, 2, 3):
        same(d2, t2, b, b)
    for h in (src, dst, twin):
        h.close()
