"""Every element, at the batch sizes where the library changes kernels.

The solver picks its kernels by batch size (no HSDDP_* switch is set in this file: the library
chooses), and most choices scale with the device's CU count (256 on an MI355X; the sizes below are
computed from the count the device reports, so the edges stay edges on a partitioned device):

  trial decided in the rollout launch / in k_decide (fused_decide)            B <= 16 / 17
  terminal tasks appended to k_lq's launch / a launch of their own (launch_lq)  ceil(B P / 8) <= 256 / 257
  column-split sweep k_riccati_cs / the one-wave sweep (sweep_split)           pairs <= CUs / CUs + 1
  two element pairs per workgroup / one (sweep_wpb)                            pairs <= 4 CUs / 4 CUs + 1
  parallel regularisation retries / the in-kernel loop                          B >= 4 / 3; 128 deferred, the scratch cap
  last sweep pair half empty, last k_decide / k_rollout_ss wave partly filled  odd B, B mod 4 != 0
  a k_rollout slot wave spanning two elements                                   S not a multiple of 64

Each case: (1) a handful of base problems solved in a handle of their own and compared with the
oracle at the suite's bounds (test_gpu_parity.py: 1e-9 relative, or 10 x the oracle's own deviation
under a 1e-15 relative change of x0, with every decision equal; full solves 1e-7 past the chaos
screen); (2) a batch of B copies of them (tests/tiled_case.py: every base element at every residue
of b mod 4, in both halves of a sweep pair beside every other, and at B - 1); (3) every copy equal to
its base element bit for bit, in every record field (tiled_case.same; what it leaves out and why is
in that file's docstring).  An element's result does not depend on its batch, slot or sweep partner
(DESIGN.md §3.1), so step 3 has no tolerance.

Horizon of the edge cases: trot 4 x 16 (S = 68, Kc = 64) and jump 8 x 8 (S = 72, the same Kc).  k_rollout
takes its wide path from S >= 65 rows per wave (RW) and 4 x 16 is the smallest trot layout there
(4 x 15 has S = 64); neither S is a multiple of 64, so slot waves span two elements; Kc = 64 is a
multiple of 8, which jump's 8 phases need.  The thresholds depend on B and P, not on the horizon, and
these take about a second a case.  The retry case needs its elements' own horizon (8 x 25), and the
last two cases are the benchmark's configuration (trot 4 x 50).
"""
import functools
import subprocess
import sys
import time

import numpy as np
import pytest

import hsddp
import oracle_lib as O
import tiled_case as TC
from hsddp import synthetic as syn
from test_gpu_parity import _chaotic, _divergence, _stack, rel
from test_gpu_parity import _weights as _parity_weights

pytestmark = pytest.mark.gpu

FIXED = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=3)
TROT, JUMP = ("trot", 4, 16), ("jump", 8, 8)
TERM_TASKS_PER_BLOCK = 8   # 4 x TERM_TPW (hsddp_lq.hip: launch_lq)
TERM_MERGED_BLOCKS = 256   # ... whose threshold is a block count, not the CU count


def _torch(expr):
    """torch's answer from a fresh process with torch imported first: in this one libhsddp_amd.so has
    brought its own HIP runtime, beside which torch finds no device (tests/gpu_interop_check.py)"""
    r = subprocess.run([sys.executable, "-c", f"import torch; print(int({expr}))"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    return int(r.stdout.split()[-1])


@functools.lru_cache(None)
def cus():
    return _torch("torch.cuda.get_device_properties(0).multi_processor_count")


def size(spec):
    """(a, c) -> a CUs + c; an int is itself"""
    return spec if isinstance(spec, int) else spec[0] * cus() + spec[1]


def _noisy(prob, seed):
    """single shooting: x0 enters only through the first state's Defect, so the elements of one
    synthetic gait differ only by their warm start (tests/test_gpu_single_shooting.py: _batch)"""
    prob["Xbar"] = prob["Xbar"] + 0.01 * np.random.default_rng(seed).standard_normal(prob["Xbar"].shape)
    return prob


@functools.lru_cache(None)
def base_set(name):
    if name == "trot":      # one layout, a shared reference
        return syn.make_batch(5, 4, 16, "trot")
    if name == "trot_ss":
        return _noisy(syn.make_batch(5, 4, 16, "trot"), 5)
    if name == "pairs":     # per-element layouts: trot beside jump halves (n_pairs decides, not B)
        return syn.make_layout_batch([TROT, JUMP, TROT, JUMP, JUMP])
    if name == "pairs_ss":
        return _noisy(syn.make_layout_batch([TROT, JUMP, TROT, JUMP, JUMP]), 6)
    if name == "jump8":     # P = 8: the terminal-task edge away from the sweep's
        return syn.make_batch(5, 8, 8, "jump")
    if name == "mixed":     # per-element references, five gaits: 10 .. 32 iterations of a full solve
        return syn.make_batch(7, 4, 16, "trot", mixed=True)
    if name == "retry":     # test_gpu_parity.py::test_parallel_retry_equals_sequential's elements
        return _stack([377, 760, 656, 321, 0], 8, 25, "jump")
    if name in RETRY_WEIGHTS:  # test_retries_match_oracle's horizon (with the weights below)
        return syn.make_batch(5, 2, 10, "trot")
    if name == "metric":    # the benchmark's configuration
        return syn.make_batch(5, 4, 50, "trot")
    raise KeyError(name)


def _gpu(prob, opts, weights=None):
    s = hsddp.Solver(prob, hsddp.load_settings(**opts), weights=weights)
    s.solve()
    g = {**s.trajectory(), **s.working(), **s.element_info()}
    g["hist"] = s.solver_info()["cost"]
    snap = TC.snapshot(s)
    s.close()
    return g, snap


def _layout_parts(prob):
    """(elements, ordinary batch of them) per layout"""
    if prob.get("layouts") is None:
        return [(list(range(prob["batch"])), prob)]
    return [(el, syn.sub_batch(prob, el, hz)) for hz, el in syn.layout_groups(prob).items()]


def _oracle_fixed(prob, g, opts):
    """test_fixed_iterations_match_oracle's comparison (test_gpu_parity.py; single shooting:
    test_gpu_single_shooting.py's), per layout"""
    ss = opts.get("MS", 1) == 0
    for el, sub in _layout_parts(prob):
        S = sub["S"]
        r = O.solve_batch(sub, O.default_options(**opts), n_threads=8)
        p2 = dict(sub); p2["x0"] = sub["x0"] * (1 + 1e-15)
        r2 = O.solve_batch(p2, O.default_options(**opts), n_threads=8)
        for f in ("Xbar", "Ubar", "K", "X", "U", "dU") + (() if ss else ("dX",)):
            a = g[f][el, :S] if f in ("Xbar", "X", "dX") else g[f][el]
            assert rel(a, r[f]) < max(1e-9, 10 * rel(r2[f], r[f])), (f, rel(a, r[f]))
        for f in ("cost", "feas", "max_tconstr") + (("merit",) if ss else ()):
            assert rel(g[f][el], r[f]) < (max(1e-9, 10 * rel(r2[f], r[f])) if ss else 1e-9), f
        for f in ("iters", "outer_iters", "status", "n_ls_trials"):
            assert np.array_equal(g[f][el], r[f]), f
        if ss:
            assert np.all(g["dX"][el] == 0)


def _oracle_full(prob, g):
    """test_full_solve_matches_oracle's comparison (test_gpu_parity.py) with its chaos screen"""
    n = prob["batch"]
    r, chaotic, r2 = _chaotic(prob, {}, list(range(n)), perturbed=True)
    ok = [b for b in range(n) if b not in chaotic]
    assert len(ok) >= n - 1  # (measured on the oracle: none of this set is chaotic)
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f][ok], r[f][ok]), f
    for f in ("Xbar", "Ubar"):
        assert rel(g[f][ok], r[f][ok]) < 1e-7, f
    assert rel(g["cost"][ok], r["cost"][ok]) < 1e-9
    for b in sorted(chaotic):
        assert g["status"][b] == r["status"][b], b
        d = _divergence(r["solver_info"][b][:, 0], r2["solver_info"][b][:, 0])
        assert d >= 2 and _divergence(g["hist"][b], r["solver_info"][b][:, 0]) >= d, (b, d)
    return r


def _oracle_retry(prob, g, snap, opts):
    """The five jump elements are chaotic from the ninth iteration on (rounding differences of 1e-9 at
    iteration 2 are O(1) by then, on the oracle against itself as on the GPU:
    test_parallel_retry_equals_sequential), so what can be compared with the oracle is what
    test_full_solve_matches_oracle compares of a screened element: the cost history up to the entry
    where the oracle departs from its own perturbed run, and finite rows.

    They were chosen because their sweeps fail on the oracle in iterations 9-12 (element 760 exhausts
    the schedule there: asserted).  Measured on an MI355X, the GPU's rounding takes them elsewhere:
    in 12 iterations none of the five has a failed sweep (ElemState::reg stays 0 after every
    iteration, every status 0, trial counts 26 32 27 29 19 against the oracle's 24 30 27 29 19 with
    element 760 stopped at 11), and the first retry comes in iteration 16 (element 321, mu = 0.064).
    So this set keeps the large batch's equality on elements whose line searches run long and
    differently, and the retry paths are asserted to run on the two sets below (RETRY_WEIGHTS), whose
    sweeps fail by construction."""
    n = prob["batch"]
    r = O.solve_batch(prob, O.default_options(**opts), n_threads=8)
    p2 = dict(prob); p2["x0"] = prob["x0"] * (1 + 1e-15)
    r2 = O.solve_batch(p2, O.default_options(**opts), n_threads=8)
    assert np.any(r["status"] == 1)
    for b in range(n):
        assert np.all(np.isfinite(g["Xbar"][b])) and np.all(np.isfinite(g["Ubar"][b])), b
        d = _divergence(r["solver_info"][b][:, 0], r2["solver_info"][b][:, 0])
        assert d >= 2 and _divergence(g["hist"][b], r["solver_info"][b][:, 0]) >= d, (b, d)
    print("[retry] GPU reg", snap["el"]["reg"].tolist(), "status", snap["el"]["status"].tolist(), "trials",
          snap["el"]["n_ls"].tolist(), "oracle status", r["status"].tolist(), "trials", r["n_ls_trials"].tolist())


# Sweeps that fail by construction (test_gpu_parity.py: test_retries_match_oracle,
# test_regularization_overflow_status): r_qJd = -0.5 makes every element's first sweep of every
# iteration fail the PSD test until mu has made the joint-velocity diagonals positive; r_qJd = -1e5
# keeps Quu indefinite for every mu <= 1e2, so every element exhausts the schedule (status 1).
RETRY_WEIGHTS = {"retry_ok": -0.5, "retry_exhausted": -1e5}


def _weights(name):
    return _parity_weights(r_qJd=RETRY_WEIGHTS[name]) if name in RETRY_WEIGHTS else None


def _oracle_forced_retry(name, prob, g, snap, opts):
    r = O.solve_batch(prob, O.default_options(**opts), n_threads=8, weights={"r_qJd": RETRY_WEIGHTS[name]})
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], r[f]), f
    if name == "retry_ok":  # test_retries_match_oracle's comparison
        assert np.all(r["status"] == 0)
        for f in ("Xbar", "Ubar", "K", "dU"):
            assert rel(g[f], r[f]) < 1e-9, f
        # a sweep that succeeds after retries leaves mu / 20 > 0 as the next regularisation
        # (backward_sweep_regularized, MultiPhaseDDP.cpp:141-181): every element retried
        assert np.all(snap["el"]["reg"] > 0), snap["el"]["reg"]
    else:  # test_regularization_overflow_status's: bad_solve in the first iteration, the nominal rows kept
        assert np.all(r["status"] == 1) and np.all(r["iters"] == 1)
        assert np.all(snap["el"]["status"] == 1) and np.all(snap["el"]["done"] == 1)
        for f in ("Xbar", "Ubar"):
            assert rel(g[f], r[f]) < 1e-9, f


@functools.lru_cache(None)
def base_run(name, optkey):
    """step 1, once per base set and options: the base handle's solve against the oracle; returns its
    snapshot"""
    opts, prob = dict(optkey), base_set(name)
    g, snap = _gpu(prob, opts, _weights(name))
    if name == "retry":
        _oracle_retry(prob, g, snap, opts)
    elif name in RETRY_WEIGHTS:
        _oracle_forced_retry(name, prob, g, snap, opts)
    elif opts:
        _oracle_fixed(prob, g, opts)
    else:
        r = _oracle_full(prob, g)
        # elements that have finished sit beside live ones in a wave only if the counts differ
        assert len(set(r["iters"].tolist())) >= 3 and len(set(g["iters"].tolist())) >= 3, g["iters"]
    return snap


def run_case(name, opts, B, seed, **kw):
    """steps 2 and 3 at batch size B; returns the index maps that ran"""
    prob, groups = base_set(name), TC.layout_groups_of(base_set(name))
    snap = base_run(name, tuple(sorted(opts.items())))
    maps = TC.draws(prob["batch"], B, seed, groups)
    for index in maps:
        t0 = time.perf_counter()
        big = hsddp.Solver(TC.tile(prob, index), hsddp.load_settings(**opts), weights=_weights(name))
        big.solve()
        t1 = time.perf_counter()
        TC.same(big, snap, index, **kw)
        print(f"[{name} B={B}] pairs {TC.n_pairs(index, groups, prob['batch'])}, device bytes {big.device_bytes()}, "
              f"create+solve {t1 - t0:.2f} s, compare {time.perf_counter() - t1:.2f} s")
        big.close()
    return maps


# ---- sweep and decide edges ----------------------------------------------------------------------------
EDGES = [16, 17, (2, -1), (2, 0), (2, 1), (8, -1), (8, 0), (8, 1)]
_IDS = lambda s: str(s) if isinstance(s, int) else f"{s[0]}CU{s[1]:+d}"  # noqa: E731


@pytest.mark.parametrize("spec", EDGES, ids=_IDS)
@pytest.mark.parametrize("name", ["trot", "pairs"])
def test_sweep_and_decide_edges(name, spec):
    """B = 16 | 17: the trial decided in the rollout launch | by k_decide.  Pairs <= CUs | more: the
    column-split sweep | the one-wave sweep, two pairs per workgroup up to 4 CUs pairs | one beyond."""
    B, seed = size(spec), EDGES.index(spec)
    maps = run_case(name, FIXED, B, seed)
    prob = base_set(name)
    groups = TC.layout_groups_of(prob)
    if B > 17:  # the side of the sweep's edge this batch is on: by its pairs
        pairs, edge = TC.n_pairs(maps[0], groups, 5), (cus() if spec[0] == 2 else 4 * cus())
        if groups is None:
            assert pairs == (B + 1) // 2
        if spec[1] != 0 or groups is None:  # (odd B: (B + 1) / 2 pairs whatever the layouts)
            assert pairs == edge + (spec[1] > 0), (B, pairs, edge)
        else:  # even B, two layouts: one pair more when both layouts' counts are odd
            assert pairs in (edge, edge + 1), (B, pairs, edge)


def test_every_base_element_is_the_last_one_somewhere():
    """over the edge sizes (seeds 0 .. 7): every base element at B - 1 or beside it"""
    for name in ("trot", "pairs"):
        groups = TC.layout_groups_of(base_set(name))
        maps = [m for k, spec in enumerate(EDGES) for m in TC.draws(5, size(spec), k, groups)]
        TC.assert_last(maps, 5)
        odd = [m for m in maps if len(m) % 2]
        assert {int(m[-1]) for m in odd} == set(range(5))  # ... and alone in the last, half-empty pair


@pytest.mark.parametrize("spec", [(2, -1), (2, 0), (2, 1), (8, -1), (8, 0), (8, 1)], ids=_IDS)
@pytest.mark.parametrize("name", ["trot_ss", "pairs_ss"])
def test_sweep_edges_single_shooting(name, spec):
    """MS 0: the sweeps' dV instantiations and k_rollout_ss (four elements per wave)"""
    run_case(name, dict(FIXED, MS=0), size(spec), 3 + spec[0] + spec[1])


# ---- terminal tasks ------------------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["merged", "own launch"])
def test_terminal_task_edge(side):
    """blocks_for(B P, 8) steps from 256 to 257 between these two B (jump, P = 8: B = 256 | 257 whatever
    the CU count, half the sweep's edge on an MI355X)"""
    P = 8
    B = TERM_MERGED_BLOCKS * TERM_TASKS_PER_BLOCK // P + (side != "merged")
    blocks = -(-B * P // TERM_TASKS_PER_BLOCK)
    assert blocks == (256 if side == "merged" else 257)
    run_case("jump8", FIXED, B, 11 + B)


# ---- per-element control flow --------------------------------------------------------------------------
@pytest.mark.parametrize("spec", [(2, 1), (8, 1)], ids=_IDS)
def test_full_solves_stop_where_the_base_stops(spec):
    """The shipped settings (early exits on): copies of one problem stop at the same iteration with
    the same trial counts (ElemState is in the records), beside copies of problems that run two and
    three times as long in the same wave."""
    run_case("mixed", {}, size(spec), 21 + spec[0])


# ---- retries -------------------------------------------------------------------------------------------
RETRY_OPTS = {"retry": dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=12), "retry_ok": FIXED, "retry_exhausted": {}}


@pytest.mark.parametrize("spec", [3, 4, (8, 1)], ids=_IDS)
@pytest.mark.parametrize("name", ["retry", "retry_ok", "retry_exhausted"])
def test_retries(name, spec):
    """B = 3 | 4: every retry inside k_riccati | the parallel retry (k_riccati_retry / _select).
    8 CUs + 1: the copies of a base element fail in the same launch — retry_ok / retry_exhausted: all
    of them, retry (on the oracle's path) some 400 — more than the 128 the retry list takes (and, at
    8 x 25, more than the 30 its scratch holds), so most run the in-kernel loop beside the deferred
    ones; retry_exhausted: k_riccati_select's no-winner path, which leaves each gain row as the last
    attempt that got past it left it."""
    B = size(spec)
    if B > 4:
        assert B // 5 > 128
    run_case(name, RETRY_OPTS[name], B, 31)


# ---- the benchmark's configuration ---------------------------------------------------------------------
@pytest.mark.parametrize("B", [4096, 4097])
def test_metric_configuration_every_element(B):
    """trot 4 x 50 at the benchmark's batch size and one past it: every element, every field, the
    gain rows included (measured: 1.7 s alone, 4.3 s inside the whole suite — 3.8 GB of records
    through the host in chunks of 512)"""
    run_case("metric", FIXED, B, B, chunk=512)


# ---- buffers past 2 GiB and 4 GiB ----------------------------------------------------------------------
def _straddling(per_elem, total, first=0):
    """[(boundary, elements)]: for every multiple of 2^31 bytes inside a buffer of `total` bytes whose
    element e starts at first + e per_elem, the 16 elements around it"""
    out = []
    for k in range(1, (first + total - 1) // 2 ** 31 + 1):
        at = k * 2 ** 31 - first
        if at <= 0:
            continue
        e, n = at // per_elem, total // per_elem
        lo = min(max(e - 8, 0), n - 16)
        out.append((at, list(range(lo, lo + 16))))
    return out


def test_buffers_past_4_gib():
    """trot 4 x 50 at the smallest B = 8 m + 1 whose fp64 gain rows pass 2^32 bytes (the LQ records then
    pass 2^31): no product of an element index and a row stride may be formed in 32 bits.  Element info,
    the cost history and the layouts of every element; full records of the first and last 16 and of
    the 16 around every multiple of 2^31 bytes in the gain rows, the LQ records and the three-buffer
    state and control sets (at this B those two sets stay below 2^31: the list says so)."""
    Kc, S_cap = 200, 200 + TC.MAXP
    k_el, lq_el = Kc * TC.KCW * 8, Kc * 176 * 8  # bytes per element: K [Kc][KCW], lq [Kc][LQW]
    B = -(-(2 ** 32 + 1) // k_el)
    B += (1 - B) % 8
    assert B % 8 == 1 and B * k_el > 2 ** 32 >= (B - 8) * k_el and B * lq_el > 2 ** 31
    prob = base_set("metric")
    snap = base_run("metric", tuple(sorted(FIXED.items())))
    # what the handle will take, from two small handles of the same problem (both past the 30 elements
    # whose retry scratch a handle of this horizon allocates)
    small = [hsddp.Solver(TC.tile(prob, np.arange(m) % 5), hsddp.load_settings(**FIXED)) for m in (40, 104)]
    per = (small[1].device_bytes() - small[0].device_bytes()) / 64
    for s in small:
        s.close()
    need = int(per * B) + (1 << 29)
    free = _torch("torch.cuda.mem_get_info()[0]")
    if free < 2 * need:
        print(f"[4 GiB] skipped: {free} bytes free, the handle needs about {need}")
        pytest.skip(f"device memory: {free} bytes free, about {need} needed twice over")
    index = TC.draw(5, B, 9)
    t0 = time.perf_counter()
    big = hsddp.Solver(TC.tile(prob, index), hsddp.load_settings(**FIXED))
    big.solve()
    t1 = time.perf_counter()
    print(f"[4 GiB] B = {B}, device bytes {big.device_bytes()} (estimated {need}), create+solve {t1 - t0:.2f} s")
    assert big.device_bytes() > 2 ** 33
    # every element: the scalars, the history, the layouts
    info, hist = big.element_info(), big.solver_info()["cost"]
    want = {"cost": "cost", "feas": "feas", "merit": "merit", "max_tconstr": "max_t", "max_pconstr": "max_p", "iters": "iters",
            "outer_iters": "outer_iters", "status": "status", "n_ls_trials": "n_ls"}
    for f, e in want.items():
        a, w = info[f], np.ascontiguousarray(snap["el"][e])[index]
        if w.dtype == np.float64:
            a, w = a.view(np.uint64), w.view(np.uint64)
        ne = np.flatnonzero(a != w)
        assert ne.size == 0, (f, ne[:8].tolist())
    for b in range(B):
        n = int(snap["el"]["hist_n"][index[b]])
        assert np.array_equal(hist[b], snap["hist"][index[b], :n, 0]), b
    # full records: the ends, and around every 2^31-byte boundary
    groups = [("first", None, list(range(16))), ("last", None, list(range(B - 16, B)))]
    sets = {"K": (k_el, B * k_el, 0), "lq": (lq_el, B * lq_el, 0)}
    for q in range(3):  # buffer q of X3 / D3 [3][B][S_cap][24] and U3 [3][B][Kc][24]
        sets[f"X3[{q}]"] = (S_cap * 192, B * S_cap * 192, q * B * S_cap * 192)
        sets[f"U3[{q}]"] = (Kc * 192, B * Kc * 192, q * B * Kc * 192)
    found = {}
    for name, (pe, total, first) in sets.items():
        for at, el in _straddling(pe, total, first):
            assert 0 <= el[0] and el[-1] < B and el[0] * pe < at < (el[-1] + 1) * pe, (name, at, el)
            assert any(e * pe < at < (e + 1) * pe or (e + 1) * pe == at for e in el)
            groups.append((name, first + at, el))
            found.setdefault(name, []).append(first + at)
    assert found.get("K") == [2 ** 31, 2 ** 32] and found.get("lq") == [2 ** 31], found
    print("[4 GiB] boundaries inside the buffers:", found)
    for name, at, el in groups:
        TC.same(big, snap, index, elements=el)
    print(f"[4 GiB] compare {time.perf_counter() - t1:.2f} s, {sum(len(g[2]) for g in groups)} full records")
    big.close()
