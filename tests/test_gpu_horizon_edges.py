"""The code paths that the horizon's size selects, either side of every threshold.

S = sum(N_i + 1) state slots.  Three kernels choose a path from p.S (a handle with per-element
layouts: the largest layout's S):

* element_cost (hsddp_sweep.hip) stages the element's slot costs in the item's LDS while two arrays
  of p.S doubles fit the item and its 16 loads per lane cover them — S <= 509 in the fp64 one-wave
  sweep, <= 254 in fp32, <= 512 in the column split — and reads global memory directly above;
* k_rollout runs its narrow instantiation for S <= 64 and WIDE from S = 65 (RW) on;
* decide_group, element_cost, rollout_boundary and k_terminal give a lane or a task to each of up
  to MAXP = 16 phases; a phase of one knot has no next knot for the sweeps' image prefetch.

Section 1 and 3 compare with the oracle under the standing fixed-iteration rule (test_gpu_parity.py):
trajectory fields rel < max(1e-9, 10 x the oracle's own deviation under x0 * (1 + 1e-15)), every
count equal, no element screened out; cost, feas and merit within 1e-9 of max(1, max|ref|) (feas
is ~0 at the tiny horizons, where a relative envelope means nothing).  Section 2 isolates the
thresholds with no tolerance at all: one long-layout element in a handle switches the path of its
short-layout neighbours, which must still be solved bit for bit as in a handle of their own
(test_gpu_layouts.py's invariant).  Every figure is printed before it is asserted (pytest -s).
"""
import functools

import numpy as np
import pytest

import hsddp
import oracle_lib as O
from hsddp import synthetic as syn

pytestmark = pytest.mark.gpu

FIELDS = ("Xbar", "Ubar", "K", "X", "U", "dU", "dX", "cost", "feas", "merit", "iters", "outer_iters", "status",
          "n_ls_trials")  # test_gpu_sweep_split.py's
TRAJ = ("Xbar", "Ubar", "K", "X", "U", "dX", "dU")
SCALARS = ("cost", "feas", "merit")
COUNTS = ("iters", "outer_iters", "status", "n_ls_trials")
SLOT_ROWS = ("Xbar", "X", "Defect", "dX")  # [B][S][24]: an element's first S_b rows
KW = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=2)
# the sweeps a small fp64 batch can be given: the column split, the one-wave kernel at one and at
# two element pairs per workgroup
SWEEPS = {"split": ("1", None), "wpb1": ("0", "1"), "wpb2": ("0", "2")}


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


def _run(monkeypatch, prob, sweep=None, fp32=False, full=False, **kw):
    if sweep is not None:
        split, wpb = SWEEPS[sweep]
        monkeypatch.setenv("HSDDP_SWEEP_SPLIT", split)
        if wpb is not None:
            monkeypatch.setenv("HSDDP_SWEEP_WPB", wpb)
    s = hsddp.Solver(prob, hsddp.load_settings(**kw), riccati_fp32=fp32)
    s.solve()
    out = {**s.trajectory(), **s.working(), **s.element_info()}
    if full:
        out["lq"], out["term"] = s.lq(), s.terminal()
    s.close()
    return out


@functools.lru_cache(maxsize=None)
def _oracle_case(B, gait, P, N, ms):
    """The batch, the oracle's solve and its solve under x0 * (1 + 1e-15); shared, left unchanged."""
    prob = syn.make_batch(B, P, N, gait)
    return (prob,) + _oracle(prob, ms)


def _oracle(prob, ms):
    opt = O.default_options(MS=ms, **KW)
    r = O.solve_batch(prob, opt, n_threads=8)
    p2 = dict(prob); p2["x0"] = prob["x0"] * (1 + 1e-15)
    return r, O.solve_batch(p2, opt, n_threads=8)


def _against_oracle(tag, g, r, r2):
    """The fixed-iteration rule; g holds the oracle's elements and rows only."""
    checks = []
    for f in TRAJ:
        checks.append((f, rel(g[f], r[f]), max(1e-9, 10 * rel(r2[f], r[f]))))
    for f in SCALARS:
        scale = max(1.0, float(np.max(np.abs(r[f]))))
        checks.append((f, float(np.max(np.abs(g[f] - r[f]))) / scale, 1e-9))
    for f, err, bound in checks:
        print(f"EDGE {tag} {f} err {err:.3e} bound {bound:.3e}")
    for f, err, bound in checks:
        assert err < bound, (tag, f, err, bound)
    assert np.all(r["status"] == 0), tag
    for f in COUNTS:
        assert np.array_equal(g[f], r[f]), (tag, f, g[f], r[f])


def _same(a, b, tag):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (tag, f)


# ---- 1. oracle parity either side of every S threshold ---------------------------------------
@pytest.mark.parametrize("ms", [1, 0])
@pytest.mark.parametrize("gait,P,N", [("trot", 4, 15), ("jump", 8, 7), ("trot", 5, 12)])
def test_rollout_width_threshold_matches_oracle(monkeypatch, gait, P, N, ms):
    """S = 64 (k_rollout's narrow instantiation at its largest: a wave holds exactly one element)
    and S = 65 (WIDE at its smallest: every wave but the first starts inside an element), multiple
    and single shooting."""
    prob, r, r2 = _oracle_case(3, gait, P, N, ms)
    assert prob["S"] == (65 if P == 5 else 64)
    _against_oracle(f"s1 {gait}{P}x{N} S{prob['S']} MS{ms}", _run(monkeypatch, prob, MS=ms, **KW), r, r2)


@pytest.mark.parametrize("S,gait,P,N", [(509, "trot", 1, 508), (510, "trot", 10, 50), (512, "jump", 8, 63),
                                         (513, "trot", 9, 56), (834, "jump", 6, 138), (835, "trot", 5, 166)])
def test_cost_staging_thresholds_match_oracle(monkeypatch, S, gait, P, N):
    """element_cost's staged and direct sums: 509 / 510 the one-wave kernel's last staged and first
    direct S, 512 / 513 the split's, 834 the last S at which two arrays fit the split's item
    (direct since the staging pass covers 512 slots), 835 direct on either count.  The three sweeps
    add the same doubles in the same order: bit-identical, and each against the oracle."""
    prob, r, r2 = _oracle_case(3, gait, P, N, 1)
    assert prob["S"] == S
    runs = {sw: _run(monkeypatch, prob, sw, **KW) for sw in SWEEPS}
    for sw, g in runs.items():
        _against_oracle(f"s1 {gait}{P}x{N} S{S} {sw}", g, r, r2)
    _same(runs["split"], runs["wpb1"], "split / wpb1")
    _same(runs["wpb2"], runs["wpb1"], "wpb2 / wpb1")


# ---- 2. the thresholds in isolation: mixed handles against uniform handles -------------------
LQ_FIELDS = ("A", "B", "lx", "lu", "lxx", "luu", "l")
TERM_FIELDS = ("Phi", "Phix", "Phixx", "Px")
ELEMENT_FIELDS = ("cost", "feas", "merit", "max_tconstr", "max_pconstr", "iters", "outer_iters", "status",
                  "n_ls_trials")


def _equal_uniform(g, prob, run, tag):
    """Every element of the mixed handle's solve g equals, bit for bit, its solve in a uniform
    handle of its layout (test_gpu_layouts.py's _check_against_uniform); returns the uniform solves
    {horizons: (elements, sub-batch, solve)}."""
    out = {}
    for hz, idx in syn.layout_groups(prob).items():
        sub = syn.sub_batch(prob, idx, hz)
        u = run(sub)
        S, P = sub["S"], len(hz)
        for f in SLOT_ROWS:
            assert np.array_equal(g[f][idx, :S], u[f]), (tag, hz[0], f)
        for f in ("Ubar", "U", "dU", "K") + ELEMENT_FIELDS:
            assert np.array_equal(g[f][idx], u[f]), (tag, hz[0], f)
        for f in LQ_FIELDS:
            assert np.array_equal(g["lq"][f][idx], u["lq"][f]), (tag, hz[0], f)
        for f in TERM_FIELDS:
            assert np.array_equal(g["term"][f][idx, :P], u["term"][f]), (tag, hz[0], f)
            assert np.all(g["term"][f][idx, P:] == 0), (tag, hz[0], f)
        out[hz] = (idx, sub, u)
    return out


def test_fp32_staging_threshold_mixed_equals_uniform(monkeypatch):
    """fp32 sweep (item of 4072 bytes: staged up to S = 254).  2 x 126 (S = 254) is staged in its
    own handle and read directly beside a 3 x 84 element (p.S = 255); both groups equal their
    uniform solves."""
    prob = syn.make_layout_batch([("trot", 2, 126)] * 2 + [("trot", 3, 84)])
    assert (prob["Kc"], prob["S"]) == (252, 255)
    kw = dict(KW, max_DDP_iter=1)
    run = lambda q: _run(monkeypatch, q, fp32=True, full=True, **kw)  # noqa: E731
    uni = _equal_uniform(run(prob), prob, run, "fp32")
    assert sorted(v[1]["S"] for v in uni.values()) == [254, 255]


@pytest.mark.parametrize("sweep", ["wpb1", "wpb2"])
def test_one_wave_staging_threshold_mixed_equals_uniform(monkeypatch, sweep):
    """fp64 one-wave sweep (item of 8144 bytes: staged up to S = 509): 1 x 508 alone is staged,
    beside a 2 x 254 element (p.S = 510) it is read directly."""
    prob = syn.make_layout_batch([("trot", 1, 508)] * 2 + [("trot", 2, 254)])
    assert (prob["Kc"], prob["S"]) == (508, 510)
    run = lambda q: _run(monkeypatch, q, sweep, full=True, **KW)  # noqa: E731
    uni = _equal_uniform(run(prob), prob, run, sweep)
    assert sorted(v[1]["S"] for v in uni.values()) == [509, 510]


@pytest.mark.parametrize("lays,Kc,Sa,Sb", [
    ([("jump", 8, 63)] * 2 + [("trot", 9, 56)], 504, 512, 513),    # the staging pass's 512 slots
    ([("jump", 6, 138)] * 2 + [("trot", 9, 92)], 828, 834, 837)])  # two arrays in the item's 13344 bytes
def test_split_staging_threshold_mixed_equals_uniform(monkeypatch, lays, Kc, Sa, Sb):
    """Column split: staged up to S = 512, what the staging pass covers (8 x 63 alone; beside a
    9 x 56 element it is read directly).  S = 834, the largest at which two arrays would fit the
    item, is read directly alone and beside S = 837."""
    prob = syn.make_layout_batch(lays)
    assert (prob["Kc"], prob["S"]) == (Kc, Sb)
    run = lambda q: _run(monkeypatch, q, "split", full=True, **KW)  # noqa: E731
    uni = _equal_uniform(run(prob), prob, run, "split")
    assert sorted(v[1]["S"] for v in uni.values()) == [Sa, Sb]


def test_rollout_narrow_equals_wide(monkeypatch):
    """k_rollout: three elements (S_b = 64, 63, 62) beside a 5 x 12 jump (Smax = 65: WIDE, every
    wave spanning two elements) and beside a 1 x 60 pace (Smax = 64: narrow, ragged S_b).  Both
    stagings form fma(eps, dX, Xbar) and share the per-slot rollout: the shared elements are
    bit-identical between the handles, every element equals its uniform solve, and every layout
    group matches the oracle."""
    shared = [("trot", 4, 15), ("pronk", 3, 20), ("bound", 2, 30)]
    wide = syn.make_layout_batch(shared + [("jump", 5, 12)])
    narrow = syn.make_layout_batch(shared + [("pace", 1, 60)])
    assert (wide["Kc"], wide["S"], narrow["Kc"], narrow["S"]) == (60, 65, 60, 64)
    run = lambda q: _run(monkeypatch, q, full=True, **KW)  # noqa: E731
    gw, gn = run(wide), run(narrow)
    for b, (_, P, N) in enumerate(shared):
        S = P * (N + 1)
        for f in SLOT_ROWS:
            assert np.array_equal(gw[f][b, :S], gn[f][b, :S]), (b, f)
        for f in ("Ubar", "U", "dU", "K") + ELEMENT_FIELDS:
            assert np.array_equal(gw[f][b], gn[f][b]), (b, f)
        for f in LQ_FIELDS:
            assert np.array_equal(gw["lq"][f][b], gn["lq"][f][b]), (b, f)
        for f in TERM_FIELDS:
            assert np.array_equal(gw["term"][f][b, :P], gn["term"][f][b, :P]), (b, f)
    for name, prob, g in (("wide", wide, gw), ("narrow", narrow, gn)):
        for hz, (idx, sub, u) in _equal_uniform(g, prob, run, name).items():
            if name == "narrow" and len(hz) > 1:
                continue  # the shared layouts' oracle comparison: done on the wide handle's
            r, r2 = _oracle(sub, 1)
            _against_oracle(f"s2 {name} {len(hz)}x{hz[0]}", u, r, r2)  # (u: the mixed handle's, bit for bit)


# ---- 3. phase-count and knot-count edges -----------------------------------------------------
@pytest.mark.parametrize("ms", [1, 0])
@pytest.mark.parametrize("gait,P,N", [("trot", 16, 1), ("jump", 16, 1), ("trot", 6, 1), ("jump", 8, 1),
                                       ("trot", 1, 1), ("trot", 1, 2), ("jump", 16, 4), ("jump", 16, 31),
                                       ("trot", 16, 52)])
def test_phase_and_knot_count_edges_match_oracle(monkeypatch, gait, P, N, ms):
    """MAXP = 16 phases (a lane or task per phase in decide_group, element_cost, rollout_boundary,
    k_terminal) at S = 32, 80 (WIDE), 512 (the last staged S) and 848 (direct); phases of one knot
    (no next knot for the sweeps' image prefetch) down to the one-knot horizon.  B = 5: a sweep
    pair with an idle half and a part-filled decide group."""
    prob, r, r2 = _oracle_case(5, gait, P, N, ms)
    _against_oracle(f"s3 {gait}{P}x{N} S{prob['S']} MS{ms}", _run(monkeypatch, prob, MS=ms, **KW), r, r2)
