"""Phases with one and three legs in stance: the solver on all 16 contact masks against the oracle.

The older GPU files run synthetic.GAITS' trot, pace, bound, pronk and jump: the eight masks with an
even number of stance legs, and touchdowns of two or four legs.  The four cycles used here hold the
rest (masks written leg 0 first, (FR, FL, HR, HL), the contacts array's order):

  crawl  three-leg stance throughout; every switch lifts one leg while another lands, with stance
         neighbours on both sides (reset maps both ways at one boundary, single-leg touchdowns)
  amble  both trot masks, each between two three-leg masks: the sweep's specialised loops
         (phase_knots_masked<MASK_TROT_A / _B>) one phase away from the runtime-mask loop in one
         element, and single-leg touchdowns and lift-offs
  hop    single-leg stance, single-leg touchdown out of flight, three-leg touchdown (0100 -> 1111,
         td_mask 13) and three-leg lift-off
  gray   all 16 masks, every switch one leg

Shapes: crawl 4 x 4, amble 8 x 4, hop 8 x 4, gray 16 x 4 (each cycle once), B = 5 (the last wave's
second half is borrowed and inactive).  Unless a test says otherwise each case runs with
HSDDP_SWEEP_SPLIT=0 (the one-wave k_riccati) and with the default, which at these sizes is the
column split k_riccati_cs.  Tolerances and compared fields are those of the tests named in each
docstring; the oracle's own deviation under a 1e-15 relative change of x0 stays below 1e-13 on
these problems, so the envelope rule max(1e-9, 10 x envelope) sits on its floor.
"""
import ctypes
import functools

import numpy as np
import pytest

import hsddp
import oracle_lib as O
from hsddp import synthetic as syn
from test_gpu_sweep_masks import _both, _same as _same_masks
from test_gpu_sweep_split import _same as _same_split

pytestmark = pytest.mark.gpu

SHAPES = {"crawl": (4, 4), "amble": (8, 4), "hop": (8, 4), "gray": (16, 4)}
CASES = [(g, P, N) for g, (P, N) in SHAPES.items()]
B = 5
FIXED = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=3)
SPLITS = pytest.mark.parametrize("split", ["0", None], ids=["one-wave", "default"])
# a trot half beside a half one leg away from it; an amble pair (the specialised loop in its two
# trot-mask phases only); halves on masks without a loop of their own
NEIGHBOURS = [("trot", 8, 4), ("amble", 8, 4), ("amble", 8, 4), ("trot", 8, 4), ("gray", 16, 2), ("crawl", 8, 4)]


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


def _set_split(monkeypatch, split):
    if split is None:
        monkeypatch.delenv("HSDDP_SWEEP_SPLIT", raising=False)
    else:
        monkeypatch.setenv("HSDDP_SWEEP_SPLIT", split)


def _weights(**kw):
    w = hsddp.Weights()
    hsddp._lib.lib().hsddp_default_weights(ctypes.byref(w))
    for k, v in kw.items():
        setattr(w, k, v)
    return w


def _run(prob, weights=None, fp32=False, constraints=False, **kw):
    s = hsddp.Solver(prob, hsddp.load_settings(**kw), weights=weights, riccati_fp32=fp32)
    s.solve()
    out = {**s.trajectory(), **s.working(), **s.element_info()}
    if constraints:
        out.update(s.constraint_params())
        out.update(s.constraint_values())
    s.close()
    return out


@functools.lru_cache(maxsize=None)
def _oracle(gait, batch, opts, r_qJd=None):
    """(problem, oracle run, oracle run from x0 (1 + 1e-15)) — computed once per case and shared by
    the tests (they only read it).  opts: the option overrides as a sorted tuple of pairs."""
    P, N = SHAPES[gait]
    prob = syn.make_batch(batch, P, N, gait)
    w = None if r_qJd is None else {"r_qJd": r_qJd}
    r = O.solve_batch(prob, O.default_options(**dict(opts)), n_threads=8, weights=w)
    p2 = dict(prob); p2["x0"] = prob["x0"] * (1 + 1e-15)
    r2 = O.solve_batch(p2, O.default_options(**dict(opts)), n_threads=8, weights=w)
    return prob, r, r2


def _opts(**kw):
    return tuple(sorted(kw.items()))


def _masks(contacts):
    """the set of Phase::cmask values of a contacts array's rows (bit l = leg l)"""
    c = np.asarray(contacts).reshape(-1, 4) != 0
    return set((c * (1 << np.arange(4))).sum(axis=1).tolist())


def test_the_shapes_reach_every_mask():
    """What the cases below run on: gray 16 x 4 holds all 16 masks as phases of a solve; crawl, amble
    and hop hold the odd masks between neighbours gray does not give them (amble: 1001 and 0110 with
    three-leg masks on either side)."""
    assert _masks(syn.make_batch(1, 16, 4, "gray")["contacts"][:, :16]) == set(range(16))
    assert _masks(syn.make_batch(1, 4, 4, "crawl")["contacts"]) == {14, 13, 11, 7}
    am = syn.make_batch(1, 8, 4, "amble")["contacts"][0]
    rows = [int((r * (1 << np.arange(4))).sum()) for r in am]
    for trot in (0b1001, 0b0110):
        i = rows.index(trot)
        assert bin(rows[i - 1]).count("1") == 3 and bin(rows[i + 1]).count("1") == 3
    assert {1, 2, 4, 8, 0, 15} <= _masks(syn.make_batch(1, 8, 4, "hop")["contacts"])
    lay = syn.make_layout_batch(NEIGHBOURS)
    assert _masks(lay["contacts"][4, :17]) == set(range(16))


# ---- fixed iterations, and the touchdown bookkeeping they leave ---------------------------------
_fixed_runs = {}


def _fixed(monkeypatch, gait, split):
    """the GPU's three fixed iterations of a case (one run per case and kernel, shared)"""
    if (gait, split) not in _fixed_runs:
        _set_split(monkeypatch, split)
        _fixed_runs[gait, split] = _run(_oracle(gait, B, _opts(**FIXED))[0], constraints=True, **FIXED)
    return _fixed_runs[gait, split]


@SPLITS
@pytest.mark.parametrize("gait,P,N", CASES)
def test_fixed_iterations_match_oracle(monkeypatch, gait, P, N, split):
    """test_gpu_parity.py::test_fixed_iterations_match_oracle's fields, tolerances (the envelope rule)
    and exact integer fields, three iterations."""
    prob, r, r2 = _oracle(gait, B, _opts(**FIXED))
    assert np.all(r["status"] == 0) and np.all(np.isfinite(r["K"]))
    g = _fixed(monkeypatch, gait, split)
    for f in ("Xbar", "Ubar", "K", "X", "U", "dX", "dU"):
        e, tol = rel(g[f], r[f]), max(1e-9, 10 * rel(r2[f], r[f]))
        print(f"{gait} split={split} {f}: rel {e:.3e} (bound {tol:.3e})")
        assert e < tol, f
    for f in ("cost", "feas", "max_tconstr"):
        assert rel(g[f], r[f]) < 1e-9, f
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], r[f]), f


@SPLITS
@pytest.mark.parametrize("gait", ["hop", "gray"])
def test_touchdown_bookkeeping(monkeypatch, gait, split):
    """td_mask as resolved from the contact rows (legs with contact 0 -> 1 across each phase end, one
    constraint per phase): single legs, and hop's three legs at once (0100 -> 1111: mask 13); the
    per-leg AL parameters (k_decide) and the stored touchdown heights against the oracle's at 1e-9,
    as test_gpu_mpc.py::test_mpc_loop_matches_oracle compares them."""
    prob, r, _ = _oracle(gait, B, _opts(**FIXED))
    g = _fixed(monkeypatch, gait, split)
    c = prob["contacts"] != 0
    want = ((~c[:, :-1] & c[:, 1:]) * (1 << np.arange(4))).sum(axis=2)  # [B][P]
    assert np.array_equal(g["td_mask"][:, :, 0], want) and not g["td_mask"][:, :, 1:].any()
    assert np.array_equal(g["td_mask"], r["td_mask"])
    seen = set(want.reshape(-1).tolist())
    if gait == "hop":
        assert {2, 8, 13, 7} <= seen  # legs 1 and 3 alone; legs 0, 2, 3; legs 0, 1, 2
    else:
        assert seen == {0, 1, 2, 4, 8}
    for f in ("al_sigma", "al_lambda", "td_h"):
        assert rel(g[f], r[f]) < 1e-9, f
    # (the heights are those of the touchdown legs alone, and not all zero)
    on = (g["td_mask"][..., None] >> np.arange(4)) & 1
    assert np.all(g["td_h"][on == 0] == 0) and np.any(g["td_h"][on == 1] != 0)


# ---- full solves --------------------------------------------------------------------------------
@SPLITS
@pytest.mark.parametrize("gait,P,N", CASES)
def test_full_solve_matches_oracle(monkeypatch, gait, P, N, split):
    """test_gpu_parity.py::test_full_solve_matches_oracle's comparisons at the shipped settings, B = 6.
    Measured on the oracle: every element ends with status 0 after 16 to 44 iterations and none is
    chaotic under that test's screen, so nothing is screened out: the screen must stay empty."""
    nb = 6
    prob, r, r2 = _oracle(gait, nb, _opts())
    chaotic = [b for b in range(nb) if r["n_ls_trials"][b] != r2["n_ls_trials"][b]
               or abs(r["cost"][b] - r2["cost"][b]) > 1e-8 * abs(r["cost"][b])]
    assert len(chaotic) == 0, chaotic
    assert np.all(r["status"] == 0)
    _set_split(monkeypatch, split)
    g = _run(prob)
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], r[f]), f
    for f in ("Xbar", "Ubar"):
        e = rel(g[f], r[f])
        print(f"{gait} split={split} {f}: rel {e:.3e}")
        assert e < 1e-7, f
    assert rel(g["cost"], r["cost"]) < 1e-9


# ---- regularisation retries ---------------------------------------------------------------------
@SPLITS
@pytest.mark.parametrize("gait,P,N", CASES)
def test_retries_match_oracle(monkeypatch, gait, P, N, split):
    """test_gpu_parity.py::test_retries_match_oracle's workload (r_qJd = -0.5: every first sweep fails
    the PSD test, in the swing legs' joint-velocity diagonals — one, two, three or four legs of them
    by phase) and comparisons; on amble and gray the in-kernel sequential schedule
    (HSDDP_SEQUENTIAL_RETRY=1) equals the parallel retries bit for bit."""
    prob, r, _ = _oracle(gait, B, _opts(**FIXED), -0.5)
    assert np.all(r["status"] == 0) and np.all(r["iters"] == 3)
    _set_split(monkeypatch, split)
    w = _weights(r_qJd=-0.5)
    g = _run(prob, weights=w, **FIXED)
    assert np.array_equal(g["status"], r["status"])
    assert np.array_equal(g["n_ls_trials"], r["n_ls_trials"])
    for f in ("Xbar", "Ubar", "K", "dU"):
        assert rel(g[f], r[f]) < 1e-9, f
    if gait in ("amble", "gray"):
        monkeypatch.setenv("HSDDP_SEQUENTIAL_RETRY", "1")
        q = _run(prob, weights=w, **FIXED)
        for f in ("Xbar", "Ubar", "K", "X", "U", "dU", "dX", "cost", "feas", "iters", "status", "n_ls_trials"):
            assert np.array_equal(g[f], q[f]), f


# ---- the sweep's dispatch on the contact mask ---------------------------------------------------
@pytest.mark.parametrize("wpb", [None, "2"])
def test_dispatch_within_one_element(monkeypatch, wpb):
    """amble 8 x 4, B = 4: phases on 1001 and 0110 take the specialised loops, their neighbours in the
    same element (1101, 1011; 1110, 0111) the runtime-mask loop; HSDDP_SWEEP_MASKS 1 against 0, bit
    for bit (test_gpu_sweep_masks.py's _both / _same), also at two pairs per workgroup."""
    if wpb:
        monkeypatch.setenv("HSDDP_SWEEP_WPB", wpb)
    _same_masks(*_both(monkeypatch, syn.make_batch(4, 8, 4, "amble")))


def test_dispatch_between_neighbouring_halves(monkeypatch):
    """Per-element layouts: a trot element paired with an amble element (the halves' masks one leg
    apart in most phases, equal on neither trot phase at the same index), an amble pair, and a pair
    on masks without a loop of their own (gray, crawl)."""
    prob = syn.make_layout_batch(NEIGHBOURS)
    a, b = _both(monkeypatch, prob)
    _same_masks(a, b)
    assert np.all(a["status"] == 0)


def test_runtime_mask_loop_matches_oracle(monkeypatch):
    """HSDDP_SWEEP_MASKS=0 on gray 16 x 4: the one-wave sweep with every phase — the two trot-mask
    phases included — on the runtime-mask loop, against the oracle (the fixed-iteration test's
    fields and bounds); with the default it takes the specialised loops there, equal bit for bit."""
    prob, r, r2 = _oracle("gray", B, _opts(**FIXED))
    assert {0b1001, 0b0110} <= _masks(prob["contacts"][:, :16])
    a, g = _both(monkeypatch, prob, **FIXED)
    _same_masks(a, g)
    for f in ("Xbar", "Ubar", "K", "X", "U", "dX", "dU"):
        assert rel(g[f], r[f]) < max(1e-9, 10 * rel(r2[f], r[f])), f
    assert rel(g["cost"], r["cost"]) < 1e-9
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], r[f]), f


# ---- the column split against the one-wave sweep ------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True], ids=["fp64", "fp32"])
@pytest.mark.parametrize("case", ["gray", "layouts"])
def test_split_equals_one_wave_sweep(monkeypatch, case, fp32):
    """test_gpu_sweep_split.py::test_split_equals_one_wave_sweep's equality (full solves, every
    compared field bit for bit) on gray 16 x 4, B = 5, and on the neighbouring-halves layouts.  (The
    fp32 mode has no column split: launch_riccati keeps it on the one-wave kernel whatever the
    switch says, which is what its two runs pin.)"""
    prob = syn.make_batch(B, 16, 4, "gray") if case == "gray" else syn.make_layout_batch(NEIGHBOURS)
    monkeypatch.setenv("HSDDP_SWEEP_SPLIT", "1")
    a = _run(prob, fp32=fp32)
    monkeypatch.setenv("HSDDP_SWEEP_SPLIT", "0")
    b = _run(prob, fp32=fp32)
    _same_split(a, b)
    assert np.all(np.isfinite(a["Xbar"])) and np.all(a["status"] == 0)


# ---- the fp32 Riccati mode ----------------------------------------------------------------------
@pytest.mark.parametrize("gait,P,N", CASES)
def test_fp32_one_iteration_within_tolerance(gait, P, N):
    """test_gpu_fp32.py::test_fp32_one_iteration_within_tolerance's bounds: 5e-5 on the arrays, 5e-6
    on the cost, equal line-search trial counts."""
    kw = dict(no_early_exit=1, max_AL_iter=1, max_DDP_iter=1)
    prob, r, _ = _oracle(gait, B, _opts(**kw))
    g = _run(prob, fp32=True, **kw)
    for f in ("K", "dU", "dX", "Xbar", "Ubar"):
        e = rel(g[f], r[f])
        print(f"{gait} fp32 {f}: rel {e:.3e}")
    print(f"{gait} fp32 cost: rel {rel(g['cost'], r['cost']):.3e}")
    for f in ("K", "dU", "dX", "Xbar", "Ubar"):
        assert rel(g[f], r[f]) < 5e-5, f
    assert rel(g["cost"], r["cost"]) < 5e-6
    assert np.array_equal(g["n_ls_trials"], r["n_ls_trials"])


# ---- single shooting ----------------------------------------------------------------------------
@SPLITS
def test_single_shooting_crawl(monkeypatch, split):
    """MS = 0 on crawl 4 x 4, three fixed iterations, test_gpu_single_shooting.py's fields and
    tolerances.  (Of the four cycles only crawl takes steps without multiple shooting — the oracle
    rejects every trial on the others — so some element must have accepted one: fewer than the four
    trials per iteration of an exhausted line search.)"""
    kw = dict(MS=0, **FIXED)
    prob, r, r2 = _oracle("crawl", B, _opts(**kw))
    assert np.all(r["iters"] == 3) and np.any(r["n_ls_trials"] < 4 * r["iters"])
    _set_split(monkeypatch, split)
    g = _run(prob, **kw)
    for f in ("Xbar", "Ubar", "K", "X", "U", "dU"):
        assert rel(g[f], r[f]) < max(1e-9, 10 * rel(r2[f], r[f])), f
    for f in ("cost", "feas", "max_tconstr", "merit"):
        assert rel(g[f], r[f]) < max(1e-9, 10 * rel(r2[f], r[f])), f
    for f in ("iters", "outer_iters", "status", "n_ls_trials"):
        assert np.array_equal(g[f], r[f]), f
    assert np.any(g["n_ls_trials"] < 4 * g["iters"])
    assert np.all(g["dX"] == 0)
