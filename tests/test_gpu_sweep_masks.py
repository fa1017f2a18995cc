"""The knot loops specialised on a phase's contact mask (phase_knots_masked, hsddp_sweep.hip)
against the runtime-mask loop.

k_riccati and k_riccati_retry sweep a phase whose two half-waves are live on one trot mask (FR + HL
or FL + HR in stance) with a loop that has the mask compiled in and issues only the structurally
non-zero multiply-adds of B_c and of A - I's omega rows; HSDDP_SWEEP_MASKS=0 keeps every phase on
the runtime-mask loop.  Every surviving multiply-add keeps its operands and its place in the
accumulation order, and an omitted fma(x, +-0, acc) changes nothing for finite x (but the sign of
an exact zero), so on finite, converging inputs the two must agree bit for bit: gains, dU,
trajectories and every branch decision.  (The non-finite paths are test_gpu_divergence.py's.)

Every case runs with HSDDP_SWEEP_SPLIT=0, so that small batches take the one-wave kernel, and
solves the same problem with HSDDP_SWEEP_MASKS 1 and 0.  Shapes: the smallest at which the
dispatch or the loop can go wrong (each was solved by the oracle first: status 0, finite rows).
"""
import ctypes

import numpy as np
import pytest

import hsddp
from hsddp import synthetic as syn

pytestmark = pytest.mark.gpu

ARRAYS = ("K", "dU", "Xbar", "Ubar")
INFO = ("status", "iters", "n_ls_trials", "cost", "outer_iters")


def _solve(prob, weights=None, fp32=False, **kw):
    s = hsddp.Solver(prob, hsddp.load_settings(**kw), weights=weights, riccati_fp32=fp32)
    s.solve()
    out = {**s.trajectory(), **s.working(), **s.element_info()}
    s.close()
    return out


def _both(monkeypatch, prob, **kw):
    """The solve with the specialised loops and with the runtime-mask loop alone."""
    monkeypatch.setenv("HSDDP_SWEEP_SPLIT", "0")
    monkeypatch.setenv("HSDDP_SWEEP_MASKS", "1")
    a = _solve(prob, **kw)
    monkeypatch.setenv("HSDDP_SWEEP_MASKS", "0")
    b = _solve(prob, **kw)
    return a, b


def _same(a, b):
    for f in ARRAYS + INFO:
        assert np.array_equal(a[f], b[f]), f
    assert np.all(np.isfinite(a["K"])) and np.all(np.isfinite(a["Xbar"]))


def _trot(B, horizons):
    """A trot batch with its own horizon per phase (make_batch's assembly; its phases are equal)."""
    P, Kc = len(horizons), sum(horizons)
    sched = syn.phase_schedule("trot", P)
    rx, ru, rf = syn._reference_slots(sched, list(horizons), syn.DT)
    return {"batch": B, "horizons": list(horizons), "dt": syn.DT, "S": rx.shape[0], "Kc": Kc, "gaits": ["trot"] * B,
            "contacts": np.ascontiguousarray(np.tile(np.array(sched, dtype=np.int32), (B, 1, 1))),
            "x0": np.stack([syn.initial_state(b, sched[0]) for b in range(B)]),
            "ref_x": rx[None].copy(), "ref_u": ru[None].copy(), "ref_foot": rf[None].copy(),
            "Xbar": np.ascontiguousarray(np.tile(rx, (B, 1, 1))), "Ubar": np.zeros((B, Kc, 24)), "K": None}


def _stack(idx, P, N, gait):  # test_gpu_parity.py's
    ps = [syn.make_batch(1, P, N, gait, first_element=i) for i in idx]
    q = dict(ps[0]); q["batch"] = len(idx)
    for k in ("contacts", "x0", "Xbar", "Ubar"):
        q[k] = np.concatenate([p[k] for p in ps])
    return q


def test_trot_masks_are_the_instantiated_ones():
    """The two masks the sweep instantiates are what synthetic.py's trot alternates between, in the
    contacts array's leg order (bit l of Phase::cmask = leg l in stance)."""
    masks = {sum(int(c != 0) << l for l, c in enumerate(row)) for row in syn.make_batch(1, 4, 5, "trot")["contacts"][0]}
    assert masks == {0b1001, 0b0110}


def test_odd_batch(monkeypatch):
    """B = 3: the last wave's second half is borrowed and inactive (its phases stay generic)."""
    _same(*_both(monkeypatch, syn.make_batch(3, 4, 5, "trot")))


def test_one_and_two_knot_phases(monkeypatch):
    """Phases of 1 and 2 knots: a first knot that is the last one (no next image to request), and
    the request-one-ahead bookkeeping at its shortest."""
    _same(*_both(monkeypatch, _trot(2, [1, 2, 1, 2])))


def test_mixed_gaits_per_element_layouts(monkeypatch):
    """mixed=True with per-element layouts: pace, bound and jump elements (flight and full-stance
    phases) — every phase takes the generic branch of the dispatch."""
    prob = syn.make_batch(6, 4, 10, "trot", mixed=True, jump_layout=True)
    assert "layouts" in prob and "jump" in prob["gaits"]
    _same(*_both(monkeypatch, prob))


def test_pairs_of_unequal_masks(monkeypatch):
    """Per-element layouts with trot elements among them: a trot pair (specialised), a trot paired
    with a pace element (the halves' masks differ in every phase: generic) and a jump pair (equal
    halves on masks without a loop of their own: generic), in one sweep."""
    lays = [("trot", 4, 10), ("trot", 4, 10), ("trot", 4, 10), ("pace", 4, 10), ("jump", 8, 5), ("jump", 8, 5)]
    _same(*_both(monkeypatch, syn.make_layout_batch(lays)))


@pytest.mark.parametrize("sequential", [False, True])
def test_regularisation_retries(monkeypatch, sequential):
    """test_gpu_parity.py::test_parallel_retry_equals_sequential's inputs (jump elements whose
    sweeps fail the PSD test in inner iterations 9-12): the parallel retries (k_riccati_retry) and
    the in-kernel attempt loop."""
    if sequential:
        monkeypatch.setenv("HSDDP_SEQUENTIAL_RETRY", "1")
    prob = _stack([377, 760, 656, 321, 0], 8, 25, "jump")
    a, b = _both(monkeypatch, prob, no_early_exit=1, max_AL_iter=1, max_DDP_iter=12)
    for f in ARRAYS + INFO:
        assert np.array_equal(a[f], b[f]), f


@pytest.mark.parametrize("sequential", [False, True])
def test_trot_retries(monkeypatch, sequential):
    """Trot elements whose every first sweep fails (test_gpu_parity.py::test_retries_match_oracle's
    r_qJd = -0.5): the retry kernel's specialised phases, and a failed half (not live) beside a
    live one in the attempt loop."""
    if sequential:
        monkeypatch.setenv("HSDDP_SEQUENTIAL_RETRY", "1")
    w = hsddp.Weights()
    hsddp._lib.lib().hsddp_default_weights(ctypes.byref(w))
    w.r_qJd = -0.5
    a, b = _both(monkeypatch, syn.make_batch(4, 2, 10, "trot"), weights=w, no_early_exit=1, max_AL_iter=1,
                 max_DDP_iter=3)
    _same(a, b)
    assert np.all(a["status"] == 0) and np.all(a["iters"] > 0)


def test_two_pairs_per_workgroup(monkeypatch):
    """HSDDP_SWEEP_WPB=2: k_riccati<..., 2>, whose loops are allocated for one wave per SIMD."""
    monkeypatch.setenv("HSDDP_SWEEP_WPB", "2")
    _same(*_both(monkeypatch, syn.make_batch(5, 4, 5, "trot")))


def test_fp32_sweep(monkeypatch):
    _same(*_both(monkeypatch, syn.make_batch(4, 4, 5, "trot"), fp32=True))


def test_single_shooting(monkeypatch):
    """MS = 0: the DV instantiations keep the inlined runtime-mask loop, so the
    switch must change nothing."""
    a, b = _both(monkeypatch, syn.make_batch(4, 4, 5, "trot"), MS=0)
    _same(a, b)
    assert np.array_equal(a["merit"], b["merit"])
