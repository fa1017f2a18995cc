"""Batches for the restart tests (test infrastructure for tests/test_gpu_restart.py): robots on the
reference's own trot and flytrot files (tests/golden/ref_*.csv, one table holding both), every
element with its own window, at a plan of 0.2 s — Kc = 20 control knots, two or three phases per
element with flight phases, touchdowns and reset maps, and layouts that differ between elements
and change from tick to tick.  These are the smallest problems with all of that (the argument of
tests/solver_params.py for Kc = 20)."""
import os

import numpy as np

import hsddp

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
PLAN = 0.2
N_WIN = 22  # QuadReference::initialize: round(0.2 / 0.01) + 2 samples
TICK = dict(max_AL_iter=2, max_DDP_iter=1)  # HKDMPCSolver::update's budget (quirk A17)


def table():
    """(table, dt, n_trot): trot's samples, then flytrot's"""
    t1, dt = hsddp.load_quad_reference(os.path.join(GOLD, "ref_trot.csv"))
    t2, _ = hsddp.load_quad_reference(os.path.join(GOLD, "ref_flytrot.csv"))
    return np.concatenate([t1, t2]), dt, len(t1)


def x0(B, seed=3):
    rng = np.random.default_rng(seed)
    x = np.zeros((B, 24))
    x[:, 5] = 0.25
    x[:, 12:] = np.float32([.2, -.14, 0, .2, .14, 0, -.2, -.14, 0, -.2, .14, 0])
    x[:, :3] += rng.uniform(-.05, .05, (B, 3))
    x[:, 6:12] += rng.uniform(-.2, .2, (B, 6))
    return x


def solver(tab, dt, starts, x, fp32=False, **opts):
    p = hsddp.reference_problem(tab, dt, starts, x, plan_duration=PLAN)
    assert p["Kc"] == 20
    return hsddp.Solver(p, hsddp.load_settings(**opts), riccati_fp32=fp32)


def snapshot(s):
    """everything a handle holds of its elements that a caller can read"""
    out = {**s.trajectory(), **s.working(), **s.element_info(), **s.constraint_params(), **s.constraint_values(),
           **s.references(), **s.phase_info()}
    si = s.solver_info(16)
    out.update({"hist_" + k: v for k, v in si.items()})
    lay = s.element_layouts()
    out.update(horizons=lay["horizons"], shooting=lay["shooting"], reach_end=lay["reach_end"])
    out["_P"], out["_S"] = s.P, s.S
    return out


SLOT_ROWS = ("Xbar", "X", "Defect", "dX", "ref_x", "ref_u", "ref_foot")  # [B][S][..]: the element's own S_b
KNOT_ROWS = ("Ubar", "K", "U", "dU", "reb_delta", "reb_eps", "grf_g")     # [B][Kc][..]
PHASE_ROWS = ("td_mask", "al_sigma", "al_lambda", "td_h", "durations")    # [B][P][..]: the element's own P_b
SCALARS = ("cost", "feas", "merit", "max_tconstr", "max_pconstr", "iters", "outer_iters", "status", "n_ls_trials")
LISTS = ("horizons", "shooting", "reach_end")
HISTS = ("hist_cost", "hist_dyn_feas", "hist_eqn_feas", "hist_ineq_feas")


def differences(a, b, ea, eb=None, shared_refs=False):
    """the fields in which element ea of snapshot a differs from element eb of snapshot b (bit for
    bit), whatever the two handles' strides: the rows past an element's own phases and slots are
    padding"""
    eb = ea if eb is None else eb
    bad = [f for f in LISTS if list(a[f][ea]) != list(b[f][eb])]
    if bad:
        return bad  # (different layouts: the rows do not correspond)
    P = len(a["horizons"][ea])
    S = sum(n + 1 for n in a["horizons"][ea])
    for f in SLOT_ROWS:
        ra, rb = (0 if shared_refs and f.startswith("ref_") else e for e in (ea, eb))
        if not np.array_equal(a[f][ra][:S], b[f][rb][:S], equal_nan=True):
            bad.append(f)
    bad += [f for f in KNOT_ROWS + SCALARS + HISTS if not np.array_equal(a[f][ea], b[f][eb], equal_nan=True)]
    bad += [f for f in PHASE_ROWS if not np.array_equal(a[f][ea][:P], b[f][eb][:P], equal_nan=True)]
    if not np.array_equal(a["contacts"][ea][:P + 1], b["contacts"][eb][:P + 1]):
        bad.append("contacts")
    return bad


def same_element(a, b, ea, eb=None, shared_refs=False):
    bad = differences(a, b, ea, eb, shared_refs)
    assert not bad, (ea, bad)
