"""Shapes, values and references shared by the per-phase terrain tests (hsddp_set_terrain).

Kc = 40 throughout: the shared layout 4 x 10 (S = 44, so a 64-slot rollout wave straddles robots)
with B = 5, and a per-element mix of 4 x 10 trots and 8 x 5 jumps with B = 6 (a lone half wave of
the sweep, B P odd or not a multiple of the terminal tasks per block).  The solves run at
solver_params.WEIGHTS / CPARAMS from warm-start controls that put friction-pyramid rows on both
sides of delta (solver_params.warm_controls' construction, for any batch).
"""
from __future__ import annotations

import numpy as np

import solver_params as SP
from hsddp import synthetic as syn

# one (mu, ground) per robot (test 1); robot b takes entry b mod 5
MU = (0.3, 0.4, 0.55, 0.7, 0.9)
GROUND = (-0.03, 0.0, 0.02, 0.05, 0.01)

ARRAYS = ("Xbar", "Ubar", "K", "X", "U", "dX", "dU")
SCALARS = ("cost", "feas", "max_tconstr", "max_pconstr")
DECISIONS = ("iters", "outer_iters", "status", "n_ls_trials")
PARAMS = ("reb_delta", "reb_eps", "al_sigma", "al_lambda")


def rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(1e-300, np.max(np.abs(b))))


def warm_controls(prob: dict, gain: float = 0.002) -> np.ndarray:
    """solver_params.warm_controls for any batch and per-element layouts: Ubar[b, kc] = gain (kc % 3)
    ref_u[slot of kc] + 0.02 z, z drawn knot by knot from default_rng(5)."""
    B, Kc = prob["batch"], prob["Kc"]
    rng = np.random.default_rng(5)
    z = rng.standard_normal((Kc, B, 24))
    U = np.zeros((B, Kc, 24))
    lays = prob.get("layouts") or [prob["horizons"]] * B
    for b in range(B):
        rb = 0 if prob["ref_u"].shape[0] == 1 else b
        kc = s = 0
        for n in lays[b]:
            for k in range(n):
                U[b, kc] = gain * (kc % 3) * prob["ref_u"][rb, s + k] + 0.02 * z[kc, b]
                kc += 1
            s += n + 1
    return U


def shared_problem() -> dict:
    prob = syn.make_batch(5, 4, 10, "trot")
    prob["Ubar"] = warm_controls(prob)
    return prob


def mixed_problem() -> dict:
    lays = [("jump", 8, 5) if b % 2 else (("trot", "pace", "bound")[b // 2], 4, 10) for b in range(6)]
    prob = syn.make_layout_batch(lays)
    prob["Ubar"] = warm_controls(prob)
    return prob


PROBLEMS = {"shared4x10": shared_problem, "mixed4x10_8x5": mixed_problem}


def phases_of(prob: dict) -> list:
    """horizons of every element"""
    return [list(h) for h in (prob.get("layouts") or [prob["horizons"]] * prob["batch"])]


def stride_P(prob: dict) -> int:
    return max(len(h) for h in phases_of(prob))


def robot_terrain(prob: dict):
    """test 1's table: robot b's (MU, GROUND)[b mod 5] on every phase, [B][P] each"""
    B, P = prob["batch"], stride_P(prob)
    mu = np.array([[MU[b % 5]] * P for b in range(B)])
    gr = np.array([[GROUND[b % 5]] * P for b in range(B)])
    return mu, gr


def phase_terrain(prob: dict):
    """a distinct (mu, ground) for every (robot, phase): mu in [0.25, 0.95) away from the cparams'
    0.4 / 0.7 by at least 0.02, ground in +-0.04 away from 0 / 0.02 by at least 0.004"""
    B, P = prob["batch"], stride_P(prob)
    q = np.arange(B * P).reshape(B, P)
    mu = 0.25 + 0.7 * ((q * 37) % (B * P)) / (B * P)
    gr = -0.04 + 0.08 * ((q * 29 + 5) % (B * P)) / (B * P)
    for v in (0.4, 0.7):
        mu = np.where(np.abs(mu - v) < 0.02, mu + 0.04, mu)
    for v in (0.0, 0.02):
        gr = np.where(np.abs(gr - v) < 0.004, gr + 0.008, gr)
    return np.ascontiguousarray(mu), np.ascontiguousarray(gr)


def oracle_robots(prob: dict, options: dict, mu, ground, x0_scale: float = 1.0) -> dict:
    """oracle_lib.solve_batch once per robot with cparams = CPARAMS + {mu_fric: mu[b], ground_height:
    ground[b]} (one value per robot), stacked at the batch's strides (rows past a robot's S and P zero)."""
    import oracle_lib as O
    B, S, P = prob["batch"], prob["S"], stride_P(prob)
    out = {}
    for hz, idx in syn.layout_groups(prob).items():
        sub = syn.sub_batch(prob, idx, hz) if prob.get("layouts") is not None else dict(prob)
        if x0_scale != 1.0:
            sub["x0"] = sub["x0"] * x0_scale
        for j, b in enumerate(idx):
            cp = SP.oracle_cparams(mu_fric=float(mu[b]), ground_height=float(ground[b]))
            r = O.solve_batch(sub, O.default_options(**options), elements=[j], weights=SP.WEIGHTS, cparams=cp)
            for k, v in r.items():
                if k == "solver_info":
                    continue
                v = np.asarray(v)
                if k not in out:
                    shape = list(v.shape[1:])
                    if k in ("Xbar", "X", "Defect", "Defect_bar", "dX"):
                        shape[0] = S
                    if k in ("al_sigma", "al_lambda", "td_mask", "td_h"):
                        shape[0] = P
                    out[k] = np.zeros([B] + shape, v.dtype)
                out[k][(b,) + tuple(slice(0, n) for n in v.shape[1:])] = v[0]
    return out


def gpu_solver(prob: dict, options: dict, cparams: dict | None = None, fp32: bool = False):
    import hsddp
    return hsddp.Solver(prob, hsddp.load_settings(**options), cparams=SP.hsddp_cparams(cparams),
                        weights=SP.hsddp_weights(), riccati_fp32=fp32)


def downloads(s) -> dict:
    """everything a solve leaves that a caller can read, as arrays"""
    out = {**s.trajectory(), **s.working(), **s.element_info()}
    out.update({"p_" + k: v for k, v in s.constraint_params().items()})
    out.update({"v_" + k: v for k, v in s.constraint_values().items()})
    out.update({"lq_" + k: v for k, v in s.lq().items()})
    out.update({"tm_" + k: v for k, v in s.terminal().items()})
    return out


SLOT_KEYS = ("Xbar", "X", "Defect", "dX")
PHASE_KEYS = ("p_td_mask", "p_al_sigma", "p_al_lambda", "v_td_h", "tm_Phi", "tm_Phix", "tm_Phixx", "tm_Px")


def mask_padding(prob: dict, g: dict) -> dict:
    """downloads with the rows past each robot's own S and P zeroed (padding at the batch's strides)"""
    g = dict(g)
    for b, hz in enumerate(phases_of(prob)):
        S, P = sum(n + 1 for n in hz), len(hz)
        for k in SLOT_KEYS:
            g[k] = g[k].copy() if b == 0 else g[k]
            g[k][b, S:] = 0
        for k in PHASE_KEYS:
            g[k] = g[k].copy() if b == 0 else g[k]
            g[k][b, P:] = 0
    return g


# ---- the host bookkeeping, restated --------------------------------------------------------------
def move_rows(rows, phase_src, fill):
    """One robot's terrain rows after a shift: rows [P_old][2], phase_src[i] the old phase that new
    phase i continues (-1: started by the shift: it takes the row of the phase before it)."""
    out = []
    for i, src in enumerate(phase_src):
        out.append(list(rows[src]) if src >= 0 else (list(out[i - 1]) if i > 0 else list(fill)))
    return out
