"""hsddp_simulate_policy's semantics (include/hsddp.h) in NumPy on the oracle's primitives.

The pseudo-code of the header, knot by knot: O.hkd_step and O.resetmap for the model, O.knot_eval
(AL and ReB off) for the running cost l and the terminal cost Phi, orc_foot_position for the
touchdown heights, the friction-pyramid rows from mu_fric, and the dense gains K as
Solver.trajectory() returns them.  The loop for n_steps is a prefix of the loop for any larger
count, so `simulate` records every knot's running totals and the state after it, and `prefix`
reads off the outputs of a call with fewer steps.
"""
from __future__ import annotations

import numpy as np

import oracle_lib as O

MU_FRIC = 0.7        # hsddp_default_constraint_params / O.default_problem
GROUND_HEIGHT = 0.0
BOUND = 1e6          # SinglePhase.cpp:205-208


def grf_rows(f, mu=MU_FRIC):
    """GRFConstraint's A_leg f (HKDConstraints.cpp:13-18)."""
    return np.array([f[2], -f[0] + mu * f[2], f[0] + mu * f[2], -f[1] + mu * f[2], f[1] + mu * f[2]])


def foot_height(x, leg):
    p = np.zeros(3)
    x = np.ascontiguousarray(x, dtype=np.float64)
    O.lib().orc_foot_position(int(leg), O.dp(x[3:6].copy()), O.dp(x[0:3].copy()), O.dp(x[12 + 3 * leg:15 + 3 * leg].copy()),
                              O.dp(p))
    return p[2]


def element_layouts(prob):
    """[B] lists of horizons (per-element layouts, else the shared one)."""
    return [list(h) for h in (prob.get("layouts") or [prob["horizons"]] * prob["batch"])]


def simulate(prob, traj, x_init, n_steps, mu=MU_FRIC, ground=GROUND_HEIGHT, weights=None):
    """weights: cost-weight overrides by field name (O.knot_eval's); mu, ground: the handle's
    mu_fric and ground_height.  prob: horizons / layouts, contacts [B][Pmax+1][4], dt, ref_x, ref_u [Bref][S][24], ref_foot
    [Bref][S][12]; traj: Xbar [B][S][24], Ubar [B][Kc][24], K [B][Kc][24][24]; x_init [B][M][24].
    Returns X, U [B][M][n][24] (zero past a diverged sample's break knot), after [B][M][n][24] (the
    state after knot j, through the reset map at a phase end with a successor), the running totals
    cost, min_grf, max_td [B][M][n] after knot j, and steps, status [B][M]."""
    x_init = np.asarray(x_init, dtype=np.float64)
    B, M = x_init.shape[:2]
    n = int(n_steps)
    lays = element_layouts(prob)
    opt = O.default_options(AL_active=0, ReB_active=0)
    dt = float(prob["dt"])
    out = {"X": np.zeros((B, M, n, 24)), "U": np.zeros((B, M, n, 24)), "after": np.zeros((B, M, n, 24)),
           "cost": np.zeros((B, M, n)), "min_grf": np.full((B, M, n), np.inf), "max_td": np.zeros((B, M, n)),
           "steps": np.zeros((B, M), np.int32), "status": np.zeros((B, M), np.int32), "x_init": x_init.copy()}
    for b in range(B):
        hz = lays[b]
        P = len(hz)
        rb = 0 if prob["ref_x"].shape[0] == 1 else b
        rx, ru, rf = prob["ref_x"][rb], prob["ref_u"][rb], prob["ref_foot"][rb]
        Xbar, Ubar, K = traj["Xbar"][b], traj["Ubar"][b], traj["K"][b]
        cs = np.asarray(prob["contacts"][b], dtype=np.int32)
        # control knot kc -> (phase i, knot k, state slot s)
        walk = []
        s0 = 0
        for i, N in enumerate(hz):
            walk += [(i, k, s0 + k) for k in range(N)]
            s0 += N + 1
        for m in range(M):
            x = x_init[b, m].copy()
            cost, min_grf, max_td = 0.0, np.inf, 0.0
            for j in range(n):
                i, k, s = walk[j]
                c, cn = cs[i], cs[i + 1]
                with np.errstate(all="ignore"):
                    u = Ubar[j] + K[j] @ (x - Xbar[s])
                    out["X"][b, m, j], out["U"][b, m, j] = x, u
                    xs = O.hkd_step(x, u, dt, c.astype(float))
                    ok = np.sqrt(np.sum(xs * xs)) <= BOUND
                if not ok:  # (a NaN compares false: diverged)
                    out["status"][b, m] = 1
                    break
                ev = O.knot_eval(c, cn, x, u, rx[s], ru[s], rf[s], options=opt, dt=dt, weights=weights)
                cost += ev["l"]
                for leg in range(4):
                    if c[leg]:
                        min_grf = min(min_grf, float(np.min(grf_rows(u[3 * leg:3 * leg + 3], mu))))
                out["steps"][b, m] = j + 1
                x = xs
                if k == hz[i] - 1:
                    ev = O.knot_eval(c, cn, x, np.zeros(24), rx[s + 1], ru[s + 1], rf[s + 1], x_end=x, xr_end=rx[s + 1],
                                     pf_end=rf[s + 1], options=opt, dt=dt, weights=weights)
                    cost += ev["Phi"]
                    for leg in range(4):
                        if c[leg] == 0 and cn[leg] == 1:
                            max_td = max(max_td, abs(foot_height(x, leg) - ground))
                    if i + 1 < P:
                        x = O.resetmap(x, c, cn)
                out["after"][b, m, j] = x
                out["cost"][b, m, j], out["min_grf"][b, m, j], out["max_td"][b, m, j] = cost, min_grf, max_td
    return out


def prefix(ref, n):
    """The outputs of the call with n_steps = n <= the simulated count: x_end, cost, min_grf,
    max_td, steps, status, X, U."""
    steps = np.minimum(ref["steps"], n)
    status = np.where((ref["status"] == 1) & (ref["steps"] < n), 1, 0).astype(np.int32)
    B, M = steps.shape
    out = {"steps": steps.astype(np.int32), "status": status, "X": ref["X"][:, :, :n].copy(), "U": ref["U"][:, :, :n].copy(),
           "x_end": ref["x_init"].copy(), "cost": np.zeros((B, M)), "min_grf": np.full((B, M), np.inf),
           "max_td": np.zeros((B, M))}
    for b in range(B):
        for m in range(M):
            j = steps[b, m] - 1
            if j >= 0:
                out["x_end"][b, m] = ref["after"][b, m, j]
                for f in ("cost", "min_grf", "max_td"):
                    out[f][b, m] = ref[f][b, m, j]
    return out
