"""Weight sets and references shared by the per-robot weights tests (hsddp_set_element_weights).

The problems are terrain_case.py's (Kc = 40: the shared layout 4 x 10 with B = 5, the mix of 4 x 10
and 8 x 5 layouts with B = 6, warm-start controls with pyramid rows on both sides of delta), the
handle's weights solver_params.WEIGHTS, the constraint parameters solver_params.CPARAMS.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

import solver_params as SP
import terrain_case as TC
from hsddp import synthetic as syn

# the field groups of hsddp_hkd_weights, as one robot at a time changes them (test 2)
GROUPS = (("q_eul",), ("q_pos",), ("q_omega",), ("q_v",), ("q_qJ",), ("qf_scale",), ("qf_gain",), ("r_grf",), ("r_qJd",),
          ("foot_w",), ("foot_gain",), ("foot_term_cost", "foot_term_grad"))
FIELDS = tuple(f for g in GROUPS for f in g)
assert set(FIELDS) == set(SP.WEIGHTS)

# five sets (robot b takes set b mod 5): every field of SP.WEIGHTS times a factor of its own per set,
# none of them 1, so each set differs from SP.WEIGHTS — and from the other sets — in every group
_FACTORS = (
    (1.30, 0.80, 1.15, 0.85, 1.40, 0.90, 1.10, 1.25, 0.75, 1.20, 0.85, 1.15, 0.90),
    (0.75, 1.20, 0.85, 1.25, 0.70, 1.10, 0.90, 0.80, 1.30, 0.85, 1.20, 0.80, 1.25),
    (1.10, 1.35, 0.70, 1.10, 1.20, 1.25, 1.30, 1.15, 1.10, 0.70, 1.10, 1.30, 1.10),
    (0.90, 0.70, 1.30, 0.75, 0.85, 0.80, 0.75, 0.90, 0.85, 1.35, 0.75, 0.90, 0.70),
    (1.20, 1.10, 0.90, 1.35, 1.10, 1.15, 1.20, 0.70, 1.20, 1.10, 1.30, 0.75, 1.35),
)


def _scaled(field, f):
    v = SP.WEIGHTS[field]
    return tuple(float(a) * f for a in v) if isinstance(v, tuple) else float(v) * f


def weight_set(k: int) -> dict:
    return {field: _scaled(field, _FACTORS[k % 5][j]) for j, field in enumerate(FIELDS)}


def robot_sets(B: int) -> list:
    """robot b on set b mod 5"""
    return [weight_set(b % 5) for b in range(B)]


def group_sets() -> list:
    """test 2's 13 robots: robot g < 12 differs from SP.WEIGHTS in GROUPS[g] alone (each field of
    the group times 1.5), robot 12 is SP.WEIGHTS (it is left unset)"""
    out = []
    for g in GROUPS:
        out.append({**SP.WEIGHTS, **{f: _scaled(f, 1.5) for f in g}})
    return out + [dict(SP.WEIGHTS)]


def rows(sets) -> list:
    """weight dicts -> hsddp.Weights"""
    return [SP.hsddp_weights(w) for w in sets]


def as_bytes(w) -> bytes:
    return bytes(C.string_at(C.addressof(w), C.sizeof(w)))


def gpu_solver(prob: dict, options: dict, weights: dict | None = None, fp32: bool = False):
    """a handle created with `weights` (None: SP.WEIGHTS) at SP.CPARAMS"""
    import hsddp
    return hsddp.Solver(prob, hsddp.load_settings(**options), cparams=SP.hsddp_cparams(),
                        weights=SP.hsddp_weights(weights), riccati_fp32=fp32)


def oracle_robots(prob: dict, options: dict, sets, x0_scale: float = 1.0) -> dict:
    """oracle_lib.solve_batch once per robot with weights = sets[b], stacked at the batch's strides
    (terrain_case.oracle_robots with the weights, not the constraint parameters, per robot)."""
    import oracle_lib as O
    B, S, P = prob["batch"], prob["S"], TC.stride_P(prob)
    out = {}
    for hz, idx in syn.layout_groups(prob).items():
        sub = syn.sub_batch(prob, idx, hz) if prob.get("layouts") is not None else dict(prob)
        if x0_scale != 1.0:
            sub["x0"] = sub["x0"] * x0_scale
        for j, b in enumerate(idx):
            r = O.solve_batch(sub, O.default_options(**options), elements=[j], weights=sets[b], cparams=SP.oracle_cparams())
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


def robot_of(g: dict, b: int) -> dict:
    """robot b's part of a handle's downloads (terrain_case.downloads)"""
    return {k: np.asarray(v)[b] for k, v in g.items()}
