"""Non-default cost weights and constraint parameters shared by the parameter tests, as data.

The shipped values coincide in many places (q_qJ = r_grf = q_omega = 0.2, q_pos[0] = q_pos[1],
qf_scale[12..23] all 0.01, qf_gain = foot_gain = foot_term_grad = 20 = 2 foot_term_cost, foot_w[2] = 0,
grf_delta = grf_delta_min, td_lambda = ground_height = 0), so a swapped index or a term dropped as
"structurally zero" computes the same numbers.  In WEIGHTS no two values are equal and none is zero;
in CPARAMS delta, delta_min and eps differ and the schedule's clamps are within reach of a few outer
iterations (0.05 * 0.1 < 0.01; 10 * 3^3 > 200).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

WEIGHTS = {
    "q_eul": (1.3, 4.7, 5.9), "q_pos": (1.1, 2.3, 31.0), "q_omega": (.21, .34, .55), "q_v": (4.1, 1.7, .6),
    "q_qJ": .27, "qf_scale": tuple(0.5 + 0.37 * j for j in range(24)), "qf_gain": 17.0, "r_grf": .13,
    "r_qJd": .19, "foot_w": (3.1, 1.9, 0.7), "foot_gain": 13.0, "foot_term_cost": 7.0, "foot_term_grad": 11.0,
}

CPARAMS = {"mu_fric": 0.4, "grf_delta": 0.05, "grf_delta_min": 0.01, "grf_eps": 0.01, "td_sigma": 10.0,
           "td_sigma_max": 200.0, "td_lambda": 0.3, "ground_height": 0.02}

# delta starts below its floor: the first outer update lifts it to grf_delta_min at any update_relax
CPARAMS_BELOW_MIN = {**CPARAMS, "grf_delta": 0.02, "grf_delta_min": 0.08}

# the non-uniform ReB / AL schedule (HSDDP_OPTION's defaults are 7 / 0.1; the shipped file has 1 / 1)
SCHEDULE = {"update_ReB": 7.0, "update_relax": 0.1, "update_penalty": 3.0}


def oracle_cparams(base: dict | None = None, **over) -> dict:
    """CPARAMS (or base, with overrides) as oracle_lib's `cparams` argument."""
    return {**(CPARAMS if base is None else base), **over}


def hsddp_weights(weights: dict | None = None, **over):
    """hsddp.Weights: the library's defaults overlaid with WEIGHTS (or `weights`) and overrides."""
    import hsddp
    w = hsddp.Weights()
    hsddp._lib.lib().hsddp_default_weights(C.byref(w))
    for k, v in {**(WEIGHTS if weights is None else weights), **over}.items():
        cur = getattr(w, k)
        if isinstance(cur, C.Array):
            assert len(v) == len(cur), k
            v = type(cur)(*[float(a) for a in v])
        setattr(w, k, v)
    return w


def hsddp_cparams(base: dict | None = None, **over):
    """hsddp.ConstraintParams: the library's defaults (the swing_* fields keep them) overlaid with
    CPARAMS (or base) and overrides."""
    import hsddp
    cp = hsddp.ConstraintParams()
    hsddp._lib.lib().hsddp_default_constraint_params(C.byref(cp))
    for k, v in oracle_cparams(base, **over).items():
        setattr(cp, k, float(v))
    return cp


def warm_controls(prob: dict, gain: float = 0.002) -> np.ndarray:
    """Warm-start controls [3][Kc][24] that put friction-pyramid rows on both sides of delta:
    Ubar[:, kc] = gain (kc % 3) ref_u[slot] + 0.02 z, z drawn knot by knot from default_rng(5).
    gain = 0.002 suits two stance legs (reference f_z = m g / 2: 0, 0.087, 0.175 against delta =
    0.05); a pronk's four share the weight, so it takes 0.004 for the same forces."""
    assert prob["batch"] == 3
    rng = np.random.default_rng(5)
    U = np.zeros((3, prob["Kc"], 24))
    kc = s = 0
    for n in prob["horizons"]:
        for k in range(n):
            z = rng.standard_normal((3, 24))
            for b in range(3):
                rb = 0 if prob["ref_u"].shape[0] == 1 else b
                U[b, kc] = gain * (kc % 3) * prob["ref_u"][rb, s + k] + 0.02 * z[b]
            kc += 1
        s += n + 1
    return U


def pyramid_rows(prob: dict, U: np.ndarray, mu: float) -> np.ndarray:
    """The friction-pyramid values of every stance leg at every knot of every element (1-D)."""
    out = []
    for b in range(prob["batch"]):
        kc = 0
        for i, n in enumerate(prob["horizons"]):
            for _ in range(n):
                for leg in range(4):
                    if prob["contacts"][b, i, leg]:
                        f = U[b, kc, 3 * leg:3 * leg + 3]
                        out += [f[2], -f[0] + mu * f[2], f[0] + mu * f[2], -f[1] + mu * f[2], f[1] + mu * f[2]]
                kc += 1
    return np.array(out)


# ---- the solver cases (tests/test_gpu_parameters.py; their oracle side in test_oracle_parameters.py) --
# B = 6 on the smallest shapes with touchdowns, resets, flight phases and per-element references
SHAPES = [("trot", 3, 6, False), ("jump", 8, 3, False), ("trot", 4, 5, True)]
SHAPE_IDS = ["trot3x6", "jump8x3", "mixed4x5"]
BATCH = 6


def shape_batch(gait, P, N, mixed, dt=0.01) -> dict:
    from hsddp import synthetic as syn
    return syn.make_batch(BATCH, P, N, gait, mixed=mixed, dt=dt)


_FIXED = {"no_early_exit": 1, "max_AL_iter": 3, "max_DDP_iter": 2}
_EXITS = {**SCHEDULE, "cost_thresh": 1e-1, "tconstr_thresh": 2e-3, "pconstr_thresh": 1e-2,
          "dynamics_feas_thresh": 5e-3, "max_AL_iter": 4, "max_DDP_iter": 4}


def _case(options, weights=WEIGHTS, cparams=CPARAMS, dt=0.01):
    return {"options": options, "weights": weights, "cparams": cparams, "dt": dt}


# name -> options (over the shipped settings), weights / cparams (None: the defaults), dt
CASES = {
    "schedule": _case({**_FIXED, **SCHEDULE}),
    "uniform": _case(dict(_FIXED)),  # update_ReB = update_relax = 1: the uniform-ReB fast path
    "below_min": _case(dict(_FIXED), cparams=CPARAMS_BELOW_MIN),
    "below_min_schedule": _case({**_FIXED, **SCHEDULE}, cparams=CPARAMS_BELOW_MIN),
    "al_off": _case({**_FIXED, "AL_active": 0}),
    "reb_off": _case({**_FIXED, "ReB_active": 0}),
    "both_off": _case({**_FIXED, "AL_active": 0, "ReB_active": 0}),
    "alpha_half": _case({"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 3, "alpha": 0.5, "gamma": 0.9},
                        None, None),
    "alpha_03": _case({"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 3, "alpha": 0.3, "gamma": 0.5},
                      None, None),
    "alpha_reject": _case({"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 2, "alpha": 0.5, "gamma": 1e6},
                          None, None),
    "merit": _case({"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 3, "merit_scale": 0.6,
                    "merit_offset": 3.0, "dynamics_feas_thresh": 1e-2}, None, None),
    "dt_coarse": _case({"no_early_exit": 1, "max_AL_iter": 2, "max_DDP_iter": 2}, dt=0.02),
    "dt_fine": _case({"no_early_exit": 1, "max_AL_iter": 2, "max_DDP_iter": 2}, dt=0.004),
    "retries": _case({"no_early_exit": 1, "max_AL_iter": 1, "max_DDP_iter": 3, "update_regularization": 3.0},
                     weights={**WEIGHTS, "r_qJd": -0.5}),
    "early_exits": _case(dict(_EXITS)),
    "single_shooting": _case({"no_early_exit": 1, "max_AL_iter": 2, "max_DDP_iter": 2, "MS": 0, **SCHEDULE}),
}


def oracle_solve(prob: dict, case: dict, x0_scale: float = 1.0) -> dict:
    """The oracle's solve of a case; x0_scale = 1 + 1e-15 gives its rounding envelope."""
    import oracle_lib as O
    if x0_scale != 1.0:
        prob = dict(prob); prob["x0"] = prob["x0"] * x0_scale
    return O.solve_batch(prob, O.default_options(**case["options"]), n_threads=8, weights=case["weights"],
                         cparams=case["cparams"])


def effective_cparams(case: dict) -> dict:
    """The case's constraint parameters by CPARAMS' keys (the shipped ones where it has none)."""
    if case["cparams"] is not None:
        return case["cparams"]
    import oracle_lib as O
    p, _ = O.default_problem([1])
    return {k: getattr(p, k) for k in O.CPARAM_FIELDS}


# ---- conditions under which a case exercises its path, from the oracle's outputs alone -----------
def schedule_fired(r: dict, cp: dict) -> bool:
    """update_REB_params moved the rows apart and the grf_delta_min clamp was hit."""
    return len(np.unique(r["reb_eps"])) > 1 and float(r["reb_delta"].min()) == cp["grf_delta_min"]


def floor_lifted_delta(r: dict, cp: dict) -> bool:
    """grf_delta < grf_delta_min: the clamp alone moves delta, to grf_delta_min."""
    return bool(np.any(r["reb_delta"] == cp["grf_delta_min"])) and cp["grf_delta"] < cp["grf_delta_min"]


def _td(r: dict, f: str) -> np.ndarray:
    """al_sigma / al_lambda of the registered touchdown constraints' legs."""
    m = (r["td_mask"][..., None] >> np.arange(4)) & 1
    return r[f][m == 1]


def sigma_capped(r: dict, cp: dict) -> bool:
    return float(_td(r, "al_sigma").max()) == cp["td_sigma_max"]


def sigma_took(r: dict, value: float) -> bool:
    return bool(np.any(_td(r, "al_sigma") == value))


def lambda_moved(r: dict, cp: dict) -> bool:
    return bool(np.any(_td(r, "al_lambda") != cp["td_lambda"]))


def iters_differ(r: dict) -> bool:
    """Early exits: the elements stop after different numbers of inner iterations."""
    return len(np.unique(r["iters"])) > 1


def outer_iters_differ(r: dict) -> bool:
    return len(np.unique(r["outer_iters"])) >= 2


CONDITIONS = {
    "schedule_fired": schedule_fired, "floor_lifted_delta": floor_lifted_delta, "sigma_capped": sigma_capped,
    "sigma_took_90": lambda r, cp: sigma_took(r, 90.0), "lambda_moved": lambda_moved,
    "iters_differ": lambda r, cp: iters_differ(r), "outer_iters_differ": lambda r, cp: outer_iters_differ(r),
    "reb_rows_moved": lambda r, cp: len(np.unique(r["reb_eps"])) > 1,
}

# case -> {condition: the shapes (SHAPE_IDS) it must hold on; None: all}.  Each entry held on the
# oracle when it was written; test_oracle_parameters.py keeps it so.  What these short solves do not
# reach: a multiplier update from td_lambda = 0.3 (the touchdown residuals stay above 0.005, so the
# penalty branch of update_al_params runs: ConstraintsBase.h:354-372) -- the multiplier branch runs
# in the cases on the shipped parameters, and the value 90 survives only where a constraint skips
# an update (3 updates take 10 to 30, 90 and the cap 200).
FIRED = {
    "schedule": {"schedule_fired": None, "sigma_capped": None},
    "uniform": {"sigma_capped": None},
    "below_min": {"floor_lifted_delta": None},
    "below_min_schedule": {"floor_lifted_delta": None, "reb_rows_moved": None},
    "alpha_half": {"lambda_moved": ("trot3x6",)},
    "alpha_03": {"lambda_moved": ("trot3x6", "mixed4x5")},
    "merit": {"lambda_moved": ("trot3x6", "jump8x3")},
    "early_exits": {"iters_differ": None, "outer_iters_differ": ("trot3x6", "jump8x3"), "schedule_fired": None,
                    "sigma_capped": None, "sigma_took_90": ("trot3x6",)},
    "single_shooting": {"sigma_took_90": None, "reb_rows_moved": ("jump8x3", "mixed4x5")},
}


def fired(name: str, shape_id: str, r: dict) -> dict:
    """{condition: bool} of the conditions FIRED sets for this case and shape, on the oracle's outputs."""
    cp = effective_cparams(CASES[name])
    return {c: bool(CONDITIONS[c](r, cp)) for c, where in FIRED.get(name, {}).items()
            if where is None or shape_id in where}
