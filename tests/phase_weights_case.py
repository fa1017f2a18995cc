"""Rows, tables and references shared by the per-phase weights tests (hsddp_set_phase_weights).

The problems are terrain_case.py's shapes (Kc = 40: the shared layout 4 x 10 with B = 5, the mix of
4 x 10 and 8 x 5 layouts with B = 6) and a pronk of the shared shape (phases alternate 1111 / 0000),
the handle's weights solver_params.WEIGHTS, the constraint parameters solver_params.CPARAMS.
"""
from __future__ import annotations

import numpy as np

import element_weights_case as EW
import solver_params as SP
import terrain_case as TC
from hsddp import synthetic as syn

NW = 46


def vec(w: dict) -> np.ndarray:
    """a weight dict as the 46 doubles of hsddp_hkd_weights"""
    return np.frombuffer(EW.as_bytes(SP.hsddp_weights(w)), np.float64).copy()


def pronk_problem() -> dict:
    prob = syn.make_batch(5, 4, 10, "pronk")
    prob["Ubar"] = TC.warm_controls(prob)
    return prob


def table(prob: dict, rows, fill=None) -> np.ndarray:
    """rows[b][i] (weight dicts, robot b's own phases) as the setter's [B][P][46] array; entries past
    a robot's phases hold `fill` (SP.WEIGHTS): they are not read"""
    B, P = prob["batch"], TC.stride_P(prob)
    t = np.tile(vec(fill or SP.WEIGHTS), (B, P, 1))
    for b in range(B):
        for i, w in enumerate(rows[b]):
            t[b, i] = vec(w)
    return np.ascontiguousarray(t)


def own_mask(prob: dict) -> np.ndarray:
    """[B][P]: 1 on every robot's own phases"""
    B, P = prob["batch"], TC.stride_P(prob)
    m = np.zeros((B, P), np.int32)
    for b, hz in enumerate(TC.phases_of(prob)):
        m[b, :len(hz)] = 1
    return m


def _factor(u):
    return 0.7 + 0.6 * u


def phase_rows(prob: dict, seed: int = 11) -> list:
    """a distinct row for every (robot, phase): each field of SP.WEIGHTS times a factor of its own in
    [0.7, 1.3) (foot_w's zero z entry gets a value in [0.5, 1.1) instead: nothing stays zero)"""
    rng = np.random.default_rng(seed)
    out = []
    for hz in TC.phases_of(prob):
        robot = []
        for _ in hz:
            w = {}
            for f in EW.FIELDS:
                v = SP.WEIGHTS[f]
                if isinstance(v, tuple):
                    w[f] = tuple(float(a) * _factor(rng.random()) if a else 0.5 + 0.6 * rng.random() for a in v)
                else:
                    w[f] = float(v) * _factor(rng.random())
            robot.append(w)
        out.append(robot)
    return out


# ---- test 1: fields a phase's contact masks out ----------------------------------------------------
def masked_rows(prob: dict, sets, swap: bool = False) -> list:
    """Robot b's phases on sets[b] with the fields their contact multiplies by zero replaced: a stance
    phase (1111) by other q_qJ and qf_scale[12..23], a flight phase (0000) by other foot_w, foot_gain,
    foot_term_cost and foot_term_grad.  swap: the replacements exchanged between stance and flight
    rows — each phase then reads a replaced value where it is not masked."""
    out = []
    for b in range(prob["batch"]):
        w = sets[b]
        stance = {**w, "q_qJ": w["q_qJ"] * 3.0 + 0.1, "qf_scale": tuple(w["qf_scale"][:12]) + tuple(v * 2.5 + 0.02 for v in w["qf_scale"][12:])}
        flight = {**w, "foot_w": tuple(v * 1.8 + 0.4 for v in w["foot_w"]), "foot_gain": w["foot_gain"] * 1.7,
                  "foot_term_cost": w["foot_term_cost"] * 0.6, "foot_term_grad": w["foot_term_grad"] * 1.5}
        robot = []
        for i in range(len(TC.phases_of(prob)[b])):
            c = prob["contacts"][b, i]
            assert c.all() or not c.any(), "pronk: all feet down or none"
            robot.append((stance if bool(c.all()) != swap else flight))
        out.append(robot)
    return out


# ---- test 2: the oracle's LQ terms with each phase's row, and a dense sweep over them ----------------
def knot_terms(prob: dict, b: int, W: dict, rows, opts: dict) -> dict:
    """oracle_lib.knot_eval over robot b's knots and phase ends at the working rows W with phase i's
    weights rows[i]: A, B, l, lx, lu, lxx, luu per control slot, Phi, Phix, Phixx, Px per phase"""
    import oracle_lib as O
    hz = TC.phases_of(prob)[b]
    rb = 0 if prob["ref_x"].shape[0] == 1 else b
    o = O.default_options(**opts)
    out = {k: [] for k in ("A", "B", "l", "lx", "lu", "lxx", "luu", "Phi", "Phix", "Phixx", "Px")}
    s = kc = 0
    z = np.zeros(24)
    for i, n in enumerate(hz):
        c, cn = prob["contacts"][b, i], prob["contacts"][b, i + 1]
        kw = dict(options=o, dt=prob["dt"], weights=rows[i], cparams=SP.oracle_cparams())
        for k in range(n):
            e = O.knot_eval(c, cn, W["X"][b, s + k], W["U"][b, kc], prob["ref_x"][rb, s + k], prob["ref_u"][rb, s + k],
                            prob["ref_foot"][rb, s + k], **kw)
            for f in ("A", "B", "l", "lx", "lu", "lxx", "luu"):
                out[f].append(np.array(e[f]))
            kc += 1
        e = O.knot_eval(c, cn, z, z, z, z, np.zeros(12), W["X"][b, s + n], prob["ref_x"][rb, s + n], prob["ref_foot"][rb, s + n], **kw)
        for f in ("Phi", "Phix", "Phixx"):
            out[f].append(np.array(e[f]))
        out["Px"].append(O.resetmap_partial(W["X"][b, s + n], c, cn) if i + 1 < len(hz) else np.zeros((24, 24)))
        s += n + 1
    return {k: np.array(v) for k, v in out.items()}


def dense_sweep(hz, T: dict, Defect: np.ndarray, reg: float = 0.0) -> dict:
    """SinglePhase::backward_sweep and the linear rollout (eps = 1) over the LQ terms T (knot_terms) with
    numpy.linalg, as tests/numpy_riccati.py forms them: the gains K, the feed-forward dU (what
    hsddp_download_working returns as dU), the linear rollout's dX, (G, H) at each phase start, and the
    smallest eigenvalue of any knot's Quu (the sweep's PSD test asks for more than 1e-9: the LDLT of
    Quu - 1e-9 I).  reg: the regularisation mu added to Qxx and Quu (a retried sweep's)."""
    P = len(hz)
    s0 = np.cumsum([0] + [n + 1 for n in hz]); k0 = np.cumsum([0] + list(hz))
    K = [None] * k0[-1]; kff = [None] * k0[-1]
    G0 = H0 = None
    V = [None] * P
    I = np.eye(24)
    min_eig = np.inf
    for i in reversed(range(P)):
        if i == P - 1:
            G, H = T["Phix"][i].copy(), T["Phixx"][i].copy()
        else:
            Px = T["Px"][i]
            G, H = T["Phix"][i] + Px.T @ G0, T["Phixx"][i] + Px.T @ H0 @ Px
        for k in reversed(range(hz[i])):
            kc = k0[i] + k
            A, B = T["A"][kc], T["B"][kc]
            Gn = G + H @ Defect[s0[i] + k + 1]
            Qx = T["lx"][kc] + A.T @ Gn; Qu = T["lu"][kc] + B.T @ Gn
            Qxx = T["lxx"][kc] + A.T @ H @ A + reg * I
            Quu = T["luu"][kc] + B.T @ H @ B + reg * I
            Qux = B.T @ H @ A
            min_eig = min(min_eig, float(np.linalg.eigvalsh((Quu + Quu.T) / 2).min()))
            Qi = np.linalg.inv(Quu); Qi = (Qi + Qi.T) / 2; Qxx = (Qxx + Qxx.T) / 2
            kff[kc] = -Qi @ Qu
            K[kc] = -Qi @ Qux
            G = Qx - Qux.T @ Qi @ Qu
            H = Qxx - Qux.T @ Qi @ Qux
        G0, H0 = G + H @ Defect[s0[i]], H
        V[i] = (G0, H0)
    dX = np.zeros((s0[-1], 24))
    dx_init = np.zeros(24)
    for i in range(P):
        if i > 0:
            dx_init = T["Px"][i - 1] @ dX[s0[i - 1] + hz[i - 1]]
        dX[s0[i]] = dx_init + Defect[s0[i]]
        for k in range(hz[i]):
            s, kc = s0[i] + k, k0[i] + k
            du = kff[kc] + K[kc] @ dX[s]
            dX[s + 1] = T["A"][kc] @ dX[s] + T["B"][kc] @ du + Defect[s + 1]
    return {"K": np.array(K), "dU": np.array(kff), "dX": dX, "G": np.array([v[0] for v in V]), "H": np.array([v[1] for v in V]),
            "min_eig": min_eig}
