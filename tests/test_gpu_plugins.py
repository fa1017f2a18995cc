"""The HKD cost / constraint plugins on the device (C-ABI hsddp_hkd_running_cost / _terminal_cost /
_grf_constraint / _touchdown_constraint — the bodies of the C++ facade's hkd:: CostBase,
PathConstraintBase and TerminalConstraintBase plugins) against the oracle's knot evaluation.

The reference splits a knot's cost over plugins (HKDTrackingCost + HKDFootPlaceReg running costs,
HKDCost.h:8-99; the GRF constraint's relaxed barrier added by SinglePhase, ConstraintsBase.h:
201-263 / SinglePhase.cpp:380-394); the oracle (orc_knot_eval) evaluates the sum, so the plugin
terms plus the barrier assembled here from the plugin's g, gu must equal it."""
import numpy as np
import pytest

import hsddp
import oracle_lib as O
import solver_params as SP
from hsddp import model
from test_oracle_pinning import CASES, _control, _refs, _state, _height_and_grad

DT = 0.01


def _close(a, b, tol=1e-12):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.max(np.abs(a - b)) <= tol * max(1.0, np.max(np.abs(b)))


# the second variant of every plugin test: solver_params.WEIGHTS, mu = 0.4, ground = 0.02, dt = 0.02
NONDEFAULT = dict(weights=SP.WEIGHTS, cparams=SP.CPARAMS, DT=0.02)


def _running_plugins_sum_to_the_oracle_knot(c, cn, seed, weights=None, cparams=None, DT=DT):
    x, u = _state(c, seed), _control(c, seed)
    xr, ur, pf = _refs(c)
    r = O.knot_eval(c, cn, x, u, xr, ur, pf, weights=weights, cparams=cparams, dt=DT)
    kw = dict(dt=DT, weights=None if weights is None else SP.hsddp_weights(weights))
    rc = {k: v[0] for k, v in model.running_cost(x, u, c, xr, ur, pf, **kw).items()}
    track = {k: v[0] for k, v in model.running_cost(x, u, c, xr, ur, pf, terms=model.TERM_TRACKING, **kw).items()}
    foot = {k: v[0] for k, v in model.running_cost(x, u, c, xr, ur, pf, terms=model.TERM_FOOT, **kw).items()}
    for k in ("lx", "lu", "lxx", "luu"):   # the terms are additive (RCostData::add)
        assert _close(track[k] + foot[k], rc[k], 1e-15), k
    n = 5 * int(sum(c))
    if cparams is None:
        g, gu = model.grf_constraint(u, c)
        cp = hsddp.load_constraint_params()
        delta, eps = cp.grf_delta, cp.grf_eps
    else:
        g, gu = model.grf_constraint(u, c, mu=cparams["mu_fric"])
        delta, eps = cparams["grf_delta"], cparams["grf_eps"]
    barr = bd = 0.0
    lu, luu = rc["lu"].copy(), rc["luu"].copy()
    rb = 0.0
    for i in range(n):
        gi = g[0, i]
        if gi > delta:
            b, d1, d2 = -np.log(gi), -1.0 / gi, gi ** -2.0
        else:
            t = (gi - 2 * delta) / delta
            b, d1, d2 = .5 * (t * t - 1) - np.log(delta), (gi - 2 * delta) / delta / delta, delta ** -2.0
        rb += eps * b
        lu += DT * eps * d1 * gu[0, i]
        luu += DT * eps * d2 * np.outer(gu[0, i], gu[0, i])
    assert np.all(g[0, n:] == 0) and np.all(gu[0, n:] == 0)
    l = rc["l"] + (DT * rb if n else 0.0)
    assert _close(l, r["l"], 1e-13)
    assert _close(rc["lx"], r["lx"]) and _close(rc["lxx"], r["lxx"])
    assert _close(lu, r["lu"]) and _close(luu, r["luu"])


@pytest.mark.gpu
@pytest.mark.parametrize("c,cn,seed", CASES)
def test_running_plugins_sum_to_the_oracle_knot(c, cn, seed):
    _running_plugins_sum_to_the_oracle_knot(c, cn, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("c,cn,seed", CASES)
def test_running_plugins_sum_to_the_oracle_knot_at_nondefault_parameters(c, cn, seed):
    _running_plugins_sum_to_the_oracle_knot(c, cn, seed, **NONDEFAULT)


def _terminal_plugins_match_the_oracle(c, seed, weights=None):
    x = _state(c, seed)
    xr, ur, pf = _refs(c)
    r = O.knot_eval(c, c, x, np.zeros(24), xr, ur, pf, x_end=x, weights=weights)   # no touchdown: no AL terms
    w = None if weights is None else SP.hsddp_weights(weights)
    t = {k: v[0] for k, v in model.terminal_cost(x, c, xr, pf, weights=w).items()}
    assert _close(t["Phi"], r["Phi"], 1e-13)
    assert _close(t["Phix"], r["Phix"]) and _close(t["Phixx"], r["Phixx"])


TERMINAL_CASES = [((1, 0, 0, 1), 5), ((1, 1, 1, 1), 6), ((0, 0, 0, 0), 7), ((0, 1, 1, 1), 10), ((0, 0, 0, 1), 11)]


@pytest.mark.gpu
@pytest.mark.parametrize("c,seed", TERMINAL_CASES)
def test_terminal_plugins_match_the_oracle(c, seed):
    _terminal_plugins_match_the_oracle(c, seed)


@pytest.mark.gpu
@pytest.mark.parametrize("c,seed", TERMINAL_CASES)
def test_terminal_plugins_match_the_oracle_at_nondefault_weights(c, seed):
    _terminal_plugins_match_the_oracle(c, seed, SP.WEIGHTS)


TOUCHDOWN_PAIR = ((1, 0, 0, 1), (1, 1, 1, 1), (1, 2))    # legs 1 and 2 touch down
# a single leg between stance neighbours; three legs at once (the rows follow the legs' order)
TOUCHDOWN_ODD = [((1, 1, 0, 1), (1, 1, 1, 1), (2,)), ((0, 1, 0, 0), (1, 1, 1, 1), (0, 2, 3))]


def _touchdown_plugin_matches_foot_kinematics(ground, c=TOUCHDOWN_PAIR[0], cn=TOUCHDOWN_PAIR[1], legs=TOUCHDOWN_PAIR[2]):
    assert legs == tuple(l for l in range(4) if not c[l] and cn[l])
    x = _state(c, 11)
    h, hx = model.touchdown_constraint(x, c, cn, ground=ground)
    for row, leg in enumerate(legs):
        hr, hxr = _height_and_grad(x, leg)
        assert _close(h[0, row], hr - ground, 1e-13) and _close(hx[0, row], hxr, 1e-13)
    n = len(legs)
    assert np.all(h[0, n:] == 0) and np.all(hx[0, n:] == 0)


@pytest.mark.gpu
def test_touchdown_plugin_matches_foot_kinematics():
    _touchdown_plugin_matches_foot_kinematics(0.0)


@pytest.mark.gpu
def test_touchdown_plugin_matches_foot_kinematics_above_the_ground():
    _touchdown_plugin_matches_foot_kinematics(SP.CPARAMS["ground_height"])


@pytest.mark.gpu
@pytest.mark.parametrize("ground", [0.0, SP.CPARAMS["ground_height"]])
@pytest.mark.parametrize("c,cn,legs", TOUCHDOWN_ODD)
def test_touchdown_plugin_on_one_and_three_legs(c, cn, legs, ground):
    _touchdown_plugin_matches_foot_kinematics(ground, c, cn, legs)
