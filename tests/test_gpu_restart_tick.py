"""The mixed tick (T4): some robots in their HKDMPCSolver::initialize, the rest in their ::update, in
one solve — advance + restart + per-robot budgets + x0 from measured states + solve + commands —
written twice: over the C-ABI with the Python mirror, and through HKDMPCSolver::restart of the C++
facade (tests/drivers/restart_facade).  Both drive the same device code, so every command field of
every tick is equal bit for bit (solve_time excepted: a wall-clock reading), and so is the handle's
state after every tick: Xbar, Ubar and the element info.  A restarted robot's mpc_time starts from 0
as after initialize(): in the tick of its restart its mpc_times are k dt_mpc exactly.

B = 6 robots on the trot file at a plan of 0.2 s (Kc = 20), six ticks, robots 1 and 4 restarted in
the fourth at windows whose layouts have three phases while the others have two; B = 5 with robot 1
restarted, one half of a sweep pair (the robots start on one layout) whose partner is kept; B = 1;
every robot restarted, onto their own layouts; no robot (an empty restart: the budgets are cleared
and nothing else happens).
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hkd-mpc_amd")
PLAN = 0.2


def _records(ticks, B):
    """[ticks][B] measured states near the nominal stance (hsddp_robot_state, float32)"""
    import hsddp
    rng = np.random.default_rng(31)
    r = np.zeros((ticks, B), dtype=hsddp.ROBOT_STATE)
    r["p"] = np.array([0.0, 0.0, 0.25]) + rng.uniform(-1, 1, (ticks, B, 3)) * np.array([0.01, 0.01, 0.005])
    r["rpy"] = rng.uniform(-.02, .02, (ticks, B, 3))
    r["omegaBody"] = rng.uniform(-.1, .1, (ticks, B, 3))
    r["vWorld"] = rng.uniform(-.1, .1, (ticks, B, 3))
    r["qJ"] = np.tile([0.0, -0.8, 1.6], 4) + rng.uniform(-.02, .02, (ticks, B, 12))
    r["foot_placements"] = np.float32([.2, -.14, 0, .2, .14, 0, -.2, -.14, 0, -.2, .14, 0])
    return r


def _hkd_state(hsddp, x, contact):
    """compute_hkd_state (HKDModel.h:65-96): stance legs' qdummy = foot position (device FK)."""
    B = x.shape[0]
    pos = hsddp.model.foot_position(np.repeat(x, 4, axis=0), np.tile(np.arange(4), B)).reshape(B, 4, 3)
    out = x.copy()
    for b in range(B):
        for leg in range(4):
            if contact[b][leg]:
                out[b, 12 + 3 * leg:15 + 3 * leg] = pos[b, leg]
    return out


ELEMENT_INFO = np.dtype([(n, np.float64) for n in ("cost", "feas", "merit", "max_tconstr", "max_pconstr")] +
                        [(n, np.int32) for n in ("iters", "outer_iters", "status", "n_ls_trials")], align=True)


def _states(path, ticks, B):
    """restart_facade's state.bin: per tick (Xbar [B][S][24], Ubar [B][Kc][24], element info [B])"""
    raw = open(path, "rb").read()
    out, at = [], 0
    for _ in range(ticks):
        S, Kc = np.frombuffer(raw, np.int32, 2, at); at += 8
        Xb = np.frombuffer(raw, np.float64, B * S * 24, at).reshape(B, S, 24); at += Xb.nbytes
        Ub = np.frombuffer(raw, np.float64, B * Kc * 24, at).reshape(B, Kc, 24); at += Ub.nbytes
        info = np.frombuffer(raw, ELEMENT_INFO, B, at); at += info.nbytes
        out.append((Xb, Ub, info))
    assert at == len(raw)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("B,restart", [(6, {1: 21, 4: 43}), (5, {1: 21}), (1, {0: 21}),
                                       (6, {0: 40, 1: 21, 2: 43, 3: 5, 4: 17, 5: 30}), (6, {})],
                         ids=["two_of_six", "pair_of_five", "single", "all", "none"])
def test_facade_restart_matches_the_c_abi_tick(tmp_path, B, restart):
    import hsddp
    r = subprocess.run(["make", "-C", os.path.join(ROOT, "tests", "drivers"), "-f", "restart.mk", "restart_facade"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ticks, at = 6, 4
    ref_csv = os.path.join(ROOT, "tests", "golden", "ref_trot.csv")
    info_file = os.path.join(PKG, "settings", "ddp_setting.info")
    rec = _records(ticks, B)
    rec.tofile(os.path.join(tmp_path, "states.bin"))
    with open(os.path.join(tmp_path, "restart.txt"), "w") as f:
        f.write("".join(f"{b} {w}\n" for b, w in restart.items()))
    r = subprocess.run([os.path.join(ROOT, "tests", "drivers", "restart_facade"), ref_csv, info_file, str(tmp_path),
                        str(B), str(ticks), str(at), repr(PLAN)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(os.path.join(tmp_path, "commands.bin"), dtype=hsddp.MPC_COMMAND).reshape(ticks, B)
    states = _states(os.path.join(tmp_path, "state.bin"), ticks, B)
    assert ELEMENT_INFO.itemsize == C.sizeof(hsddp.ElementInfo)

    # the same ticks over the C-ABI
    tab, dt = hsddp.load_quad_reference(ref_csv)
    x0 = np.zeros((B, 24)); x0[:, 5] = 0.2486
    x0[:, 12:] = np.tile([0.0, -0.8, 1.6], 4)
    p = hsddp.reference_problem(tab, dt, [0] * B, x0, plan_duration=PLAN)
    p["x0"] = _hkd_state(hsddp, x0, p["contacts"][:, 0])
    full = hsddp.load_settings(info_file)
    s = hsddp.Solver(p, full)
    s.solve()
    dt_mpc = float(np.float32(0.01))
    phases = []
    for t in range(1, ticks + 1):
        s.set_options(hsddp.load_settings(info_file, max_AL_iter=2, max_DDP_iter=1))
        s.advance(None, 1, PLAN, dt_mpc)
        if t == at and restart:
            mask, ws = np.zeros(B, np.int32), np.zeros(B, np.int32)
            al, ddp = np.full(B, 2, np.int32), np.full(B, 1, np.int32)
            for b, w in restart.items():
                mask[b], ws[b], al[b], ddp[b] = 1, w, full.max_AL_iter, full.max_DDP_iter
            s.restart_elements(mask, ws, None, PLAN, dt_mpc)
            s.set_element_budgets(al, ddp)
        else:
            s.set_element_budgets(None, None)
        s.update_problem_measured(rec[t - 1])
        s.solve()
        cmd = s.extract_commands_measured(1, 0.01 * t, dt_mpc, None, 0.0)
        if t == at:  # a restarted robot's time starts from 0, as after initialize()
            for b in restart:
                for k in range(int(cmd[b]["N_mpcsteps"])):
                    cmd["mpc_times"][b, k] = k * dt_mpc
        if t > at:  # ... and counts on from there
            for b in restart:
                for k in range(int(cmd[b]["N_mpcsteps"])):
                    cmd["mpc_times"][b, k] = (0.01 * t - 0.01 * at) + k * dt_mpc
        phases.append(list(s.element_layouts()["n_phases"]))
        e = s.element_info()
        tr = s.trajectory()
        Xb, Ub, info = states[t - 1]
        assert Xb.shape == tr["Xbar"].shape and np.array_equal(Xb, tr["Xbar"]), t
        assert np.array_equal(Ub, tr["Ubar"]), t
        for f in ELEMENT_INFO.names:
            assert np.array_equal(info[f], e[f], equal_nan=True), (t, f)
        if t == at and 0 < len(restart) < B:  # the two budgets ran side by side
            assert all(e["outer_iters"][b] <= 2 for b in range(B) if b not in restart)
            assert full.max_AL_iter * full.max_DDP_iter > 2
        for b in range(B):
            for f in ("N_mpcsteps", "mpc_times", "hkd_controls", "des_body_state", "contacts", "statusTimes",
                      "foot_placement", "feedback"):
                assert np.array_equal(got[t - 1][b][f], cmd[b][f]), (t, b, f)
    s.close()
    for b in restart:
        assert got[at - 1][b]["mpc_times"][0] == 0.0 and got[at][b]["mpc_times"][0] > 0.0
    if (B, len(restart)) == (6, 2):  # the restarted robots' layouts differed from the others'
        assert len(set(phases[at - 1])) > 1, phases
