#!/usr/bin/env python3
"""MPC tick benchmark: the reference's HKDMPCSolver::update loop for a
batch of robots driven by the reference's trot data (tests/golden/ref_trot.csv, 0.6 s plan =
60 knots), per tick: hsddp_advance (HKDProblem::update: host bookkeeping, k_shift_gather,
k_build_refs, inputs), hsddp_solve with max_AL_iter = 2, max_DDP_iter = 1 (quirk A17), and
hsddp_extract_commands (k_extract_commands).  Every C-ABI call returns synchronised, so the
wall-clock split is per stage; kernel durations come from rocprofv3 over the same script.

    python tools/mpc_bench.py [--batch B] [--ticks T]     -> one JSON line

--closed-loop puts the plant on the device: each tick's x0 is the solved policy simulated for the
tick's step (hsddp_simulate_policy, one sample per robot), handed over by
hsddp_update_problem_simulated after an advance with pending inputs; the plant's time per tick
is reported beside advance (which then includes that hand-over) and solve.

--host-state and --measured feed both the same measured robot records (hsddp_robot_state, seeded)
tick by tick and time the two ways from a record to the handle's x0: --host-state is the caller's
route without the ingest (advance with pending inputs, phase_info's contacts, the foot-position
primitive on 4 B replicated rows, update_problem(None, x0)); --measured is advance +
update_problem_measured, with the commands from extract_commands_measured.  "advance" is then the
whole of it, "state" the part after hsddp_advance.

--restart-frac F restarts a seeded set of round(F B) robots (at least one when F > 0) every tick at
the sample their windows have reached (hsddp_restart_elements between the advance with pending
inputs and update_problem(None, x0)): the handle then has per-robot reference windows, also at
F = 0 (an empty mask), and "restart" is the call's time per tick beside advance (which includes
the x0 update) and solve.  "reupload_all" is the only route without the call — hsddp_upload_problem
+ hsddp_upload_warm_start of the whole batch — timed the same way after the ticks.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch  # noqa: F401  (binds the library to torch's HIP runtime, as bench.py does)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hkd-mpc_amd"))
import hsddp  # noqa: E402


def robot_records(rng, B):
    """[B] measured states near the nominal stance (hsddp_robot_state, all float32)"""
    r = np.zeros(B, dtype=hsddp.ROBOT_STATE)
    r["p"] = np.array([0.0, 0.0, 0.25]) + rng.uniform(-1, 1, (B, 3)) * np.array([0.01, 0.01, 0.005])
    r["rpy"] = rng.uniform(-.02, .02, (B, 3))
    r["omegaBody"] = rng.uniform(-.1, .1, (B, 3))
    r["vWorld"] = rng.uniform(-.1, .1, (B, 3))
    r["qJ"] = np.tile([0.0, -0.8, 1.6], 4) + rng.uniform(-.02, .02, (B, 12))
    r["foot_placements"] = np.float32([.2, -.14, 0, .2, .14, 0, -.2, -.14, 0, -.2, .14, 0])
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--ticks", type=int, default=20)
    ap.add_argument("--sync", action="store_true",
                    help="synchronous extraction into pageable memory (round 3's path) instead of the "
                         "asynchronous copy into the handle's pinned buffers")
    ap.add_argument("--closed-loop", action="store_true",
                    help="x0 of every tick from the policy simulated on the device instead of host noise")
    ap.add_argument("--host-state", action="store_true",
                    help="x0 of every tick formed on the host from measured records (the route without the ingest)")
    ap.add_argument("--measured", action="store_true",
                    help="x0 of every tick formed on the device from the same records (update_problem_measured)")
    ap.add_argument("--restart-frac", type=float, default=None,
                    help="restart this fraction of the robots every tick (per-robot reference windows; 0: an empty mask)")
    ap.add_argument("--terrain", action="store_true",
                    help="per-phase terrain (set_terrain): a random friction coefficient in [0.3, 0.9] per robot and a "
                         "ground height within +-0.03 per phase, the whole table set again every tick after the advance")
    ap.add_argument("--weights", action="store_true",
                    help="per-robot cost weights (set_element_weights): every field of each robot's row drawn within "
                         "+-30 %% of the defaults, the whole table set again every tick after the advance")
    ap.add_argument("--phase-weights", action="store_true",
                    help="per-phase cost weights (set_phase_weights): every field of each (robot, phase) row drawn "
                         "within +-30 %% of the defaults; every tick after the advance the table the phases carried on is "
                         "read back and set again with the phases that entered given rows of their own")
    args = ap.parse_args()
    if args.host_state + args.measured + args.closed_loop + (args.restart_frac is not None) + args.terrain + args.weights + args.phase_weights > 1:
        ap.error("--host-state, --measured, --closed-loop, --restart-frac, --terrain, --weights and --phase-weights are separate legs")
    B = args.batch
    tab, dt = hsddp.load_quad_reference(os.path.join(ROOT, "tests", "golden", "ref_trot.csv"))
    rng = np.random.default_rng(7)
    x0 = np.zeros((B, 24))
    x0[:, 5] = 0.25
    x0[:, 12:] = np.tile(np.float32([.2, -.14, 0, .2, .14, 0, -.2, -.14, 0, -.2, .14, 0]), 1)
    x0[:, 6:12] += rng.uniform(-.2, .2, (B, 6))
    restarts = args.restart_frac is not None
    p = hsddp.reference_problem(tab, dt, [0] * B if restarts else [0], x0)
    s = hsddp.Solver(p, hsddp.load_settings())
    s.solve()
    s.set_options(hsddp.load_settings(max_AL_iter=2, max_DDP_iter=1))
    feet = np.tile(np.float32([.2, -.14, 0, .2, .14, 0, -.2, -.14, 0, -.2, .14, 0]), (B, 1))
    t_adv, t_solve, t_cmd, t_plant, t_state, t_restart, t_terrain = [], [], [], [], [], [], []
    if args.terrain:
        rng_t = np.random.default_rng(13)
        s.set_terrain(np.repeat(rng_t.uniform(0.3, 0.9, (B, 1)), s.P, axis=1), rng_t.uniform(-0.03, 0.03, (B, s.P)))
    t_weights, rows = [], None
    if args.weights:
        import ctypes
        rng_w = np.random.default_rng(17)
        base = hsddp.Weights()
        hsddp.lib().hsddp_default_weights(ctypes.byref(base))
        n = ctypes.sizeof(hsddp.Weights) // 8
        vals = np.frombuffer(ctypes.string_at(ctypes.addressof(base), 8 * n), np.float64) * rng_w.uniform(0.7, 1.3, (B, n))
        rows = np.ascontiguousarray(vals)  # [B][46]: passed on as it stands
        s.set_element_weights(rows)
    t_pw, pw_base, rng_p = [], None, np.random.default_rng(19)
    if args.phase_weights:
        import ctypes
        base = hsddp.Weights()
        hsddp.lib().hsddp_default_weights(ctypes.byref(base))
        n = ctypes.sizeof(hsddp.Weights) // 8
        pw_base = np.frombuffer(ctypes.string_at(ctypes.addressof(base), 8 * n), np.float64)
        s.set_phase_weights(np.ascontiguousarray(pw_base * rng_p.uniform(0.7, 1.3, (B, s.P, n))))  # [B][P][46]
    n_restart = 0
    if restarts and args.restart_frac > 0:
        n_restart = min(B, max(1, int(round(args.restart_frac * B))))
    rng_r = np.random.default_rng(11)
    legs = np.tile(np.arange(4, dtype=np.int32), B)
    plant_ok = True
    flags = 0
    ticket, cmd, t_last = None, None, 0.0
    for it in range(args.ticks):
        if args.closed_loop:
            tp = time.perf_counter()
            plant = s.simulate_policy(None, 1)
            t0 = time.perf_counter()
            t_plant.append(t0 - tp)
            plant_ok = plant_ok and bool(np.all(plant["summary"]["status"] == 0))
            flags += sum(s.advance(None, 1))
            s.update_problem_simulated(0)
        elif args.host_state or args.measured:
            rec = robot_records(rng, B)
            feet = rec["foot_placements"]
            t0 = time.perf_counter()
            flags += sum(s.advance(None, 1))
            ts = time.perf_counter()
            if args.measured:
                s.update_problem_measured(rec)
            else:  # compute_hkd_state by hand: every robot's row once per leg through the primitive
                c0 = s.phase_info()["contacts"][:, 0]
                xt = np.zeros((B, 24))
                xt[:, 0:3], xt[:, 3:6] = rec["rpy"][:, ::-1], rec["p"]
                xt[:, 6:9], xt[:, 9:12], xt[:, 12:] = rec["omegaBody"], rec["vWorld"], rec["qJ"]
                fp = hsddp.model.foot_position(np.repeat(xt, 4, axis=0), legs).reshape(B, 12)
                on = np.repeat(c0 != 0, 3, axis=1)
                xt[:, 12:][on] = fp[on]
                s.update_problem(None, xt)
            t_state.append(time.perf_counter() - ts)
        elif restarts:
            xt = x0 + rng.uniform(-.01, .01, x0.shape)
            mask = np.zeros(B, np.int32)
            mask[rng_r.choice(B, n_restart, replace=False)] = 1
            ws = np.full(B, it + 1, np.int32)  # the sample every robot's window has reached
            t0 = time.perf_counter()
            flags += sum(s.advance(None, 1))
            tr = time.perf_counter()
            s.restart_elements(mask, ws)
            t_restart.append(time.perf_counter() - tr)
            s.update_problem(None, xt)
        elif args.terrain:  # advance -> set_terrain -> x0 -> solve (the table goes up with the solve's first launch)
            xt = x0 + rng.uniform(-.01, .01, x0.shape)
            t0 = time.perf_counter()
            flags += sum(s.advance(None, 1))
            tt = time.perf_counter()
            t = s.terrain()  # the rows the phases carried on; a phase that entered took the last one's
            s.set_terrain(t["mu"], t["ground"])
            t_terrain.append(time.perf_counter() - tt)
            s.update_problem(None, xt)
        elif args.weights:  # advance -> set_element_weights -> x0 -> solve (the rows go up with the solve's first launch)
            xt = x0 + rng.uniform(-.01, .01, x0.shape)
            t0 = time.perf_counter()
            flags += sum(s.advance(None, 1))
            tw = time.perf_counter()
            rows[it % B, 12] *= 1.0 + 1e-9  # (q_qJ of one robot: an unchanged table is not uploaded again)
            s.set_element_weights(rows)
            t_weights.append(time.perf_counter() - tw)
            s.update_problem(None, xt)
        elif args.phase_weights:  # advance -> set_phase_weights -> x0 -> solve (the table goes up with the solve's first launch)
            xt = x0 + rng.uniform(-.01, .01, x0.shape)
            t0 = time.perf_counter()
            flags += sum(s.advance(None, 1))
            tw = time.perf_counter()
            rows, is_set = s.phase_weights()  # the overrides the phases carried on; a phase that entered has none
            new = is_set == 0
            rows[new] = pw_base * rng_p.uniform(0.7, 1.3, (int(new.sum()), rows.shape[2]))
            rows[it % B, 0, 12] *= 1.0 + 1e-9  # (q_qJ of one phase: an unchanged table is not uploaded again)
            s.set_phase_weights(rows)
            t_pw.append(time.perf_counter() - tw)
            s.update_problem(None, xt)
        else:
            xt = x0 + rng.uniform(-.01, .01, x0.shape)
            t0 = time.perf_counter()
            flags += sum(s.advance(xt, 1))
        t1 = time.perf_counter()
        s.solve()
        t2 = time.perf_counter()
        info = None if args.measured else s.phase_info()
        t3 = time.perf_counter()
        if args.measured:  # feet and durations from the handle
            cmd = s.extract_commands_measured(1, 0.01 * (it + 1), float(np.float32(0.01)), None, 0.0)
        elif args.sync:
            cmd = s.extract_commands(1, 0.01 * (it + 1), float(np.float32(0.01)), info["durations"], feet, 0.0)
        else:  # the records of tick t cross PCIe during tick t + 1's advance and solve
            if ticket is not None:
                cmd = s.commands_wait(ticket, copy=False)
            ticket = s.extract_commands_async(1, 0.01 * (it + 1), float(np.float32(0.01)), info["durations"], feet,
                                              0.0)
        t4 = time.perf_counter()
        t_adv.append(t1 - t0); t_solve.append(t2 - t1); t_cmd.append(t4 - t3)
    if not args.sync and not args.measured:
        t5 = time.perf_counter()
        cmd = s.commands_wait(ticket, copy=False)
        t_last = time.perf_counter() - t5
    lay = s.element_layouts() if restarts else s.layout()
    if restarts:
        lay = {"horizons": [int(v) for v in lay["horizons"][0]]}
    finite = bool(np.isfinite(s.element_info()["cost"]).all()) and bool(np.isfinite(cmd["hkd_controls"]).all())
    S, Kc = sum(n + 1 for n in lay["horizons"]), sum(lay["horizons"])
    # k_shift_gather moves every element's warm start once: Xbar [S][24], Ubar [Kc][24] and the
    # compact gains [Kc][12][24] read (gathered) and written
    shift_bytes = 2 * B * (S * 24 + Kc * 24 + Kc * 12 * 24) * 8
    med = lambda v: float(np.median(v)) * 1e3  # noqa: E731
    out = {"metric": "MPC tick (advance + solve + extract), HKD trot reference file", "batch": B,
           "ticks": args.ticks, "plan_knots": Kc, "final_horizons": lay["horizons"], "contact_change_steps": flags,
           "ms_per_tick_median": {"advance": med(t_adv), "solve": med(t_solve), "extract_commands": med(t_cmd)},
           "extract_mode": "sync (pageable)" if args.sync or args.measured else "async (pinned, overlapped with the next tick)",
           "last_copy_wait_ms": t_last * 1e3,
           "robot_ticks_per_s": B / (np.median(t_adv) + np.median(t_solve) + np.median(t_cmd)),
           "shift_gather_algorithmic_bytes": shift_bytes, "all_finite": finite}
    if args.closed_loop:
        out["metric"] = "closed-loop MPC tick (plant + advance + solve + extract), HKD trot reference file"
        out["ms_per_tick_median"]["plant"] = med(t_plant)
        out["plant_all_ok"] = plant_ok
    if restarts:
        out["metric"] = "MPC tick with restarts (advance + restart + x0 + solve + extract), HKD trot reference file"
        out["restarted_per_tick"] = n_restart
        out["ms_per_tick_median"]["advance"] = med(np.array(t_adv) - np.array(t_restart))
        out["ms_per_tick_median"]["restart"] = med(t_restart)
        t_up = []
        for _ in range(5):  # the whole batch as a new problem: hsddp_upload_problem + hsddp_upload_warm_start
            c = s.phase_info()["contacts"]
            tu = time.perf_counter()
            s.upload_problem(c, x0)
            s.warm_start()
            t_up.append(time.perf_counter() - tu)
        out["ms_per_tick_median"]["reupload_all"] = med(t_up)
    if args.weights:
        out["metric"] = "MPC tick with per-robot weights (advance + set_element_weights + x0 + solve + extract), HKD trot reference file"
        out["ms_per_tick_median"]["advance"] = med(np.array(t_adv) - np.array(t_weights))
        out["ms_per_tick_median"]["weights"] = med(t_weights)
    if args.phase_weights:
        out["metric"] = "MPC tick with per-phase weights (advance + phase_weights + set_phase_weights + x0 + solve + extract), HKD trot reference file"
        out["ms_per_tick_median"]["advance"] = med(np.array(t_adv) - np.array(t_pw))
        out["ms_per_tick_median"]["phase_weights"] = med(t_pw)
        out["phase_weight_overrides"] = int(s.phase_weights()[1].sum())
    if args.terrain:
        out["metric"] = "MPC tick with per-phase terrain (advance + set_terrain + x0 + solve + extract), HKD trot reference file"
        out["ms_per_tick_median"]["advance"] = med(np.array(t_adv) - np.array(t_terrain))
        out["ms_per_tick_median"]["terrain"] = med(t_terrain)
        t = s.terrain()
        out["terrain_mu_range"] = [float(t["mu"].min()), float(t["mu"].max())]
    if args.host_state or args.measured:
        out["metric"] = ("MPC tick from measured robot states, x0 formed on the %s, HKD trot reference file"
                         % ("device (update_problem_measured)" if args.measured else "host (foot-position primitive)"))
        out["ms_per_tick_median"]["state"] = med(t_state)
    print(json.dumps(out), flush=True)
    s.close()


if __name__ == "__main__":
    main()
