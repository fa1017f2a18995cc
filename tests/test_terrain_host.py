"""The host side of the per-phase terrain (hsddp_set_terrain) without a GPU: the rows' moves through
hsddp_advance and hsddp_restart_elements on the reference's trot file (walk_advance, plan_restart_batch)
against oracle/ref_oracle.py's ProblemTracker with the rows riding on its phases, and through
caller-flagged shifts and arriving elements (plan_shift, plan_import_batch: no table, so no tracker)
against a restatement of HKDProblem::update's bookkeeping driven by the same flags
(hkd-mpc_amd/csrc/hsddp_phases.cpp: shift_terrain, put_terrain_rows, export_element;
tests/drivers/terrain_check is built from that one source); and the two symbols' prototypes and
NULL refusals."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "tests", "drivers")
sys.path.insert(0, os.path.join(ROOT, "hkd-mpc_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
KC, S_CAP = 20, 36
FILL = (0.7, 0.0125)


def _codes():
    hdr = open(os.path.join(ROOT, "include", "hsddp.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(HSDDP_(?:OK|ERR_[A-Z]+))\s*=\s*(-?\d+)", hdr)}


# ---- the restatement ------------------------------------------------------------------------------
def robot(b, N, reach=None):
    """robot b: horizons, reach flags, and its rows as the driver makes them"""
    N = list(N)
    return dict(N=N, reach=list(reach) if reach else [0] * len(N),
                rows=[[0.30 + (16 * b + i) / 256.0, -0.05 + (16 * b + i) / 2048.0] for i in range(len(N))])


def arriving(tag, N, reach=None):
    N = list(N)
    rows = None if tag < 0 else [[0.5 + (16 * tag + i) / 256.0, (16 * tag + i) / 1024.0] for i in range(len(N))]
    return dict(N=N, reach=list(reach) if reach else [0] * len(N), rows=rows, tag=tag)


def step(e, change):
    """one step of HKDProblem::update's bookkeeping (HKDProblem.cpp:117-222; PhaseStepper) with the
    terrain rows riding on the phases; the moves themselves are terrain_case.move_rows'"""
    import terrain_case as TC
    src = list(range(len(e["N"])))
    if e["N"][0] <= 1:
        e["N"].pop(0); e["reach"].pop(0); src.pop(0)
    else:
        e["N"][0] -= 1
    if change and e["reach"][-1]:
        e["N"].append(1); e["reach"].append(0); src.append(-1)
    else:
        e["N"][-1] += 1
        if change:
            e["reach"][-1] = 1
    e["rows"] = TC.move_rows(e["rows"], src, FILL)


def take(batch, dst, e):
    batch[dst] = dict(N=list(e["N"]), reach=list(e["reach"]),
                      rows=[list(r) for r in e["rows"]] if e["rows"] is not None else [list(FILL) for _ in e["N"]])


def expected(batch):
    P = max(len(e["N"]) for e in batch)
    return P, [sum(e["rows"] + [list(FILL)] * (P - len(e["N"])), []) for e in batch]


# ---- the driver ------------------------------------------------------------------------------------
def _line(e):
    return f"{len(e['N'])} {' '.join(map(str, e['N']))} {' '.join(map(str, e['reach']))}"


@pytest.fixture(scope="module")
def driver():
    r = subprocess.run(["make", "-C", DRIVERS, "-f", "terrain.mk", "terrain_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(DRIVERS, "terrain_check")


def run(driver, batch, elem, commands):
    """commands: ("shift", flags [B][n]) or ("take", [(dst, element)]); returns the states after the
    start and after each command as (P, rows [B][2 P], horizons [B])"""
    text = f"rows {KC} {S_CAP} {len(batch)} {int(elem)} {FILL[0]!r} {FILL[1]!r}\n" + "".join(_line(e) + "\n" for e in batch)
    for kind, arg in commands:
        if kind == "shift":
            text += f"shift {len(arg[0])}\n" + "".join(" ".join(map(str, f)) + "\n" for f in arg)
        else:
            text += f"take {len(arg)}\n" + "".join(f"{d} {e['tag']} {_line(e)}\n" for d, e in arg)
    return _states(driver, text, len(batch), len(commands))


def _states(driver, text, B, n_commands):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    states, lines = [], r.stdout.splitlines()
    assert not any(l.startswith(("refused", "export mismatch")) for l in lines), lines
    for q, l in enumerate(lines):
        if l.startswith("state"):
            P = int(re.search(r"P=(\d+)", l).group(1))
            els = [dict(w.split("=", 1) for w in m.split()[2:]) for m in lines[q + 1:q + 1 + B]]
            states.append((P, [[float(v) for v in e["rows"].split(",")] for e in els],
                           [[int(v) for v in e["N"].split(",")] for e in els]))
    assert len(states) == 1 + n_commands
    return states


def check(driver, batch, elem, commands):
    states = run(driver, batch, elem, commands)
    assert states[0][:2] == expected(batch)
    for (kind, arg), got in zip(commands, states[1:]):
        if kind == "shift":
            for e, flags in zip(batch, arg):
                for f in flags:
                    step(e, f)
        else:
            for d, e in arg:
                take(batch, d, e)
        P, rows = expected(batch)
        assert got[2] == [e["N"] for e in batch]
        assert got[0] == P and got[1] == rows, (kind, got, rows)
    return batch


def test_rows_ride_the_phases_through_shifts(driver):
    """Four robots of one 4 x 5 layout crossing phase boundaries at different steps: the row of a
    removed first phase is dropped, an appended phase takes the row of the robot's previous last
    phase (whatever the stride becomes), the others keep theirs; enough steps that every robot has
    dropped a first phase and appended a last one."""
    batch = [robot(b, [5, 5, 5, 5]) for b in range(4)]
    flags = [[[1, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 1], [1, 1, 0, 0]],
             [[0, 0, 0, 0], [1, 0, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0]],
             [[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0]]]
    after = check(driver, batch, False, [("shift", f) for f in flags])
    for b, e in enumerate(after):  # twelve steps: phases 0 and 1 are gone, the last one's row was inherited
        rows = robot(b, [5] * 4)["rows"]
        assert e["rows"][0] == rows[2] and e["rows"].count(rows[3]) >= 2, (b, e)


def test_one_flag_set_for_the_batch_keeps_the_shared_layout(driver):
    batch = [robot(b, [2, 8, 10]) for b in range(3)]
    f = [[0, 1, 1, 0, 0]] * 3
    after = check(driver, batch, False, [("shift", f), ("shift", [[0, 0, 0, 1, 1]] * 3)])
    assert all(e["N"] == after[0]["N"] for e in after)


def test_arriving_and_restarted_elements(driver):
    """A per-element batch: an element arrives with its rows in place; one arrives from a source
    without terrain and one restarts (cparams rows); one arrives with more phases than the stride
    (every robot's rows move to the new stride, the padding at cparams), then the stride shrinks
    again when it is replaced — and the shifts after that carry all of it on."""
    batch = [robot(0, [10, 10]), robot(1, [5, 5, 5, 5]), robot(2, [10, 10]), robot(3, [4, 16], [0, 1]), robot(4, [5, 5, 5, 5])]
    cmds = [("take", [(2, arriving(7, [10, 10]))]),
            ("take", [(0, arriving(-1, [10, 10])), (4, arriving(-1, [5, 5, 5, 5]))]),
            ("take", [(3, arriving(9, [2, 3, 3, 4, 4, 4], [0, 0, 0, 0, 0, 1]))]),
            ("shift", [[1, 0], [0, 0], [0, 1], [1, 0], [0, 0]]),
            ("take", [(3, arriving(5, [10, 10]))]),
            ("shift", [[0, 1], [1, 1], [0, 0], [0, 0], [1, 0]])]
    check(driver, batch, True, cmds)


def test_shared_batch_takes_an_element_of_another_layout(driver):
    batch = [robot(b, [10, 10]) for b in range(3)]
    check(driver, batch, False, [("take", [(1, arriving(3, [5, 5, 5, 5]))]), ("shift", [[0], [1], [0]])])


# ---- hsddp_advance and hsddp_restart_elements on the reference's trot file ---------------------------
sys.path.insert(0, os.path.join(ROOT, "oracle"))
PLAN, N_WIN, KC_T, S_CAP_T = 0.4, 42, 40, 56  # a 0.4 s plan: round(0.4 / 0.01) + 2 samples, Kc = 40
STARTS = [0, 4, 9, 15, 20]  # within 16 ticks every robot drops a first phase and appends a last one


class Tracked:
    """oracle/ref_oracle.py's ProblemTracker per robot with the terrain rows riding on its phases: a
    popped first phase drops its row, an appended phase takes the row of the phase before it, a
    restart gives the cparams pair"""

    def __init__(self):
        import ref_oracle as R
        self.R = R
        self.ref, self.dt = R.load_quad_reference(os.path.join(ROOT, "tests", "golden", "ref_trot.csv"))
        self.tk = [R.ProblemTracker(self.ref, w, self.dt, plan_duration=PLAN) for w in STARTS]
        self.rows = [robot(b, t.horizons)["rows"] for b, t in enumerate(self.tk)]
        self.events = [set() for _ in STARTS]

    def advance(self, n):
        import terrain_case as TC
        for b, t in enumerate(self.tk):
            for _ in range(n):
                n0, pop = len(t.horizons), t.horizons[0] <= 1
                t.step()
                app = len(t.horizons) - (n0 - pop)
                self.rows[b] = TC.move_rows(self.rows[b], list(range(int(pop), n0)) + [-1] * app, FILL)
                self.events[b] |= ({"pop"} if pop else set()) | ({"append"} if app else set())

    def restart(self, b, start):
        self.tk[b] = self.R.ProblemTracker(self.ref, start, self.dt, plan_duration=PLAN)
        self.rows[b] = [list(FILL) for _ in self.tk[b].horizons]

    def expected(self):
        P = max(len(r) for r in self.rows)
        return P, [sum(r + [list(FILL)] * (P - len(r)), []) for r in self.rows], [list(t.horizons) for t in self.tk]


def test_rows_ride_the_phases_through_advances_and_restarts(driver):
    """walk_advance's plan and plan_restart_batch on five robots whose windows start at different
    samples of the trot file: after every hsddp_advance (one step, and three at once) and every
    restart — of one robot in place, and of the robots that hold the batch's largest phase count, so
    that every robot's rows move to a smaller stride — the rows equal the ProblemTracker
    restatement's, and so do the layouts."""
    tr = Tracked()
    text = f"table {len(tr.ref)} {float(tr.dt)!r} {N_WIN} {PLAN!r} 0.01 0.01 {KC_T} {S_CAP_T} {FILL[0]!r} {FILL[1]!r}\n"
    text += "".join(" ".join(str(int(c)) for c in q["contact"]) + " " +
                    " ".join(repr(float(d)) for d in q["status_dur"]) + "\n" for q in tr.ref)
    text += f"{len(STARTS)}\n" + " ".join(map(str, STARTS)) + "\n"
    cmds = [("advance", 1)] * 12 + [("restart", [(1, 30)]), ("advance", 3), ("advance", 1), ("advance", 1), ("advance", 1)]
    cmds += [("restart", "widest"), ("advance", 1), ("advance", 1), ("advance", 1)]
    want = [tr.expected()]
    strides = []
    for kind, arg in cmds:
        if kind == "advance":
            text += f"advance {arg}\n"
            tr.advance(arg)
        else:
            if arg == "widest":  # the robots that hold the batch's largest phase count: the stride shrinks with them
                n = [len(r) for r in tr.rows]
                arg = [(b, 60) for b in range(len(n)) if n[b] == max(n)]
                assert len(arg) < len(n), n
            text += f"restart {len(arg)} " + " ".join(f"{b} {w}" for b, w in arg) + "\n"
            for b, w in arg:
                tr.restart(b, w)
        want.append(tr.expected())
        strides.append(want[-1][0])
    got = _states(driver, text, len(STARTS), len(cmds))
    for q, (g, w) in enumerate(zip(got, want)):
        assert g[2] == w[2], (q, g[2], w[2])
        assert g[0] == w[0] and g[1] == w[1], (q, g, w)
    assert all(ev == {"pop", "append"} for ev in tr.events), tr.events
    assert len(set(strides)) > 1 and min(strides[-4:]) < max(strides)  # the rows crossed stride changes, both ways


# ---- the C ABI -------------------------------------------------------------------------------------
def test_symbols_and_null_handles():
    import hsddp
    from hsddp._lib import DP, EXPORTS
    E = _codes()
    L = hsddp.lib()
    V = C.c_void_p
    hdr = open(os.path.join(ROOT, "include", "hsddp.h")).read()
    for name in ("hsddp_set_terrain", "hsddp_get_terrain"):
        assert name in EXPORTS and re.search(r"\b" + name + r"\(", hdr)
        assert list(getattr(L, name).argtypes) == [V, DP, DP]
    one = (C.c_double * 1)(0.5)
    assert L.hsddp_set_terrain(None, one, one) == E["HSDDP_ERR_ARG"]
    assert L.hsddp_set_terrain(None, None, None) == E["HSDDP_ERR_ARG"]
    assert L.hsddp_get_terrain(None, one, one) == E["HSDDP_ERR_ARG"]
    assert L.hsddp_last_error()


def test_facade_collects_per_phase_terrain():
    """tests/drivers/terrain_facade host: describe() with set_friction_coefficient / update_ground_height
    called per phase — collected as per-phase terrain; phases that agree stay cparams; two touchdown
    constraints of one phase with different ground, and a differing delta_min, are still refused."""
    r = subprocess.run(["make", "-C", DRIVERS, "-f", "terrain.mk", "terrain_facade"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(DRIVERS, "terrain_facade"), "host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "terrain_facade host ok" in r.stdout, r.stdout + r.stderr
