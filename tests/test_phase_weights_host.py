"""The host side of the per-phase weights (hsddp_set_phase_weights) without a GPU: the override flags
and rows' moves through hsddp_advance and hsddp_restart_elements on the reference's trot file
(walk_advance, plan_restart_batch) against oracle/ref_oracle.py's ProblemTracker with the overrides
riding on its phases, and through caller-flagged shifts and arriving elements (plan_shift,
plan_import_batch) against a restatement of HKDProblem::update's bookkeeping driven by the same flags
(hkd-mpc_amd/csrc/hsddp_phases.cpp: shift_phase_weights, put_phase_weight_rows, export_element;
tests/drivers/phase_weights_check is built from that one source, and a second time with the address
and undefined-behaviour sanitizers); the two symbols' prototypes and NULL refusals; the element
record's version and header."""
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
sys.path.insert(0, os.path.join(ROOT, "oracle"))
KC, S_CAP = 20, 36
NW = 46


# ---- the restatement ------------------------------------------------------------------------------
def _row(base):
    """(first, last) field of the row whose field j is base + (j + 1) / 64"""
    return [base + 1 / 64.0, base + NW / 64.0]


NONE = (0, [0.0, 0.0])


def start_rows(b, n):
    """robot b's overrides as the driver makes them: on the phases with (b + i) % 3 != 0"""
    return [(1, _row(100 * b + i)) if (b + i) % 3 else NONE for i in range(n)]


def robot(b, N, reach=None):
    N = list(N)
    return dict(N=N, reach=list(reach) if reach else [0] * len(N), rows=start_rows(b, len(N)))


def arriving(tag, N, reach=None):
    N = list(N)
    rows = [(1, _row(5000 + 100 * tag + i)) if tag >= 0 and i % 2 == 0 else NONE for i in range(len(N))]
    return dict(N=N, reach=list(reach) if reach else [0] * len(N), rows=rows, tag=tag)


def move(rows, phase_src):
    """one robot's overrides after a shift: an old phase keeps its own, a phase the shift started has none"""
    return [rows[src] if src >= 0 else NONE for src in phase_src]


def step(e, change):
    """one step of HKDProblem::update's bookkeeping (HKDProblem.cpp:117-222; PhaseStepper) with the
    overrides riding on the phases"""
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
    e["rows"] = move(e["rows"], src)


def flat(rows_per_robot):
    P = max(len(r) for r in rows_per_robot)
    pad = [list(r) + [NONE] * (P - len(r)) for r in rows_per_robot]
    return P, [[f for f, _ in r] for r in pad], [sum((v for _, v in r), []) for r in pad]


# ---- the driver ------------------------------------------------------------------------------------
def _line(e):
    return f"{len(e['N'])} {' '.join(map(str, e['N']))} {' '.join(map(str, e['reach']))}"


@pytest.fixture(scope="module", params=["phase_weights_check", "phase_weights_check_san"])
def driver(request):
    """the driver, and its build with -fsanitize=address,undefined (a stand-alone program: any report ends
    it with a non-zero status)"""
    r = subprocess.run(["make", "-C", DRIVERS, "-f", "phase_weights.mk", request.param], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return os.path.join(DRIVERS, request.param)


def _states(driver, text, B, n_commands):
    r = subprocess.run([driver], input=text, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-2000:]
    states, lines = [], r.stdout.splitlines()
    assert not any(l.startswith(("refused", "export mismatch")) or "torn" in l for l in lines), lines
    for q, l in enumerate(lines):
        if l.startswith("state"):
            P = int(re.search(r"P=(\d+)", l).group(1))
            els = [dict(w.split("=", 1) for w in m.split()[2:]) for m in lines[q + 1:q + 1 + B]]
            states.append((P, [[int(v) for v in e["set"].split(",")] for e in els],
                           [[float(v) for v in e["rows"].split(",")] for e in els],
                           [[int(v) for v in e["N"].split(",")] for e in els]))
    assert len(states) == 1 + n_commands
    return states


def check(driver, batch, elem, commands):
    text = f"rows {KC} {S_CAP} {len(batch)} {int(elem)}\n" + "".join(_line(e) + "\n" for e in batch)
    for kind, arg in commands:
        if kind == "shift":
            text += f"shift {len(arg[0])}\n" + "".join(" ".join(map(str, f)) + "\n" for f in arg)
        else:
            text += f"take {len(arg)}\n" + "".join(f"{d} {e['tag']} {_line(e)}\n" for d, e in arg)
    states = _states(driver, text, len(batch), len(commands))
    assert states[0][:3] == flat([e["rows"] for e in batch])
    for (kind, arg), got in zip(commands, states[1:]):
        if kind == "shift":
            for e, flags in zip(batch, arg):
                for f in flags:
                    step(e, f)
        else:
            for d, e in arg:
                batch[d] = dict(N=list(e["N"]), reach=list(e["reach"]), rows=list(e["rows"]))
        assert got[3] == [e["N"] for e in batch]
        assert got[:3] == flat([e["rows"] for e in batch]), (kind, got)
    return batch


def test_overrides_ride_the_phases_through_shifts(driver):
    """Four robots of one 4 x 5 layout crossing phase boundaries at different steps: the override of a
    removed first phase is dropped, an appended phase has none, the others keep theirs; twelve steps,
    so every robot has dropped two first phases and appended last ones."""
    batch = [robot(b, [5, 5, 5, 5]) for b in range(4)]
    flags = [[[1, 0, 1, 0], [0, 0, 0, 0], [0, 1, 0, 1], [1, 1, 0, 0]],
             [[0, 0, 0, 0], [1, 0, 0, 1], [0, 0, 0, 0], [0, 0, 1, 0]],
             [[0, 1, 0, 0], [0, 0, 1, 0], [1, 0, 0, 0], [0, 1, 0, 0]]]
    after = check(driver, batch, False, [("shift", f) for f in flags])
    for b, e in enumerate(after):
        first = start_rows(b, 4)
        assert e["rows"][:2] == first[2:], (b, e)
        assert all(r == NONE for r in e["rows"][2:]) and len(e["rows"]) > 2, (b, e)


def test_one_flag_set_for_the_batch_keeps_the_shared_layout(driver):
    batch = [robot(b, [2, 8, 10]) for b in range(3)]
    after = check(driver, batch, False, [("shift", [[0, 1, 1, 0, 0]] * 3), ("shift", [[0, 0, 0, 1, 1]] * 3)])
    assert all(e["N"] == after[0]["N"] for e in after)


def test_arriving_elements(driver):
    """A per-element batch: an element arrives with its overrides in place; two arrive without any;
    one arrives with more phases than the stride (every robot's flags and rows move to the new
    stride), then the stride shrinks again when it is replaced — and the shifts after that carry all
    of it on.  The record an arrived element would leave with carries what it came with."""
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
PLAN, N_WIN, KC_T, S_CAP_T = 0.4, 42, 40, 56  # a 0.4 s plan: round(0.4 / 0.01) + 2 samples, Kc = 40
STARTS = [0, 4, 9, 15, 20]  # within 16 ticks every robot drops a first phase and appends a last one


class Tracked:
    """oracle/ref_oracle.py's ProblemTracker per robot with the overrides riding on its phases: a
    popped first phase drops its own, an appended phase has none, a restart leaves none"""

    def __init__(self):
        import ref_oracle as R
        self.R = R
        self.ref, self.dt = R.load_quad_reference(os.path.join(ROOT, "tests", "golden", "ref_trot.csv"))
        self.tk = [R.ProblemTracker(self.ref, w, self.dt, plan_duration=PLAN) for w in STARTS]
        self.rows = [start_rows(b, len(t.horizons)) for b, t in enumerate(self.tk)]
        self.events = [set() for _ in STARTS]

    def advance(self, n):
        for b, t in enumerate(self.tk):
            for _ in range(n):
                n0, pop = len(t.horizons), t.horizons[0] <= 1
                t.step()
                app = len(t.horizons) - (n0 - pop)
                self.rows[b] = move(self.rows[b], list(range(int(pop), n0)) + [-1] * app)
                self.events[b] |= ({"pop"} if pop else set()) | ({"append"} if app else set())

    def restart(self, b, start):
        self.tk[b] = self.R.ProblemTracker(self.ref, start, self.dt, plan_duration=PLAN)
        self.rows[b] = [NONE for _ in self.tk[b].horizons]

    def expected(self):
        return flat(self.rows) + ([list(t.horizons) for t in self.tk],)


def test_overrides_ride_the_phases_through_advances_and_restarts(driver):
    """walk_advance's plan and plan_restart_batch on five robots whose windows start at different
    samples of the trot file: after every hsddp_advance (one step, and three at once) and every
    restart — of one robot in place, and of the robots that hold the batch's largest phase count, so
    that every robot's rows move to a smaller stride — flags and rows equal the ProblemTracker
    restatement's, and so do the layouts."""
    tr = Tracked()
    text = f"table {len(tr.ref)} {float(tr.dt)!r} {N_WIN} {PLAN!r} 0.01 0.01 {KC_T} {S_CAP_T}\n"
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
            if arg == "widest":
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
        assert g[3] == w[3], (q, g[3], w[3])
        assert g[:3] == w[:3], (q, g, w)
    assert all(ev == {"pop", "append"} for ev in tr.events), tr.events
    assert len(set(strides)) > 1 and min(strides[-4:]) < max(strides)  # the rows crossed stride changes, both ways


# ---- the C ABI -------------------------------------------------------------------------------------
def _codes():
    hdr = open(os.path.join(ROOT, "include", "hsddp.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(HSDDP_(?:OK|ERR_[A-Z]+))\s*=\s*(-?\d+)", hdr)}


def test_symbols_and_null_handles():
    import hsddp
    from hsddp._lib import EXPORTS
    E = _codes()
    L = hsddp.lib()
    V = C.c_void_p
    hdr = open(os.path.join(ROOT, "include", "hsddp.h")).read()
    for name, n in (("hsddp_set_phase_weights", 3), ("hsddp_get_phase_weights", 3)):
        assert name in EXPORTS and re.search(r"\b" + name + r"\(", hdr)
        assert list(getattr(L, name).argtypes) == [V] * n
    w = (hsddp.Weights * 4)()
    flags = (C.c_int * 4)()
    assert L.hsddp_set_phase_weights(None, C.addressof(w), None) == E["HSDDP_ERR_ARG"]
    assert L.hsddp_set_phase_weights(None, None, None) == E["HSDDP_ERR_ARG"]
    assert L.hsddp_get_phase_weights(None, C.addressof(w), C.addressof(flags)) == E["HSDDP_ERR_ARG"]
    assert L.hsddp_last_error()
    assert hasattr(hsddp.Solver, "set_phase_weights") and hasattr(hsddp.Solver, "phase_weights")


def test_record_version_and_override_block(tmp_path):
    """The element record carries the overrides in a block of whole lines between the header and the
    payload (PhaseOverrides: flags [16] and rows [16][46]): version word "HEL4"; the header is the size
    it was and every payload piece shifts by exactly the block."""
    import shutil
    src = open(os.path.join(ROOT, "hkd-mpc_amd", "csrc", "hsddp_elements.h")).read()
    m = re.search(r"RECORD_VERSION\s*=\s*(0x[0-9a-fA-F]+)", src)
    assert m and int(m.group(1), 16) == int.from_bytes(b"HEL4", "big")
    prog = tmp_path / "block.cpp"
    prog.write_text('#include <cstdio>\n#include "hsddp_elements.h"\nint main(){\n'
                    'const hsddp::RecordLayout a = hsddp::record_layout(40, 56, 0), b = hsddp::record_layout(40, 56, 0, true);\n'
                    'std::printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(hsddp::PhaseOverrides), hsddp::PW_BLOCK, a.pw, b.pw, '
                    'a.K, b.K, a.hist, b.hist, b.bytes - a.bytes);\nreturn 0;}\n')
    exe = tmp_path / "block"
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    r = subprocess.run([hipcc, "-x", "hip", "--offload-arch=gfx950", "-std=c++17", "-I", os.path.join(ROOT, "hkd-mpc_amd", "csrc"),
                        "-I", os.path.join(ROOT, "include"), str(prog), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    size, block, pa, pb, ka, kb, ha, hb, grow = (int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert size == 4 + 16 * 4 + 4 + 16 * NW * 8 and block == (size + 127) // 128 * 128
    assert pa == 0 and pb == ka and pb % 128 == 0
    assert kb - ka == block and hb - ha == block and grow == block


def test_facade_collects_per_phase_rows():
    """tests/drivers/phase_weights_facade host: describe() derives one weight row per phase — the hkd::
    terms' own weights, and the reference classes' diagonals by the quotient rule per phase, masked
    fields from the handle-wide derivation; the phases that differ from the handle's set are the
    overrides, phases that agree give none; qJ weight on a stance leg is still refused."""
    r = subprocess.run(["make", "-C", DRIVERS, "-f", "phase_weights.mk", "phase_weights_facade"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(DRIVERS, "phase_weights_facade"), "host"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "phase_weights_facade host ok" in r.stdout, r.stdout + r.stderr
