"""The host bookkeeping of hsddp_advance and hsddp_restart_elements (hkd-mpc_amd/csrc/hsddp_phases.cpp:
the walk over the reference table, the new contact and duration rows, the restart's batch decisions,
the slot maps and the sweep pairs) against the oracle's ProblemTracker, without a GPU:
tests/drivers/horizon_check is built from that one source and holds a small batch's host state, which
it steps and restarts as hsddp_horizon.cpp's entry points do, minus the device.

Every element is compared, after every command, with a tracker of its own: one constructed at the
element's last restart sample and updated since.  Everything is integer or float data movement, so
every comparison is exact."""
import copy
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import ref_oracle as R  # noqa: E402

DRIVERS = os.path.join(ROOT, "tests", "drivers")
GOLD = os.path.join(ROOT, "tests", "golden")
N_WIN = 62  # QuadReference::initialize: round(0.6 / 0.01) + 2 samples
KC, S_CAP = 60, 76  # plan_duration / dt_sim control slots; the handle's capacity Kc + HSDDP_MAX_PHASES


def _codes():
    hdr = open(os.path.join(ROOT, "include", "hsddp.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(HSDDP_(?:OK|ERR_[A-Z]+))\s*=?\s*(-?\d+)", hdr)}


_REFS = {}


def _ref(name):
    if name not in _REFS:
        _REFS[name] = R.load_quad_reference(os.path.join(GOLD, f"ref_{name}.csv"))
    return _REFS[name]


def _ints(word):
    return [int(v) for v in word.split(",")] if word else []


def _fields(line):
    words = line.split()
    out = {"_head": [w for w in words if "=" not in w], "f": []}
    for w in words:
        if "=" in w:
            k, v = w.split("=", 1)
            if k == "f":
                out["f"].append(_ints(v))
            else:
                out[k] = v
    return out


def _run(name, B, Bref, starts, commands, binary=None):
    """the driver (or another build of it, `binary`) over one gait file; returns the reply lines (the
    'ok start' line dropped)"""
    ref, dt = _ref(name)
    if binary is None:
        r = subprocess.run(["make", "-C", DRIVERS, "horizon_check"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        binary = os.path.join(DRIVERS, "horizon_check")
    text = f"{len(ref)} {float(dt)!r} {N_WIN} 0.6 0.01 0.01 {KC} {S_CAP}\n"
    text += "".join(" ".join(str(int(c)) for c in q["contact"]) + " " +
                    " ".join(repr(float(d)) for d in q["status_dur"]) + "\n" for q in ref)
    text += f"{B} {Bref}\n" + " ".join(str(s) for s in starts) + "\n" + "\n".join(commands) + "\n"
    r = subprocess.run([binary], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert lines[0] == "ok start", lines[0]
    return lines[1:]


class Replies:
    """the reply lines of a run, consumed command by command"""

    def __init__(self, lines, B):
        self.lines, self.B, self.at = lines, B, 0

    def reply(self):
        self.at += 1
        return self.lines[self.at - 1]

    def state(self):
        batch = _fields(self.reply())
        assert batch["_head"] == ["batch"]
        els = []
        for b in range(self.B):
            f = _fields(self.reply())
            assert f["_head"] == ["el", str(b)]
            els.append(f)
        return batch, els

    def done(self):
        return self.at == len(self.lines)


def _check_element(f, tk, stride_P, where):
    """one element's state line against its tracker"""
    hz = _ints(f["N"])
    P = len(hz)
    assert hz == tk.horizons, where
    assert _ints(f["ss"]) == tk.shooting, where
    assert _ints(f["reach"]) == tk.reach_end, where
    rows = np.array(_ints(f["rows"])).reshape(stride_P + 1, 4)
    assert np.array_equal(rows[:P + 1], tk.contact_rows()), where  # rows 0 .. P
    assert not rows[P + 1:].any(), where                           # the stride's padding
    dur = np.array([float(v) for v in f["dur"].split(",")]).reshape(stride_P, 4)
    assert np.array_equal(dur[:P], np.array(tk.durations)), where
    assert not dur[P:].any(), where
    assert int(f["ws"]) == tk.start, where
    assert float(np.float32(float(f["t"]))) == float(tk.t_cur), where
    # the references' slot samples of this layout (padding slots repeat the last one)
    slots = _ints(f["slots"])
    want = [R.sample_at(t, tk.dt, N_WIN - 1) for t in R.slot_times(hz, 0.01)]
    assert slots[:len(want)] == want and set(slots[len(want):]) <= {want[-1]}, where
    return tuple(hz)


def _key(f):
    return tuple(_ints(f["key"]))


def _pair_layouts_model(keys):
    """the pairing rule: elements of equal layout key, two per entry, the groups in key order"""
    groups = {}
    for b, k in enumerate(keys):
        groups.setdefault(k, []).append(b)
    pairs = []
    for k in sorted(groups):
        g = groups[k]
        for j in range(0, len(g), 2):
            pairs += [g[j], g[j + 1] if j + 1 < len(g) else -1]
    return pairs


def _patch_pairs_model(pairs, n_pairs, keys, listed):
    """the in-place rule: a listed element leaves its pair (its partner stays alone), the listed pair up among
    themselves by new key, taking emptied entries from the last emptied on, else a new entry; what
    stays empty is filled from the end, the highest first"""
    pr, n = list(pairs), n_pairs
    of = {e: q // 2 for q, e in enumerate(pr[:2 * n]) if e >= 0}
    freed = []
    for b in listed:
        q = of.pop(b)
        partner = pr[2 * q + 1] if pr[2 * q] == b else pr[2 * q]
        pr[2 * q:2 * q + 2] = [partner, -1]
        if partner < 0:
            freed.append(q)
    groups = {}
    for b in listed:
        groups.setdefault(keys[b], []).append(b)
    for k in sorted(groups):
        g = groups[k]
        for j in range(0, len(g), 2):
            if freed:
                q = freed.pop()
            else:
                q, n = n, n + 1
            pr += [-1] * (2 * q + 2 - len(pr))
            pr[2 * q:2 * q + 2] = [g[j], g[j + 1] if j + 1 < len(g) else -1]
    for q in sorted(freed, reverse=True):
        if q != n - 1:
            pr[2 * q:2 * q + 2] = pr[2 * n - 2:2 * n]
        n -= 1
    return pr[:2 * n], n


def _check_pairs(batch, els, where):
    """the sweep pairs of a per-element state: a partition of the elements into pairs of equal layout"""
    B = len(els)
    keys = [_key(f) for f in els]
    n_pairs = int(batch["n_pairs"])
    pair_of = _ints(batch["pair_of"])

    def valid(pairs, n):
        seen = []
        for q in range(n):
            a, b = pairs[2 * q], pairs[2 * q + 1]
            assert a >= 0, (where, "an empty entry below n_pairs")
            seen.append(a)
            if b >= 0:
                seen.append(b)
                assert keys[a] == keys[b], (where, "partners of different layout")
        assert sorted(seen) == list(range(B)), (where, "not every element in exactly one pair")

    pairs = _ints(batch["pairs"])
    valid(pairs, n_pairs)
    for q in range(n_pairs):
        for e in pairs[2 * q:2 * q + 2]:
            assert e < 0 or pair_of[e] == q, where
    fresh = _ints(batch["fresh"])  # pair_layouts of the same layouts
    valid(fresh, len(fresh) // 2)
    assert len(fresh) // 2 <= n_pairs, where
    assert fresh == _pair_layouts_model(keys), where  # and in the rule's order
    return {"pairs": pairs, "n": n_pairs, "keys": keys}


def _check_patch(before, after, touched, listed, where):
    """patch_pairs: only the entries it reports differ from before, and they are what the rule gives"""
    touched = set(touched)
    assert touched, where
    for q in range(max(len(before["pairs"]), len(after["pairs"])) // 2):
        if q not in touched:
            assert before["pairs"][2 * q:2 * q + 2] == after["pairs"][2 * q:2 * q + 2], (where, q)
    want, n = _patch_pairs_model(before["pairs"], before["n"], after["keys"], listed)
    assert (after["pairs"][:2 * n], after["n"]) == (want, n), where


ADVANCE_CASES = [("trot", 0, 36, 1, 6), ("flytrot", 6, 8, 2, 2), ("flytrot", 3, 12, 3, 2), ("trot", 7, 36, 1, 4),
                 ("trot", 19, 24, 2, 4)]


@pytest.mark.parametrize("name,start,steps,n,flag_sum", ADVANCE_CASES)
def test_advance_matches_the_tracker(name, start, steps, n, flag_sum):
    """`steps` simulation steps in ticks of n"""
    ref, dt = _ref(name)
    ticks = steps // n
    rp = Replies(_run(name, 1, 1, [start], ["state"] + [f"advance {n}", "state"] * ticks), 1)
    tk = R.ProblemTracker(ref, start, dt)
    _, els = rp.state()
    _check_element(els[0], tk, len(tk.horizons), "start")
    total, reach_last, most_phases, most_td = 0, 0, 0, 0
    for tick in range(ticks):
        flags = tk.update(n)
        f = _fields(rp.reply())
        assert f["_head"] == ["ok"] and f["maps"] == "1" and f["agree"] == "1", (tick, f)
        assert f["f"] == [flags] and _ints(f["or"]) == flags, tick
        batch, els = rp.state()
        assert batch["elem"] == "0" and int(batch["P"]) == len(tk.horizons)
        _check_element(els[0], tk, len(tk.horizons), tick)
        total += sum(flags)
        reach_last += tk.reach_end[-1]
        most_phases = max(most_phases, len(tk.horizons))
        most_td = max(most_td, max(len(t) for t in tk.td))
    assert rp.done()
    assert total == flag_sum and total >= 2
    if name == "trot" and start in (0, 7):  # ticks whose last phase has reached its end: row P from plan + dt_mpc
        assert reach_last == {0: 3, 7: 2}[start]
    if name == "trot" and start == 0:
        assert most_phases == 7 and most_td == 2


def test_shared_layout_batch_follows_element_zero():
    """B = 3 on one reference window with identical contact rows: element 0's bookkeeping, one slot map"""
    ref, dt = _ref("trot")
    rp = Replies(_run("trot", 3, 1, [0, 0, 0], ["advance 1", "state"] * 36), 3)
    tk = R.ProblemTracker(ref, 0, dt)
    for tick in range(36):
        flags = tk.update(1)
        f = _fields(rp.reply())
        assert f["maps"] == "1" and f["agree"] == "1" and f["f"] == [flags] * 3, tick
        batch, els = rp.state()
        assert batch["elem"] == "0" and batch["maps"] == "1"
        for b in range(3):
            _check_element(els[b], tk, len(tk.horizons), (tick, b))


def test_diverging_elements_keep_their_own_layouts():
    ref, dt = _ref("trot")
    starts = (0, 7)
    rp = Replies(_run("trot", 2, 2, starts, ["state"] + ["advance 1", "state"] * 30), 2)
    tks = [R.ProblemTracker(ref, s, dt) for s in starts]
    batch, els = rp.state()
    assert batch["elem"] == "1"
    for tick in range(30):
        flags = [tk.update(1) for tk in tks]
        f = _fields(rp.reply())
        assert f["_head"] == ["ok"] and f["maps"] == "2" and f["agree"] == "0", tick
        assert f["f"] == flags and _ints(f["or"]) == [flags[0][0] | flags[1][0]], tick
        batch, els = rp.state()
        P, S = int(batch["P"]), int(batch["S"])
        assert batch["elem"] == "1" and batch["maps"] == "2"
        assert P == max(len(tk.horizons) for tk in tks)
        assert S == max(sum(h + 1 for h in tk.horizons) for tk in tks) and S <= 67 <= S_CAP
        lays = [_check_element(els[b], tks[b], P, (tick, b)) for b in range(2)]
        assert lays[0] != lays[1]
        _check_pairs(batch, els, tick)
        assert int(batch["n_pairs"]) == 2


def test_disagreement_under_shared_references_is_refused():
    """B = 2 on one window; the contact row of element 1's last phase altered before a tick without a
    contact change, so element 1 sees one where element 0 sees none"""
    ref, dt = _ref("trot")
    tk, k = R.ProblemTracker(ref, 0, dt), 0
    while copy.deepcopy(tk).update(1) != [0]:  # the first tick at which element 0 sees no contact change
        tk.update(1)
        k += 1
    P = len(tk.horizons)
    last = tk.contact_rows()[P - 1]
    cmds = [f"advance {k}", "state", f"alter 1 {P - 1} 0 {1 - int(last[0])}", "state", "advance 1", "state"]
    lines = _run("trot", 2, 1, [0, 0], cmds)
    assert lines[0].startswith("ok maps=1 agree=1") and lines[4] == "ok alter"
    words = lines[8].split(None, 2)
    assert words[:2] == ["refused", str(_codes()["HSDDP_ERR_UNSUPPORTED"])], lines[8]
    assert "elements disagree" in words[2] and "ref_per_element = 1" in words[2]
    assert lines[1:4] != lines[5:8] and lines[9:12] == lines[5:8]  # altered, then unchanged by the refusal


def test_table_end():
    """one step at a time: accepted through tick 129, refused when the window start reaches the table's length"""
    ref, dt = _ref("trot")
    assert len(ref) == 130
    rp = Replies(_run("trot", 1, 1, [0], ["advance 1", "state"] * 131), 1)
    tk = R.ProblemTracker(ref, 0, dt)
    for tick in range(1, 130):
        flags = tk.update(1)
        f = _fields(rp.reply())
        assert f["_head"] == ["ok"] and f["f"] == [flags], tick
        batch, els = rp.state()
        _check_element(els[0], tk, int(batch["P"]), tick)
    assert tk.start == 129
    before = rp.lines[rp.at - 2:rp.at]
    tk.start += 1  # tick 130: QuadReference::step would move the window start to 130 = the table length
    assert tk.start == len(ref)
    words = rp.reply().split(None, 2)
    assert words[:2] == ["refused", str(_codes()["HSDDP_ERR_ARG"])] and "ran past the table" in words[2]
    assert rp.lines[rp.at:rp.at + 2] == before  # the state unchanged


def _restart_sequence():
    """B = 3 on per-element references: 20 ticks, element 1 restarted at sample 20, 5 ticks, elements 0
    and 2 at samples 33 and 40, 10 ticks, then all three at sample 40 (one layout, one clock, and other strides)"""
    cmds = ["state"] + ["advance 1", "state"] * 20 + ["restart 1 1 20", "state"] + ["advance 1", "state"] * 5
    cmds += ["restart 2 0 33 2 40", "state"] + ["advance 1", "state"] * 10 + ["restart 3 0 40 1 40 2 40", "state"]
    cmds += ["advance 1", "state"] * 3
    return cmds


def _walk_restart_sequence(lines):
    ref, dt = _ref("trot")
    rp = Replies(lines, 3)
    tks = [R.ProblemTracker(ref, 0, dt) for _ in range(3)]
    seen = {"restarts": [], "layouts": set()}
    pairs_before = None

    def check_state(where):
        nonlocal pairs_before
        batch, els = rp.state()
        P = int(batch["P"])
        for b in range(3):
            seen["layouts"].add(_check_element(els[b], tks[b], P, (where, b)))
        lays = {tuple(tk.horizons) for tk in tks}
        if batch["elem"] == "1":
            # the strides are the maxima over the elements' tracker layouts
            assert P == max(len(tk.horizons) for tk in tks), where
            assert int(batch["S"]) == max(sum(h + 1 for h in tk.horizons) for tk in tks), where
            pairs_before = _check_pairs(batch, els, where)
        else:
            assert len(lays) == 1 and P == len(tks[0].horizons), where
            assert len({els[b]["t"] for b in range(3)}) == 1, where  # the shared clock
            pairs_before = None
        return batch

    def ticks(k, where):
        for tick in range(k):
            flags = [tk.update(1) for tk in tks]
            f = _fields(rp.reply())
            assert f["_head"] == ["ok"] and f["f"] == flags, (where, tick)
            check_state((where, tick))

    def restart(listed, where):
        before = pairs_before
        for b, s in listed:
            tks[b] = R.ProblemTracker(ref, s, dt)
        f = _fields(rp.reply())
        assert f["_head"] == ["ok"], (where, f)
        P, S = int(f["P"]), int(f["S"])
        assert (P, S) == (int(f["strideP"]), int(f["strideS"])), where  # the plan's strides are the state's
        # the device rows of the listed elements: contact rows, window starts, slot maps
        rows = np.array(_ints(f["rows"])).reshape(len(listed), P + 1, 4)
        idx, map_id = np.array(_ints(f["idx"])).reshape(-1, S), _ints(f["map_id"])
        assert _ints(f["start"]) == [s for _, s in listed], where
        for m, (b, s) in enumerate(listed):
            hz = tks[b].horizons
            assert np.array_equal(rows[m, :len(hz) + 1], tks[b].contact_rows()) and not rows[m, len(hz) + 1:].any(), where
            want = [R.sample_at(t, tks[b].dt, N_WIN - 1) for t in R.slot_times(hz, 0.01)]
            assert list(idx[map_id[m], :len(want)]) == want, where
        assert len(idx) == len({tuple(tks[b].horizons) for b, _ in listed}), where
        check_state(where)
        kind = "one" if f["one"] == "1" else "in_place" if f["in_place"] == "1" else "restride" if f["restride"] == "1" else "relayout"
        if kind == "in_place":
            _check_patch(before, pairs_before, _ints(f["touched"]), [b for b, _ in listed], where)
        seen["restarts"].append((kind, f["restride"] == "1"))

    check_state("start")
    ticks(20, "a")
    restart([(1, 20)], "restart 1")
    ticks(5, "b")
    restart([(0, 33), (2, 40)], "restart 0, 2")
    ticks(10, "c")
    restart([(0, 40), (1, 40), (2, 40)], "restart all")
    ticks(3, "d")
    assert rp.done()
    return seen


def test_restarts_and_per_element_clocks():
    seen = _walk_restart_sequence(_run("trot", 3, 3, [0, 0, 0], _restart_sequence()))
    # a shared-layout batch whose element 1 takes another layout of the same strides: every element's
    # layout is installed; per-element layouts whose strides stand: in place; all three onto one
    # layout of fewer phases: the shared layout and clock again, at new strides
    assert seen["restarts"] == [("relayout", False), ("in_place", False), ("one", True)]
    assert len(seen["layouts"]) >= 8


def test_in_place_and_restriding_restarts():
    """B = 4 with per-element layouts from the start: restarts that keep the strides are in place and patch
    the sweep pairs; one that brings a layout of more phases raises the strides, and the restart of
    the element that alone holds them lowers them again"""
    ref, dt = _ref("trot")
    starts = [0, 0, 1, 1]
    tks = [R.ProblemTracker(ref, s, dt) for s in starts]
    P0 = max(len(tk.horizons) for tk in tks)
    # restart samples of test_restart_host.py's list, by the phases of a new problem there
    by_P = {s: len(R.ProblemTracker(ref, s, dt).horizons) for s in (0, 1, 7, 19, 20, 21, 33, 40, 57)}
    more = [s for s, P in by_P.items() if P > P0]
    same = [s for s, P in by_P.items() if P == P0 and s not in (0, 1)]
    assert more and len(same) >= 3
    calls = [([(1, same[0])], "in_place"), ([(0, same[1]), (3, same[1])], "in_place"), ([(2, more[0])], "restride"),
             ([(2, same[2])], "restride")]
    cmds = ["state"]
    for listed, _ in calls:
        cmds += [f"restart {len(listed)} " + " ".join(f"{b} {s}" for b, s in listed), "state"]
    cmds += ["advance 1", "state"]
    rp = Replies(_run("trot", 4, 4, starts, cmds), 4)

    def check(where):
        batch, els = rp.state()
        assert batch["elem"] == "1"
        P = int(batch["P"])
        assert P == max(len(tk.horizons) for tk in tks) and int(batch["S"]) == max(sum(h + 1 for h in tk.horizons) for tk in tks)
        for b in range(4):
            _check_element(els[b], tks[b], P, (where, b))
        return batch, _check_pairs(batch, els, where)

    _, before = check("start")
    strides = []
    for listed, kind in calls:
        for b, s in listed:
            tks[b] = R.ProblemTracker(ref, s, dt)
        f = _fields(rp.reply())
        assert f["_head"] == ["ok"] and f["one"] == "0", f
        assert (f["in_place"], f["restride"]) == (("1", "0") if kind == "in_place" else ("0", "1")), (listed, f)
        batch, after = check(listed)
        if kind == "in_place":
            _check_patch(before, after, _ints(f["touched"]), [b for b, _ in listed], listed)
        before = after
        strides.append(int(batch["P"]))
    assert strides == [P0, P0, P0 + 1, P0]
    flags = [tk.update(1) for tk in tks]
    assert _fields(rp.reply())["f"] == flags
    check("tick")
    assert rp.done()
