"""The host side of hsddp_copy_elements / hsddp_export_elements / hsddp_import_elements without a
GPU: plan_import_batch's decisions (hkd-mpc_amd/csrc/hsddp_phases.cpp; tests/drivers/elements_check
is built from that one source) against a short restatement, the four symbols' prototypes and NULL
refusals, and traffic.py's bytes per moved element against the buffer table of DESIGN.md §2."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "tests", "drivers")
sys.path.insert(0, os.path.join(ROOT, "hkd-mpc_amd"))
KC, S_CAP = 20, 36


def _codes():
    hdr = open(os.path.join(ROOT, "include", "hsddp.h")).read()
    return {k: int(v) for k, v in re.findall(r"\b(HSDDP_(?:OK|ERR_[A-Z]+))\s*=\s*(-?\d+)", hdr)}


# ---- the restatement -----------------------------------------------------------------------------------
def el(N, reach=None, clock=0.0, tag=0, ss=None):
    """one element: horizons, reach flags, clock, the tag its rows are made from"""
    N = list(N)
    return dict(N=N, ss=list(ss) if ss else [n + 1 for n in N], reach=list(reach) if reach else [0] * len(N),
                clock=clock, tag=tag, ws=100 + tag)


def _S(e):
    return sum(n + 1 for n in e["N"])


def _lay(e):
    return (e["N"], e["ss"])


def _key(e):
    return tuple(e["N"]) + (-1,) + tuple(e["ss"])


def _rows(e, P):
    c = [[(e["tag"] + i + l) & 1 for l in range(4)] if i <= len(e["N"]) else [0] * 4 for i in range(P + 1)]
    d = [[e["tag"] + i / 4.0 + l / 64.0 for l in range(4)] if i < len(e["N"]) else [0.0] * 4 for i in range(P)]
    return sum(c, []), sum(d, [])


def _fresh_pairs(els, which=None):
    which = list(range(len(els))) if which is None else which
    groups = {}
    for b in which:
        groups.setdefault(_key(els[b]), []).append(b)
    out = []
    for k in sorted(groups):
        g = groups[k]
        out += [[g[j], g[j + 1] if j + 1 < len(g) else -1] for j in range(0, len(g), 2)]
    return out


def _patch_pairs(pairs, els_after, moved):
    """patch_pairs: a listed element leaves its pair, the listed pair up among themselves by new
    layout (emptied entries reused from the last one emptied), other emptied entries are filled
    from the end"""
    pairs = [list(p) for p in pairs]
    of = {b: q for q, p in enumerate(pairs) for b in p if b >= 0}
    freed = []
    for b in moved:
        q = of[b]
        partner = pairs[q][1] if pairs[q][0] == b else pairs[q][0]
        pairs[q] = [partner, -1]
        if partner < 0:
            freed.append(q)
    for g in _fresh_pairs(els_after, moved):
        if freed:
            pairs[freed.pop()] = g
        else:
            pairs.append(g)
    for q in sorted(freed, reverse=True):
        last = len(pairs) - 1
        if q != last:
            pairs[q] = pairs[last]
        pairs.pop()
    return pairs


def model(batch, elem, shared_clock, t_cur, moves):
    """what move_elements' host side must leave: (decisions, batch state)"""
    B = len(batch)
    dsts = [d for d, _ in moves]
    P0, S0 = max(len(e["N"]) for e in batch), max(_S(e) for e in batch)
    after = [dict(e, clock=t_cur if shared_clock else e["clock"]) for e in batch]
    for d, e in moves:
        after[d] = dict(e)
    Pn, Sn = max(len(e["N"]) for e in after), max(_S(e) for e in after)
    every = len(moves) == B
    first = moves[0][1]
    agree = all(_lay(e) == _lay(first) and e["reach"] == first["reach"] for _, e in moves)
    one = agree and (every or (not elem and _lay(first) == _lay(batch[0]) and first["reach"] == batch[0]["reach"]))
    restride = (Pn, Sn) != (P0, S0)
    in_place = bool(elem) and not restride and not every
    clocks = [e["clock"] for _, e in moves]
    same = all(c == clocks[0] for c in clocks)
    keeps = same if every else (shared_clock and same and clocks[0] == t_cur)
    dec = dict(one=int(one), in_place=int(in_place), restride=int(restride), all=int(every), P=Pn, S=Sn)
    if one:
        pairs = []
    elif in_place:
        pairs = _patch_pairs(_fresh_pairs(batch), after, dsts)
    else:
        pairs = _fresh_pairs(after)
    return dec, dict(elem=int(not one), pairs=pairs, shared_clock=int(keeps), t_cur=clocks[0] if every and same else t_cur,
                     els=after, P=Pn)


# ---- the driver ----------------------------------------------------------------------------------------
def _line(e):
    return " ".join(str(v) for v in [len(e["N"])] + e["N"] + e["ss"] + e["reach"])


def _run(batch, elem, shared_clock, t_cur, moves, s_cap=S_CAP):
    r = subprocess.run(["make", "-C", DRIVERS, "-f", "elements.mk", "elements_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    text = f"{KC} {s_cap} {len(batch)} {int(elem)} {int(shared_clock)} {t_cur!r}\n"
    text += "".join(f"{_line(e)} {e['clock']!r} {e['tag']}\n" for e in batch)
    text += f"{len(moves)}\n" + "".join(f"{d} {_line(e)} {e['clock']!r} {e['ws']} {e['tag']}\n" for d, e in moves)
    r = subprocess.run([os.path.join(DRIVERS, "elements_check")], input=text, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return r.stdout.splitlines()


def _fields(line):
    return dict(w.split("=", 1) for w in line.split() if "=" in w)


def _ints(word):
    return [int(v) for v in word.split(",")] if word else []


def _check(batch, elem, shared_clock, t_cur, moves):
    lines = _run(batch, elem, shared_clock, t_cur, moves)
    assert lines[0].startswith("ok "), lines[0]
    dec, want = model(batch, elem, shared_clock, t_cur, moves)
    got = _fields(lines[0])
    assert {k: int(got[k]) for k in dec} == dec
    assert int(got["strideP"]) == dec["P"] and int(got["strideS"]) == dec["S"]
    b = _fields(lines[1])
    assert int(b["elem"]) == want["elem"]
    assert int(b["shared_clock"]) == want["shared_clock"]
    if want["shared_clock"]:
        assert float(b["t_cur"]) == want["t_cur"]
    pairs = _ints(b["pairs"])
    assert [pairs[2 * q:2 * q + 2] for q in range(int(b["n_pairs"]))] == want["pairs"]
    if want["elem"]:
        of = _ints(b["pair_of"])
        for q, p in enumerate(want["pairs"]):
            for e in p:
                assert e < 0 or of[e] == q
    P = want["P"]
    for i, e in enumerate(want["els"]):
        f = _fields(lines[2 + i])
        assert _ints(f["N"]) == e["N"] and _ints(f["ss"]) == e["ss"] and _ints(f["reach"]) == e["reach"], i
        rows, dur = _rows(e, P)
        assert _ints(f["rows"]) == rows, i
        assert [float(v) for v in f["dur"].split(",")] == dur, i
        assert int(f["ws"]) == e["ws"], i
        assert float(f["t"]) == (want["t_cur"] if want["shared_clock"] else e["clock"]), i
    return dec


A2, B2, C2 = [8, 12], [5, 15], [16, 4]
A3, B3 = [5, 10, 5], [3, 15, 2]


def test_in_place_on_a_per_element_batch():
    batch = [el(A2, tag=0), el(A3, tag=1), el(A3, [0, 1, 0], tag=2), el(A2, tag=3), el(B2, tag=4)]
    moves = [(0, el(B2, clock=0.03125, tag=7)), (3, el(C2, [0, 1], clock=0.03125, tag=8))]
    dec = _check(batch, True, True, 0.015625, moves)  # clocks differ from the batch's: per-element clocks
    assert dec == dict(one=0, in_place=1, restride=0, all=0, P=3, S=23)
    moves = [(0, el(A2, clock=0.015625, tag=7))]         # the batch's clock: it stays shared
    assert _check(batch, True, True, 0.015625, moves)["in_place"] == 1
    _check(batch, True, False, 0.0, [(4, el(A3, clock=0.5, tag=9)), (1, el(A3, clock=0.25, tag=5))])


def test_restride_up_and_down():
    batch = [el(A2, tag=0), el(B2, tag=1), el(C2, tag=2), el(A2, tag=3)]
    dec = _check(batch, True, True, 0.015625, [(2, el(B3, [0, 1, 0], clock=0.03125, tag=6))])
    assert dec["restride"] == 1 and (dec["P"], dec["S"]) == (3, 23)
    batch = [el(A2, tag=0), el(A3, [0, 0, 1], tag=1), el(C2, tag=2), el(A2, tag=3)]  # the largest-P element leaves
    dec = _check(batch, True, False, 0.0, [(1, el(B2, clock=0.03125, tag=6))])
    assert dec["restride"] == 1 and (dec["P"], dec["S"]) == (2, 22)
    # ... and stays when another element holds the stride too
    batch = [el(A3, tag=0), el(A3, [0, 0, 1], tag=1), el(C2, tag=2)]
    assert _check(batch, True, False, 0.0, [(1, el(B2, clock=0.03125, tag=6))])["in_place"] == 1


def test_shared_layout_leaves_and_returns():
    batch = [el(A2, [0, 1], tag=b) for b in range(4)]
    dec = _check(batch, False, True, 0.015625, [(2, el(B2, clock=0.015625, tag=9))])  # another layout: per element
    assert dec == dict(one=0, in_place=0, restride=0, all=0, P=2, S=22)
    dec = _check(batch, False, True, 0.015625, [(2, el(A2, [0, 1], clock=0.015625, tag=9))])  # the shared layout and flags
    assert dec["one"] == 1
    dec = _check(batch, False, True, 0.015625, [(2, el(A2, [0, 0], clock=0.015625, tag=9))])  # ... other flags
    assert dec["one"] == 0
    # every slot of a per-element batch replaced by one layout: shared again, on the arrivals' clock
    batch = [el(A2, tag=0), el(A3, tag=1), el(B2, tag=2)]
    moves = [(b, el(C2, [0, 1], clock=0.0625, tag=5 + b)) for b in (2, 0, 1)]
    dec = _check(batch, True, True, 0.015625, moves)
    assert dec["one"] == 1 and dec["all"] == 1 and dec["restride"] == 1
    moves = [(b, el(C2, [0, 1], clock=0.0625 + b, tag=5 + b)) for b in (2, 0, 1)]  # ... on clocks of their own
    _check(batch, True, True, 0.015625, moves)


def test_refusals():
    E = _codes()
    batch = [el(A2, tag=0), el(A3, tag=1), el(B2, tag=2)]
    for moves in ([(3, el(A2))], [(-1, el(A2))], [(1, el(A2)), (1, el(B2))], [(0, el([8, 13]))]):
        lines = _run(batch, True, True, 0.0, moves)
        assert lines[0].startswith(f"refused {E['HSDDP_ERR_ARG']} "), lines[0]
    lines = _run(batch, True, True, 0.0, [(0, el([5, 5, 5, 5]))], s_cap=23)  # S = 24 past the capacity
    assert lines[0].startswith(f"refused {E['HSDDP_ERR_ARG']} "), lines[0]


# ---- the C ABI -----------------------------------------------------------------------------------------
def test_symbols_and_null_handles():
    import hsddp
    from hsddp._lib import EXPORTS, IP
    E = _codes()
    L = hsddp.lib()
    V = C.c_void_p
    want = {"hsddp_copy_elements": ([V, V, C.c_int, IP, IP], C.c_int),
            "hsddp_element_record_bytes": ([V], C.c_size_t),
            "hsddp_export_elements": ([V, C.c_int, IP, V], C.c_int),
            "hsddp_import_elements": ([V, C.c_int, IP, V], C.c_int)}
    hdr = open(os.path.join(ROOT, "include", "hsddp.h")).read()
    for name, (args, res) in want.items():
        assert name in EXPORTS and re.search(r"\b" + name + r"\(", hdr)
        f = getattr(L, name)
        assert list(f.argtypes) == args and f.restype == res
    one = (C.c_int * 1)(0)
    buf = (C.c_char * 16)()
    assert L.hsddp_copy_elements(None, None, 1, one, one) == E["HSDDP_ERR_ARG"]
    assert L.hsddp_copy_elements(None, None, 0, None, None) == E["HSDDP_ERR_ARG"]
    assert L.hsddp_element_record_bytes(None) == 0
    assert L.hsddp_export_elements(None, 1, one, buf) == E["HSDDP_ERR_ARG"]
    assert L.hsddp_import_elements(None, 1, one, buf) == E["HSDDP_ERR_ARG"]
    assert L.hsddp_last_error()


# ---- the byte model ------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp32", [False, True])
@pytest.mark.parametrize("coincide", [True, False])
def test_bytes_per_moved_element(fp32, coincide):
    """traffic.element_move_bytes against a direct sum over DESIGN.md §2's buffers: (per state slot,
    per control slot, per phase, per element) bytes of every buffer an element carries"""
    from hsddp import traffic
    S, Kc, P, hist = 64, 60, 4, 3
    f = 4 if fp32 else 8
    table = {  # buffer: (bytes per slot, per knot, per phase, per element)
        "X3 nominal": (192, 0, 0, 0), "X3 working": (0 if coincide else 192, 0, 0, 0), "D3 working": (192, 0, 0, 0),
        "dX": (192, 0, 0, 0), "U3 nominal": (0, 192, 0, 0), "U3 working": (0, 0 if coincide else 192, 0, 0),
        "dU": (0, 192, 0, 0), "du": (0, 192, 0, 0), "K": (0, 12 * 24 * f, 0, 0),
        "reb_delta": (0, 160, 0, 0), "reb_eps": (0, 160, 0, 0), "cf_u": (0, 96, 0, 0), "cf_flag": (0, 4, 0, 0),
        "td_mask": (0, 0, 16, 0), "al_sigma": (0, 0, 128, 0), "al_lambda": (0, 0, 128, 0), "term_h": (0, 0, 32, 0),
        "slot_cost": (8, 0, 0, 0), "slot_feas": (8, 0, 0, 0), "slot_viol": (8, 0, 0, 0), "slot_div": (4, 0, 0, 0),
        "ref_x": (192, 0, 0, 0), "ref_u": (192, 0, 0, 0), "ref_foot": (96, 0, 0, 0),
        "def32": (96 if fp32 else 0, 0, 0, 0),
        "ElemState": (0, 0, 0, 160), "sel": (0, 0, 0, 4), "x0": (0, 0, 0, 192), "contacts": (0, 0, 16, 16),
        "hist": (0, 0, 0, 16 * hist),
    }
    read = sum(S * a + Kc * b + P * c + d for a, b, c, d in table.values())
    m = traffic.element_move_bytes(S, Kc, P, fp32, coincide, hist)
    assert m["read"] == read
    assert m["written"] == read + S * 480 + 272  # + ref_t's columns and the layout record
    assert m["total"] == m["read"] + m["written"]
    assert traffic.element_move_bytes(S, Kc, P, fp32, coincide, hist, in_place=False)["written"] == read + S * 480
