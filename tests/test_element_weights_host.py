"""Per-robot weights (hsddp_set_element_weights): what needs no GPU.

tests/drivers/element_weights_check (g++ from hsddp_dispatch.h and hsddp_phases.cpp alone): the
launchers' dispatch with two optional tables — tests/test_dispatch_host.py's combinations extended by
the weight table — and the element record's weight row.  The NULL-handle refusals of the two entry
points through the library, which initialises no device for them."""
import ctypes as C
import os
import subprocess

import hsddp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "tests", "drivers")


def _lines():
    r = subprocess.run(["make", "-C", DRIVERS, "-f", "element_weights.mk", "element_weights_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(DRIVERS, "element_weights_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [ln.split() for ln in r.stdout.splitlines()]


def test_every_flag_and_table_combination_reaches_its_instantiation_once():
    """with_flags_tables: for N = 0 .. 4 flags, each of the 2^N combinations and each of the four
    (terrain, weights) cases the callable runs once, its constants equal the flags in argument order
    and the pack after them is (), (terrain), (weights) or (terrain, weights) — a weights
    instantiation launched without its table, or a plain one with it, would read the wrong argument."""
    seen = {}
    for ln in (l for l in _lines() if l[0] != "export"):
        n, flags, calls, consts, terrain, weights, pack = (int(v) for v in ln)
        assert calls == 1 and consts == flags, ln
        assert pack == terrain + 2 * weights, ln
        seen.setdefault((n, flags), set()).add((terrain, weights))
    for n in range(5):
        for flags in range(1 << n):
            assert seen.get((n, flags)) == {(0, 0), (1, 0), (0, 1), (1, 1)}, (n, flags)


def test_record_header_carries_the_row_only_while_the_table_is_on():
    ex = [l for l in _lines() if l[0] == "export"]
    assert len(ex) == 6
    for _, b, has, first, last in ex[:3]:
        assert (int(has), float(first), float(last)) == (0, 0.0, 0.0)
    for _, b, has, first, last in ex[3:]:
        assert int(has) == 1 and float(first) == 1.0 + 46 * int(b) and float(last) == 46.0 + 46 * int(b)


def test_null_handle_is_refused():
    """HSDDP_ERR_ARG (-1) from both entry points, with a table, with NULL (table off) and on the read"""
    L = hsddp.lib()
    w = (hsddp.Weights * 2)()
    assert L.hsddp_set_element_weights(None, C.addressof(w), None) == -1
    assert L.hsddp_set_element_weights(None, None, None) == -1
    assert L.hsddp_get_element_weights(None, C.addressof(w)) == -1
    assert C.sizeof(hsddp.Weights) == 46 * 8
