"""The launchers' dispatch helper (hkd-mpc_amd/csrc/hsddp_dispatch.h) without HIP or a GPU:
tests/drivers/dispatch_check is built by g++ from that header alone.

with_flags turns N runtime flags into N std::bool_constant arguments of the callable that launches a
kernel instantiation.  A swapped or dropped flag would launch, for instance, a per-element-layout
kernel on a handle without layouts, so for N = 0 .. 4 and every one of the 2^N combinations the
callable must run exactly once with constants equal to the flags, in argument order;
with_flags_table must pass the terrain table after the constants exactly when it is non-null."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVERS = os.path.join(ROOT, "tests", "drivers")


def _lines():
    r = subprocess.run(["make", "-C", DRIVERS, "dispatch_check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([os.path.join(DRIVERS, "dispatch_check")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]


def test_every_flag_combination_reaches_its_instantiation_once():
    lines = _lines()
    # per combination: with_flags, with_flags_table without and with a table
    seen = {}
    for n, flags, calls, consts, table, at in lines:
        assert calls == 1, (n, flags, calls)
        assert consts == flags, (n, flags, consts)
        assert at == (n if table else -1), (n, flags, table, at)
        seen.setdefault((n, flags), []).append(table)
    for n in range(5):
        for flags in range(1 << n):
            assert seen.get((n, flags), [])[:3] == [0, 0, 1], (n, flags)
    # the two integer-flag cases on top of the 2^N bool ones (N = 2: flags 1 and 2 seen twice)
    assert len(lines) == 3 * (sum(1 << n for n in range(5)) + 2)
