"""Host-side checks of the measured-state ingest: the C and numpy layouts of hsddp_robot_state agree
and the built library exports the three entry points (no GPU needed: symbols resolve at load)."""
import ctypes
import os
import subprocess

import hsddp
from hsddp import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["p", "vWorld", "rpy", "omegaBody", "qJ", "foot_placements"]  # lcmtypes/hkd_data_lcmt.lcm's order


def test_robot_state_layout_matches_c(tmp_path):
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hsddp.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(hsddp_robot_state));\n' +
                   "".join(f'printf("%zu\\n", offsetof(hsddp_robot_state, {f}));\n' for f in FIELDS) +
                   "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == 144 and hsddp.ROBOT_STATE.itemsize == 144
    assert list(hsddp.ROBOT_STATE.names) == FIELDS
    assert vals[1:] == [hsddp.ROBOT_STATE.fields[f][1] for f in FIELDS]
    assert vals[1:] == [0, 12, 24, 36, 48, 96]


def test_measured_symbols_resolve():
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("hsddp_hkd_state", "hsddp_update_problem_measured", "hsddp_extract_commands_measured"):
        assert name in _lib.EXPORTS
        assert getattr(L, name) is not None
