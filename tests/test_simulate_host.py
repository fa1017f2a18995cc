"""Host-side checks of the policy simulation: the C and numpy layouts of hsddp_sim_sample agree,
and the NumPy restatement of hsddp_simulate_policy (tests/sim_reference.py) — the reference the
GPU tests compare against — equals the oracle's own rollout where the two compute the same thing.
"""
import os
import subprocess

import numpy as np

import hsddp
import oracle_lib as O
import sim_reference as R
from hsddp import synthetic as syn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sim_sample_layout_matches_c(tmp_path):
    fields = list(hsddp.SIM_SAMPLE.names)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "hsddp.h"\nint main(void){\n'
                   'printf("%zu\\n", sizeof(hsddp_sim_sample));\n' +
                   "".join(f'printf("%zu\\n", offsetof(hsddp_sim_sample, {f}));\n' for f in fields) +
                   "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    vals = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert vals[0] == 32 and hsddp.SIM_SAMPLE.itemsize == 32
    assert fields == ["cost", "min_grf", "max_td", "steps", "status"]
    assert vals[1:] == [hsddp.SIM_SAMPLE.fields[f][1] for f in fields]


def test_helper_matches_the_oracle_rollout():
    """Under MS = 0 a new problem's initial rollout (SinglePhase.cpp:181-233 at eps = 0) simulates
    phase 0 from X[0] = Xbar[0] with U = Ubar + K (X - Xbar) and the warm start's K: the helper's
    X, U over n <= N_0 steps from x_init = Xbar[0].  With an iteration budget of zero the oracle's
    solve is that rollout alone (its working rows X, U on return), so the two are fp64 compositions
    of the same C routines: 1e-12 relative."""
    B, P, N = 3, 2, 6
    prob = syn.make_batch(B, P, N, "trot")
    rng = np.random.default_rng(3)
    prob["Xbar"] = prob["Xbar"] + 0.01 * rng.standard_normal(prob["Xbar"].shape)
    prob["K"] = 0.5 * rng.standard_normal((B, prob["Kc"], 24, 24))
    r = O.solve_batch(prob, O.default_options(MS=0, max_AL_iter=0, max_DDP_iter=0), n_threads=1)
    assert np.all(r["diverged_init"] == 0)
    Xo, Uo = r["X"][:, :N + 1], r["U"][:, :N]  # phase 0
    assert np.all(np.isfinite(Xo)) and np.all(np.isfinite(Uo))
    assert np.all(np.sqrt(np.sum(Xo * Xo, axis=-1)) < 1e6)
    # the feedback acts: the rollout leaves the warm start (else K would not be exercised)
    assert np.max(np.abs(Uo - prob["Ubar"][:, :N])) > 1e-3
    ref = R.simulate(prob, {"Xbar": prob["Xbar"], "Ubar": prob["Ubar"], "K": prob["K"]},
                     prob["Xbar"][:, None, 0, :].copy(), N)
    assert np.all(ref["status"] == 0) and np.all(ref["steps"] == N)
    for n in (1, 3, N):
        q = R.prefix(ref, n)
        for b in range(B):
            sx = np.max(np.abs(Xo[b, :n])); su = np.max(np.abs(Uo[b, :n]))
            assert np.max(np.abs(q["X"][b, 0] - Xo[b, :n])) <= 1e-12 * sx, (n, b)
            assert np.max(np.abs(q["U"][b, 0] - Uo[b, :n])) <= 1e-12 * su, (n, b)
    # the state after knot n - 1 inside the phase is the oracle's next row
    q = R.prefix(ref, N - 1)
    assert np.max(np.abs(q["x_end"][:, 0] - Xo[:, N - 1])) <= 1e-12 * np.max(np.abs(Xo))


def test_prefix_of_a_diverged_sample():
    """prefix() on a sample that breaks the bound a few knots in (at knot k): calls with n <= k see
    no divergence, later ones stop there with the last accepted state."""
    prob = syn.make_batch(1, 2, 10, "trot")
    traj = {"Xbar": prob["Xbar"], "Ubar": prob["Ubar"], "K": np.zeros((1, prob["Kc"], 24, 24))}
    x = np.repeat(prob["Xbar"][:, None, 0, :], 2, axis=1)
    x[0, 1, 9] = 9.99e5  # v_x: pos_x grows by dt v_x per knot and the norm passes 1e6 inside phase 0
    ref = R.simulate(prob, traj, x, 8)
    assert ref["status"].tolist() == [[0, 1]]
    k = int(ref["steps"][0, 1])
    assert 0 < k < 8
    q = R.prefix(ref, k)
    assert q["status"][0, 1] == 0 and q["steps"][0, 1] == k
    q = R.prefix(ref, k + 1)
    assert q["status"][0, 1] == 1 and q["steps"][0, 1] == k
    assert np.array_equal(q["x_end"][0, 1], ref["after"][0, 1, k - 1])
    assert np.array_equal(q["X"][0, 1, k], ref["after"][0, 1, k - 1]) and np.all(ref["X"][0, 1, k + 1:] == 0)
