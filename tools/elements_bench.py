#!/usr/bin/env python3
"""Element-move benchmark: hsddp_copy_elements between two live handles of B
robots on the bench's trot 4 x 50 problem with per-element references and layouts (so the moves are
patched in place), and a fan-out of one robot over n slots within one handle.  Per case: a warm-up,
then --runs calls; the call's wall time (the call returns synchronised) and the kernels' device time
(HSDDP_COPY_TIMING=1, parsed from the library's stderr line), medians, beside the byte model
(traffic.element_move_bytes: bytes read plus bytes written per element) as achieved TB/s.

    python tools/elements_bench.py [--batch B] [--moved 1,41,4096] [--fanout 41] [--runs 5]  -> JSON lines

The handles hold new problems with their default warm start (nominal and working rows in one
buffer, no solver-info entries), which fixes the byte count per element.
"""
import argparse
import json
import os
import re
import sys
import tempfile
import time

os.environ["HSDDP_COPY_TIMING"] = "1"

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (binds the library to torch's HIP runtime, as bench.py does)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hkd-mpc_amd"))
import hsddp  # noqa: E402
from hsddp import synthetic, traffic  # noqa: E402


class Stderr:
    """the process's stderr (the C library's too) into a file while the block runs"""

    def __enter__(self):
        self.f = tempfile.TemporaryFile(mode="w+")
        sys.stderr.flush()
        self.saved = os.dup(2)
        os.dup2(self.f.fileno(), 2)
        return self

    def __exit__(self, *exc):
        os.dup2(self.saved, 2)
        os.close(self.saved)
        self.f.seek(0)
        self.text = self.f.read()
        self.f.close()


def handle(B):
    p = synthetic.make_batch(B, 4, 50, "trot")
    for k in ("ref_x", "ref_u", "ref_foot"):  # per-element references
        p[k] = np.ascontiguousarray(np.repeat(p[k], B, axis=0))
    p["layouts"] = [list(p["horizons"])] * B   # per-element layouts: a move is patched in place
    return hsddp.Solver(p, hsddp.load_settings()), p


def timed(dst, src, di, si, runs):
    wall, kern = [], []
    for it in range(runs + 1):  # (the first call is the warm-up)
        with Stderr() as err:
            t0 = time.perf_counter()
            dst.copy_elements(src, di, si)
            t1 = time.perf_counter()
        m = re.findall(r"kernels ms: ([0-9.]+) \(([^)]*)\)", err.text)
        assert len(m) == 1, err.text
        if it:
            wall.append((t1 - t0) * 1e3)
            kern.append(float(m[0][0]))
        note = m[0][1]
    return wall, kern, note


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--moved", default="1,41,4096")
    ap.add_argument("--fanout", type=int, default=41)
    ap.add_argument("--runs", type=int, default=5)
    args = ap.parse_args()
    B = args.batch
    src, p = handle(B)
    dst, _ = handle(B)
    per = traffic.element_move_bytes(p["S"], p["Kc"], len(p["horizons"]), False, True, 0, True)
    rng = np.random.default_rng(5)

    def report(mode, n, wall, kern, note):
        k = float(np.median(kern))
        print(json.dumps({"metric": "element move, trot 4 x 50", "mode": mode, "batch": B, "moved": n,
                          "call_ms_median": float(np.median(wall)), "kernels_ms_median": k, "kernels_ms": kern,
                          "bytes_per_element": per, "model_TB_per_s": per["total"] * n / (k * 1e-3) / 1e12,
                          "library_note": note}), flush=True)

    for n in (int(v) for v in args.moved.split(",")):
        n = min(n, B)
        di = np.sort(rng.choice(B, n, replace=False)).astype(np.int32)
        si = np.sort(rng.choice(B, n, replace=False)).astype(np.int32)
        report("copy between two handles", n, *timed(dst, src, di, si, args.runs))
    if args.fanout > 0 and args.fanout < B:
        n = args.fanout
        report("fan-out of one robot within one handle", n,
               *timed(dst, dst, np.arange(1, n + 1, dtype=np.int32), np.zeros(n, np.int32), args.runs))
    src.close()
    dst.close()


if __name__ == "__main__":
    main()
