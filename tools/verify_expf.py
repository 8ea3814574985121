#!/usr/bin/env python3
"""Exhaustive check of rt_expf (csrc/rt_math.hpp) on the CPU, through the host batch rt_expf_batch: the worst error in fp32 ulp against float64
exp over EVERY fp32 x in [-87, 0] (1.12e9 values), and the contract on the way: rt_expf(+-0) == 1, 0 for x <= -87 and NaN, every result in [0, 1], none denormal.
float64 exp is within one float64 ulp, 2^-29 of an fp32 one.  Prints a progress line per chunk and the figure the CPU test asserts against.

    python tools/verify_expf.py [--chunk 16777216] > profiles/e26_expf_exhaustive.txt
"""
import argparse, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as G


def ulp_error(x, y):
    """|y - exp(x)| in units of the fp32 spacing at exp(x): (errors float64, reference float64)"""
    ref = np.exp(x.astype(np.float64))
    ulp = np.ldexp(1.0, np.frexp(ref)[1] - 1 - 23)
    return np.abs(y.astype(np.float64) - ref) / ulp, ref


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunk", type=int, default=1 << 24)
    args = ap.parse_args()
    p = G.load_package()
    t0 = time.time()
    lo, hi = 0x80000000, int(np.array(-87.0, np.float32).view(np.uint32))   # the bit patterns of -0 ... -87, ascending with |x|
    worst, worst_x, bad = 0.0, 0.0, 0
    for first in range(lo, hi + 1, args.chunk):
        bits = np.arange(first, min(first + args.chunk, hi + 1), dtype=np.uint32)
        x = bits.view(np.float32)
        y = p.api.expf_batch(x)
        live = x > np.float32(-87.0)
        err, _ = ulp_error(x[live], y[live])
        k = int(np.argmax(err)) if len(err) else 0
        if len(err) and err[k] > worst:
            worst, worst_x = float(err[k]), float(x[live][k])
        tiny = np.float32(np.finfo(np.float32).tiny)
        bad += int((~(y >= 0) | ~(y <= 1)).sum()) + int((y[live] < tiny).sum()) + int((y[~live] != 0).sum())
        print(f"x bits [{first:#010x}, {int(bits[-1]) + 1:#010x}): worst so far {worst:.4f} ulp at x = {worst_x!r}, contract violations {bad}  ({time.time() - t0:.0f}s)", flush=True)
    edge = p.api.expf_batch(np.array([0.0, -0.0, np.nan, -np.inf, -88.0, -1e30], np.float32))
    bad += int(not (edge[0] == 1 and edge[1] == 1 and (edge[2:] == 0).all()))
    print(f"WORST {worst:.6f} ulp at x = {worst_x!r} ({np.float32(worst_x).view(np.uint32):#010x}) over {hi - lo + 1} values; contract violations {bad}; {time.time() - t0:.0f}s")
    sys.exit(1 if bad else 0)
