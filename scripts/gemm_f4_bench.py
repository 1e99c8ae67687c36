"""Interleaved timing of the FP4 / MXFP4 probe GEMM against the FP8 / MXFP8 probe GEMM.

Rounds alternate the arms in one process; every arm is timed with device events over ``--reps``
launches after a warm-up launch. FLOPs are 2*M*N*K for every arm. Prints one JSON line per shape
(median, best and max - min spread of TFLOP/s per arm, and the mxfp4 / mxfp8 ratio of medians) and one
line with the host time of a ``readiness_f8`` call per mode next to ``readiness``.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from dcos_commons_amd import ops
from gemm_bench import bench_arms, readiness_host_ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,8192")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for size in (int(x) for x in args.sizes.split(",")):
        m = n = k = size
        ab8 = torch.empty((m + n, k), dtype=torch.uint8, device=dev)
        ops.f8_fill(ab8, seed=size, kind="e4m3")
        a8, b8 = ab8[:m].view(torch.float8_e4m3fn), ab8[m:].view(torch.float8_e4m3fn)
        ab4 = torch.empty((m + n, k // 2), dtype=torch.uint8, device=dev)
        ops.f8_fill(ab4, seed=size + 2, kind="e2m1")
        a4, b4 = ab4[:m], ab4[m:]
        sc = torch.empty((m + n, k // 32), dtype=torch.uint8, device=dev)
        ops.f8_fill(sc, seed=size + 1, kind="scale")
        out = torch.empty((m, n), device=dev, dtype=torch.float32)
        arms = {
            "mxfp4": lambda: ops.gemm_f4_nt(a4, b4, sc[:m], sc[m:], out=out),
            "f4": lambda: ops.gemm_f4_nt(a4, b4, out=out),
            "mxfp8": lambda: ops.gemm_f8_nt(a8, b8, sc[:m], sc[m:], out=out),
            "f8_e4m3": lambda: ops.gemm_f8_nt(a8, b8, out=out),
        }
        med, fields = bench_arms(arms, 2.0 * m * n * k, args.rounds, args.reps)
        print(json.dumps({"shape": [m, n, k], "reps": args.reps, "rounds": args.rounds, **fields,
                          "mxfp4_over_mxfp8": round(med["mxfp4"] / med["mxfp8"], 3)}), flush=True)
    print(json.dumps(readiness_host_ms(("fp8", "bf8", "mxfp8", "mxfp4"))), flush=True)


if __name__ == "__main__":
    main()
