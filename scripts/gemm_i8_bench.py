"""Interleaved timing of the INT8 probe GEMM against the unscaled FP8 probe GEMM (same bytes per element).

Rounds alternate the arms in one process; every arm is timed with device events over ``--reps``
launches after a warm-up launch. Operations are 2*M*N*K for every arm (TOP/s for int8, TFLOP/s for f8;
the JSON fields keep the shared ``tflops`` names). Prints one JSON line per shape (median, best and
max - min spread per arm, and the int8 / f8 ratio of medians) and one line with the host time of a
``readiness_f8`` call per mode next to ``readiness``.
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
        abi = torch.empty((m + n, k), dtype=torch.int8, device=dev)
        ops.f8_fill(abi, seed=size + 2, kind="i8")
        ai, bi = abi[:m], abi[m:]
        out = torch.empty((m, n), device=dev, dtype=torch.float32)
        outi = torch.empty((m, n), device=dev, dtype=torch.int32)
        arms = {
            "int8": lambda: ops.gemm_i8_nt(ai, bi, out=outi),
            "f8_e4m3": lambda: ops.gemm_f8_nt(a8, b8, out=out),
        }
        med, fields = bench_arms(arms, 2.0 * m * n * k, args.rounds, args.reps)
        print(json.dumps({"shape": [m, n, k], "reps": args.reps, "rounds": args.rounds, **fields,
                          "int8_over_f8": round(med["int8"] / med["f8_e4m3"], 3)}), flush=True)
    print(json.dumps(readiness_host_ms(("fp8", "mxfp4", "int8"))), flush=True)


if __name__ == "__main__":
    main()
