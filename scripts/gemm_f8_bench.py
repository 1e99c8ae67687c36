"""Interleaved timing of the FP8 / MXFP8 probe GEMM against the bf16 probe GEMM variants.

Rounds alternate the arms in one process; every arm is timed with device events over ``--reps``
launches after a warm-up launch. FLOPs are 2*M*N*K for every arm. Prints one JSON line per shape
(median, best and spread of TFLOP/s per arm, and the f8 / tile128 ratio: same tile shape, half the
bytes per K element) and one line with the host time of a ``readiness_f8`` call next to ``readiness``.
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
        g = torch.Generator(device=dev)
        g.manual_seed(size)
        a = (torch.rand((m, k), generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
        bt = (torch.rand((n, k), generator=g, device=dev) * 2 - 1).to(torch.bfloat16)
        ab8 = torch.empty((m + n, k), dtype=torch.uint8, device=dev)
        ops.f8_fill(ab8, seed=size, kind="e4m3")
        a8, b8 = ab8[:m].view(torch.float8_e4m3fn), ab8[m:].view(torch.float8_e4m3fn)
        sc = torch.empty((m + n, k // 32), dtype=torch.uint8, device=dev)
        ops.f8_fill(sc, seed=size + 1, kind="scale")
        out = torch.empty((m, n), device=dev, dtype=torch.float32)
        arms = {
            "f8_e4m3": lambda: ops.gemm_f8_nt(a8, b8, out=out),
            "mxfp8": lambda: ops.gemm_f8_nt(a8, b8, sc[:m], sc[m:], out=out),
            "bf16_tile128": lambda: ops.gemm_bf16_nt(a, bt, out, variant="tile128"),
            "bf16_glds256": lambda: ops.gemm_bf16_nt(a, bt, out, variant="glds256"),
        }
        med, fields = bench_arms(arms, 2.0 * m * n * k, args.rounds, args.reps)
        print(json.dumps({"shape": [m, n, k], "reps": args.reps, "rounds": args.rounds, **fields,
                          "f8_over_tile128": round(med["f8_e4m3"] / med["bf16_tile128"], 3),
                          "mxfp8_over_tile128": round(med["mxfp8"] / med["bf16_tile128"], 3)}), flush=True)
    print(json.dumps(readiness_host_ms(("fp8", "bf8", "mxfp8"))), flush=True)


if __name__ == "__main__":
    main()
