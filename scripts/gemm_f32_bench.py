"""Interleaved timing of the FP32 probe GEMM against torch.matmul (the vendor SGEMM) on the same operands.

Rounds alternate the arms in one process; every arm is timed with device events over ``--reps``
launches after a warm-up launch. Operations are 2*M*N*K for both arms. Prints one JSON line per shape
(median, best and max - min spread of TFLOP/s per arm, the f32 / matmul ratio of medians and the
relative Frobenius difference of the two products), one line with the ``rel_err`` of
``readiness_f8(mode="fp32")`` over ``--seeds`` seeds (the healthy level that
``gpu_health.MAX_GEMM_F32_REL_ERR`` is set against) and one line with the host time of a
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seeds", type=int, default=16)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    # the vendor arm must be an fp32 SGEMM, not a tf32 one
    torch.backends.cuda.matmul.allow_tf32 = False
    for size in (int(x) for x in args.sizes.split(",")):
        m = n = k = size
        ab = torch.empty((m + n, k), dtype=torch.float32, device=dev)
        ops.f8_fill(ab, seed=size, kind="f32")
        a, bt = ab[:m], ab[m:]
        out = torch.empty((m, n), device=dev, dtype=torch.float32)
        ref = torch.empty((m, n), device=dev, dtype=torch.float32)
        arms = {
            "f32": lambda: ops.gemm_f32_nt(a, bt, out=out),
            "torch_matmul": lambda: torch.matmul(a, bt.t(), out=ref),
        }
        med, fields = bench_arms(arms, 2.0 * m * n * k, args.rounds, args.reps)
        rel = (torch.linalg.norm(out.double() - ref.double()) / torch.linalg.norm(ref.double())).item()
        print(json.dumps({"shape": [m, n, k], "reps": args.reps, "rounds": args.rounds, **fields,
                          "f32_over_matmul": round(med["f32"] / med["torch_matmul"], 3),
                          "rel_diff_vs_matmul": rel}), flush=True)
        del ab, out, ref
    rels = [ops.readiness_f8(0, seed, "fp32") for seed in range(args.seeds)]
    print(json.dumps({"readiness_fp32_rel_err": rels, "max": max(rels), "min": min(rels)}), flush=True)
    print(json.dumps(readiness_host_ms(("fp8", "int8", "fp64", "fp32"))), flush=True)


if __name__ == "__main__":
    main()
