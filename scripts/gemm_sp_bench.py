"""Interleaved timing of the 2:4 sparse probe GEMM against the dense bf16 probe GEMM on the expanded A.

Rounds alternate the arms in one process; every arm is timed with device events over ``--reps``
launches after a warm-up launch. Operations are 2*M*N*K for both arms: dense-equivalent flops for the
sparse arm, which multiplies half of them. Both arms compute the same product (the sparse operands
are the ``bf16`` and ``meta24`` fills, the dense A is their ``sp24_expand``). Prints one JSON line per
shape (median, best and max - min spread of TFLOP/s per arm, the sparse / dense ratio of medians and the
relative Frobenius difference of the two products) and one line with the host time of a
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
        vb = torch.empty((n + m // 2, k), dtype=torch.bfloat16, device=dev)
        ops.readiness_fill(vb, seed=size)
        bt, vals = vb[:n], vb[n:].reshape(m, k // 2)
        meta = torch.empty((m, k // 8), dtype=torch.uint8, device=dev)
        ops.f8_fill(meta, seed=size + 1, kind="meta24")
        a = ops.sp24_expand(vals, meta)
        out = torch.empty((m, n), device=dev, dtype=torch.float32)
        ref = torch.empty((m, n), device=dev, dtype=torch.float32)
        arms = {
            "sparse24": lambda: ops.gemm_sp_bf16_nt(vals, meta, bt, out=out),
            "dense_glds256": lambda: ops.gemm_bf16_nt(a, bt, out=ref, variant="glds256"),
        }
        med, fields = bench_arms(arms, 2.0 * m * n * k, args.rounds, args.reps)
        rel = (torch.linalg.norm(out - ref) / torch.linalg.norm(ref)).item()
        print(json.dumps({"shape": [m, n, k], "reps": args.reps, "rounds": args.rounds, **fields,
                          "sparse24_over_dense": round(med["sparse24"] / med["dense_glds256"], 3),
                          "rel_diff_vs_dense": rel}), flush=True)
        del vb, meta, a, out, ref
    print(json.dumps(readiness_host_ms(("fp8", "fp64", "sparse24"))), flush=True)


if __name__ == "__main__":
    main()
