"""GPU readiness/health check for pods that are given MI355X GPUs.

Runs the HIP probe kernels on one device and decides healthy / unhealthy:

* **MFMA GEMM numerics** -- bf16 ``C = A @ Bt^T`` on the probe GEMM (256x256 LDS-DMA pipeline
  where the shape tiles, else 128x128) checked against the same bf16 values in fp32: the full
  probe compares with a dense fp32 matmul, the readiness probe with an fp32 VALU reference of
  every element computed on the device (``ops.readiness``, one native call). Relative error
  must stay < 1e-3;
* **FP8 / MXFP8 MFMA numerics** (opt-in, ``matrix=`` / ``--matrix``) -- the f8f6f4 matrix path and
  its E8M0 block-scale inputs, which the bf16 check never touches: ``ops.readiness_f8`` runs the
  f8 GEMM on hashed operands against a VALU reference of every element, per mode ``fp8`` (E4M3),
  ``bf8`` (E5M2), ``mxfp8`` (E4M3 with block scales), ``mxfp4`` (packed E2M1 with block scales: the
  ``cbsz:4 blgp:4`` FP4 decode and nibble routing, on a kernel of its own), ``int8`` (the integer MFMAs and
  their int32 accumulators, the W8A8 path: exact, a healthy device gives 0). Same < 1e-3 bound;
* **FP64 MFMA numerics** (opt-in, ``fp64``) -- ``v_mfma_f64_16x16x4_f64`` and its fp64 accumulators, the
  path HPC payloads run on: the f64 GEMM on hashed doubles against an fp64 VALU reference, the difference
  taken in fp64. Its bound is ``MAX_GEMM_F64_REL_ERR`` = 1e-10, not 1e-3: a product silently computed at
  single precision (2^-24) must fail;
* **2:4 sparse MFMA numerics** (opt-in, ``sparse24``) -- ``v_smfmac_f32_16x16x64_bf16``, whose per-lane index
  register drives a 2-of-4 operand mux that no dense instruction uses: the sparse GEMM on a compressed hashed A
  with hashed legal metadata, against the dense bf16 VALU check of the expanded A. The sparse product has the
  terms of the dense one, so the bound is the shared < 1e-3; a wrong index gives an O(1) error;
* **FP32 MFMA numerics** (opt-in, ``fp32``) -- ``v_mfma_f32_32x32x2_f32``, the single-precision multiplier array
  that every SGEMM lands on: the f32 GEMM on hashed floats against an fp32 VALU reference. Its bound is
  ``MAX_GEMM_F32_REL_ERR`` = 1e-5, not 1e-3: a product whose operands went through an 11-bit (tf32-like) path
  (2.6e-4) must fail;
* **MFMA rate** -- register-resident ``v_mfma_f32_32x32x16_bf16`` loop (TFLOP/s);
* **HBM** -- 16-B/lane streaming copy of a buffer larger than the 256 MiB Infinity Cache
  (read+write GB/s) and an address-hashed write/verify pattern (bad words must be 0).

``python -m dcos_commons_amd.ops.gpu_health --device 0 --json`` prints the report and exits 0
only when healthy; it is the readiness-check command used for GPU pods.
"""
from __future__ import annotations

import argparse
import json
import sys
import time

MIN_TFLOPS = 200.0       # far below the ~2.5 PF dense peak: catches a broken/throttled matrix pipe
MIN_HBM_GBPS = 1000.0    # far below the ~5.5 TB/s measured copy rate: catches a degraded stack
MAX_GEMM_REL_ERR = 1e-3
# The fp64 mode's own bound, for the readiness K of 128 (ops.READINESS_F64_SHAPE). It sits between two levels.
# Healthy: the GEMM and the VALU reference are both fp64 sums of K terms in different orders, each within
# K * 2^-53 * sum|a||b| of exact; for the hashed fill (mixed signs, |x| in [0.5, 1)) the norm of sum|a||b| over
# the norm of sum(ab) is about sqrt(K), so the relative Frobenius error is at most about 2 * K^1.5 * 2^-53,
# 3e-13 at K = 128. Faulty: a product rounded once through fp32 is off by about 2^-24 = 6e-8 per element, which
# the shared 1e-3 would pass. 1e-10 is near the geometric middle of the two (1.4e-10).
MAX_GEMM_F64_REL_ERR = 1e-10
# The fp32 mode's own bound, for the readiness K of 128 (ops.READINESS_F32_SHAPE). It sits between two levels.
# Faulty: a product whose operands were rounded to 11 significant bits (a tf32 / xf32-like path) is off by 2.6e-4
# relative Frobenius on hashed-fill-like values, the same at K = 128, 256 and 512 (computed on the CPU in float64;
# bf16-rounded operands give 2.1e-3). The shared 1e-3 would pass it. Healthy: the GEMM and the VALU reference are
# both fp32 sums of 128 terms in different orders; two sequential fp32 sums in different orders differ by about
# 2.5e-7 (a CPU estimate), and readiness_f8(mode="fp32") on a healthy MI355X measured 2.28e-7 to 2.33e-7 over 24
# seeds (profiles/gemm_f32.md). The geometric mean of 2.33e-7 and 2.6e-4 is 7.8e-6; 1e-5 is the power of ten
# nearest to it, 43x above the measured maximum and 26x below the faulty level.
MAX_GEMM_F32_REL_ERR = 1e-5
# bf16 is always checked; the rest are opt-in
MATRIX_MODES = ("bf16", "fp8", "bf8", "mxfp8", "mxfp4", "int8", "fp64", "sparse24", "fp32")


def _max_rel_err(mode: str) -> float:
    return {"fp64": MAX_GEMM_F64_REL_ERR, "fp32": MAX_GEMM_F32_REL_ERR}.get(mode, MAX_GEMM_REL_ERR)


def _f8_modes(matrix) -> list:
    unknown = [m for m in matrix if m not in MATRIX_MODES]
    if unknown:
        raise ValueError(f"unknown matrix mode(s) {unknown}: {list(MATRIX_MODES)}")
    return [m for m in MATRIX_MODES[1:] if m in matrix]


def readiness_probe(device: int = 0, matrix=("bf16",)) -> dict:
    """The fast form used as a pod readiness check: numerics + memory integrity only, as ONE
    native call (``ops.readiness``): hashed bf16 operands, the MFMA GEMM, a dense fp32 check of
    every product element and the 64 MiB pattern test on a private stream with a single read-back. It sits on the deploy and
    recovery critical path of every GPU pod, and the GIL is released while it runs. Each of ``fp8``, ``bf8``,
    ``mxfp8``, ``mxfp4``, ``int8``, ``fp64``, ``sparse24``, ``fp32`` in ``matrix`` adds one ``ops.readiness_f8`` call and a ``gemm_<mode>_rel_err`` field."""
    from dcos_commons_amd import ops

    t0 = time.perf_counter()
    rel, bad = ops.readiness(device, seed=4321 + device)
    rep = {"device": device, "gemm_rel_err": rel, "mem_bad_words": bad}
    healthy = rel < MAX_GEMM_REL_ERR and bad == 0
    for mode in _f8_modes(matrix):
        rel8 = ops.readiness_f8(device, seed=4321 + device, mode=mode)
        rep[f"gemm_{mode}_rel_err"] = rel8
        healthy = healthy and rel8 < _max_rel_err(mode)
    rep["healthy"] = bool(healthy)
    rep["probe_seconds"] = round(time.perf_counter() - t0, 4)
    return rep


def run_probe(device: int = 0, quick: bool = True, matrix=("bf16",)) -> dict:
    import torch

    from dcos_commons_amd import ops

    t_start = time.perf_counter()
    torch.cuda.set_device(device)
    dev = torch.device("cuda", device)
    props = torch.cuda.get_device_properties(dev)
    report = {"device": device, "name": props.name, "arch": getattr(props, "gcnArchName", ""),
              "total_mem_gib": round(props.total_memory / 2**30, 1), "cus": props.multi_processor_count}
    g = torch.Generator(device=dev)
    g.manual_seed(1234 + device)

    # 1. MFMA GEMM numerics
    m = n = 512 if quick else 2048
    k = 1024 if quick else 4096
    a = torch.randn((m, k), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    bt = torch.randn((n, k), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    c = ops.gemm_bf16_nt(a, bt)
    ref = a.float() @ bt.float().t()
    rel = float(torch.linalg.norm(c - ref) / torch.linalg.norm(ref))
    report["gemm_rel_err"] = rel

    # GEMM throughput on a square shape
    s = 2048 if quick else 8192
    a2 = torch.randn((s, s), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    b2 = torch.randn((s, s), generator=g, device=dev, dtype=torch.float32).to(torch.bfloat16)
    out = torch.empty((s, s), dtype=torch.float32, device=dev)
    ops.gemm_bf16_nt(a2, b2, out)
    reps = 5 if quick else 10
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        ops.gemm_bf16_nt(a2, b2, out)
    e1.record()
    e1.synchronize()
    report["gemm_tflops"] = round(2.0 * s * s * s * reps / (e0.elapsed_time(e1) / 1e3) / 1e12, 1)
    f8_ok = True
    for mode in _f8_modes(matrix):
        # numerics through the native check (hashed operands), throughput on the same square shape
        rel8 = ops.readiness_f8(device, seed=1234 + device, mode=mode)
        report[f"gemm_{mode}_rel_err"] = rel8
        f8_ok = f8_ok and rel8 < _max_rel_err(mode)
        if mode == "int8":
            ab8 = torch.empty((2 * s, s), dtype=torch.int8, device=dev)
            ops.f8_fill(ab8, seed=1234 + device, kind="i8")
            out32 = torch.empty((s, s), dtype=torch.int32, device=dev)
            ops.gemm_i8_nt(ab8[:s], ab8[s:], out=out32)
            e0.record()
            for _ in range(reps):
                ops.gemm_i8_nt(ab8[:s], ab8[s:], out=out32)
            e1.record()
            e1.synchronize()
            report["gemm_int8_tops"] = round(2.0 * s * s * s * reps / (e0.elapsed_time(e1) / 1e3) / 1e12, 1)
            del ab8, out32
            continue
        if mode == "fp64":
            ab64 = torch.empty((2 * s, s), dtype=torch.float64, device=dev)
            ops.f8_fill(ab64, seed=1234 + device, kind="f64")
            out64 = torch.empty((s, s), dtype=torch.float64, device=dev)
            ops.gemm_f64_nt(ab64[:s], ab64[s:], out=out64)
            e0.record()
            for _ in range(reps):
                ops.gemm_f64_nt(ab64[:s], ab64[s:], out=out64)
            e1.record()
            e1.synchronize()
            report["gemm_fp64_tflops"] = round(2.0 * s * s * s * reps / (e0.elapsed_time(e1) / 1e3) / 1e12, 1)
            del ab64, out64
            continue
        if mode == "fp32":
            ab32 = torch.empty((2 * s, s), dtype=torch.float32, device=dev)
            ops.f8_fill(ab32, seed=1234 + device, kind="f32")
            ops.gemm_f32_nt(ab32[:s], ab32[s:], out=out)
            e0.record()
            for _ in range(reps):
                ops.gemm_f32_nt(ab32[:s], ab32[s:], out=out)
            e1.record()
            e1.synchronize()
            report["gemm_fp32_tflops"] = round(2.0 * s * s * s * reps / (e0.elapsed_time(e1) / 1e3) / 1e12, 1)
            del ab32
            continue
        if mode == "sparse24":
            # gemm_sparse24_tflops counts 2 * s^3, the flops of the dense product of the same square shape
            # (dense-equivalent: the kernel multiplies half of them)
            vb = torch.empty((s + s // 2, s), dtype=torch.bfloat16, device=dev)
            ops.readiness_fill(vb, seed=1234 + device)
            va, vbt = vb[s:].reshape(s, s // 2), vb[:s]
            vm = torch.empty((s, s // 8), dtype=torch.uint8, device=dev)
            ops.f8_fill(vm, seed=1234 + device, kind="meta24")
            ops.gemm_sp_bf16_nt(va, vm, vbt, out=out)
            e0.record()
            for _ in range(reps):
                ops.gemm_sp_bf16_nt(va, vm, vbt, out=out)
            e1.record()
            e1.synchronize()
            report["gemm_sparse24_tflops"] = round(2.0 * s * s * s * reps / (e0.elapsed_time(e1) / 1e3) / 1e12, 1)
            del vb, va, vbt, vm
            continue
        dt = torch.uint8 if mode == "mxfp4" else torch.float8_e5m2 if mode == "bf8" else torch.float8_e4m3fn
        ab8 = torch.empty((2 * s, s // 2 if mode == "mxfp4" else s), dtype=torch.uint8, device=dev)
        ops.f8_fill(ab8, seed=1234 + device, kind={"bf8": "e5m2", "mxfp4": "e2m1"}.get(mode, "e4m3"))
        a8, b8 = ab8[:s].view(dt), ab8[s:].view(dt)
        sc = None
        if mode in ("mxfp8", "mxfp4"):
            sc = torch.empty((2 * s, s // 32), dtype=torch.uint8, device=dev)
            ops.f8_fill(sc, seed=4321 + device, kind="scale")
        run8 = (lambda: ops.gemm_f4_nt(a8, b8, sc[:s], sc[s:], out=out)) if mode == "mxfp4" else \
            (lambda: ops.gemm_f8_nt(a8, b8, sc[:s], sc[s:], out=out)) if sc is not None else \
            (lambda: ops.gemm_f8_nt(a8, b8, out=out))
        run8()
        e0.record()
        for _ in range(reps):
            run8()
        e1.record()
        e1.synchronize()
        report[f"gemm_{mode}_tflops"] = round(2.0 * s * s * s * reps / (e0.elapsed_time(e1) / 1e3) / 1e12, 1)
        del ab8, a8, b8, sc
    del a2, b2, out

    # 2. MFMA issue rate
    secs, flops = ops.mfma_peak(device, blocks=2048, iters=512 if quick else 4096)
    report["mfma_tflops"] = round(flops / secs / 1e12, 1)

    # 3. HBM bandwidth (buffers larger than the Infinity Cache)
    nbytes = (512 if quick else 2048) * 2**20
    src = torch.empty(nbytes // 4, dtype=torch.int32, device=dev)
    dst = torch.empty_like(src)
    ops.pattern_write(src, seed=7)
    ops.hbm_copy(src, dst)
    reps = 5
    e0.record()
    for _ in range(reps):
        ops.hbm_copy(src, dst)
    e1.record()
    e1.synchronize()
    report["hbm_copy_gbps"] = round(2.0 * nbytes * reps / (e0.elapsed_time(e1) / 1e3) / 1e9, 1)

    # 4. HBM integrity: the copy must preserve the pattern, and a fresh pattern must verify
    bad = ops.pattern_check(dst, seed=7)
    ops.pattern_write(src, seed=99)
    bad += ops.pattern_check(src, seed=99)
    report["mem_bad_words"] = bad
    del src, dst
    torch.cuda.synchronize(dev)

    report["healthy"] = bool(rel < MAX_GEMM_REL_ERR and f8_ok and bad == 0 and report["mfma_tflops"] > MIN_TFLOPS and
                             report["hbm_copy_gbps"] > MIN_HBM_GBPS)
    report["probe_seconds"] = round(time.perf_counter() - t_start, 3)
    return report


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--full", action="store_true", help="larger shapes (slower, more precise)")
    ap.add_argument("--readiness", action="store_true", help="fast numerics + memory check only")
    ap.add_argument("--matrix", default="bf16", help="comma-separated matrix data paths to check: bf16 (always), "
                    "fp8, bf8, mxfp8, mxfp4, int8, fp64, sparse24, fp32")
    ap.add_argument("--json", action="store_true")
    args = ap.parse_args(argv)
    matrix = tuple(m for m in args.matrix.split(",") if m)
    rep = readiness_probe(args.device, matrix) if args.readiness else \
        run_probe(args.device, quick=not args.full, matrix=matrix)
    print(json.dumps(rep) if args.json else "\n".join(f"{k}: {v}" for k, v in rep.items()))
    return 0 if rep["healthy"] else 1


if __name__ == "__main__":
    sys.exit(main())
