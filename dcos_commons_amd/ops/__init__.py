"""MI355X device ops: HIP probe kernels behind a torch-tensor API.

The kernels live in seven files under ``csrc/``:

* ``probe_kernels.hip``: MFMA bf16 GEMM, MFMA issue-rate loop, HBM streaming copy, HBM pattern test,
  the hashed operand fill and the shared parts of the dense VALU check;
* ``f8_kernels.hip``: FP8 / MXFP8 MFMA GEMM and its check;
* ``f4_kernels.hip``: FP4 / MXFP4 MFMA GEMM and its check;
* ``i8_kernels.hip``: INT8 MFMA GEMM (int32 accumulators) and its exact check;
* ``f64_kernels.hip``: FP64 MFMA GEMM (``v_mfma_f64_16x16x4_f64``, fp64 accumulators), its check, which
  subtracts in fp64, and the hashed fp64 operand fill;
* ``sp_kernels.hip``: 2:4 sparse bf16 MFMA GEMM (``v_smfmac_f32_16x16x64_bf16``) on a compressed A, the VALU
  expansion of a compressed A to dense (the dense bf16 check then serves as its reference) and the hashed
  metadata fill;
* ``f32_kernels.hip``: FP32 MFMA GEMM (``v_mfma_f32_32x32x2_f32``, 4-byte operands) and its check against an
  fp32 VALU reference; its operands come from the shared hashed fill with an fp32 mask pair.

They are compiled for gfx950 into the in-tree ``_amdprobe.so`` (``python -m dcos_commons_amd.ops.build``)
and back the GPU readiness/health check that gates pods which request ``gpus``
(``dcos_commons_amd.ops.gpu_health``).

There is deliberately no PyTorch fallback: on a machine with a GPU, a missing or stale
extension raises ``ProbeUnavailable`` instead of silently running something else.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_amdprobe.so")
_lib: Optional[ctypes.CDLL] = None
_lock = threading.Lock()

GEMM_TILE_M = 128
GEMM_TILE_N = 128
GEMM_TILE_K = 64


class ProbeUnavailable(RuntimeError):
    pass


class ProbeError(RuntimeError):
    pass


def _bind(lib: ctypes.CDLL) -> None:
    vp, i, u, sz, f, d = (ctypes.c_void_p, ctypes.c_int, ctypes.c_uint, ctypes.c_size_t, ctypes.c_float,
                          ctypes.c_double)
    pd, pull = ctypes.POINTER(d), ctypes.POINTER(ctypes.c_ulonglong)
    for name, restype, argtypes in (
            ("version", i, None),
            ("gemm_bf16_nt", i, [vp, vp, vp, i, i, i, vp]),
            ("gemm_bf16_nt_variant", i, [vp, vp, vp, i, i, i, i, vp]),
            ("mfma_peak", i, [vp, i, i, f, vp]),
            ("mfma_peak_flops", d, [i, i]),
            ("hbm_copy", i, [vp, vp, sz, i, vp]),
            ("pattern_write", i, [vp, sz, u, i, vp]),
            ("pattern_check", i, [vp, sz, u, vp, i, vp]),
            ("gemm_check", i, [vp, vp, vp, i, i, i, i, vp, vp]),
            ("readiness_fill", i, [vp, sz, u, vp, vp]),
            ("readiness", i, [i, u, i, pd, pull]),
            ("gemm_f8_nt", i, [vp, vp, vp, i, i, i, i, i, vp, vp, vp]),
            ("gemm_f8_check", i, [vp, vp, vp, i, i, i, i, i, vp, vp, i, vp, vp]),
            ("f8_fill", i, [vp, sz, u, i, vp, vp]),
            ("gemm_f4_nt", i, [vp, vp, vp, i, i, i, vp, vp, vp]),
            ("gemm_f4_check", i, [vp, vp, vp, i, i, i, vp, vp, i, vp, vp]),
            ("gemm_i8_nt", i, [vp, vp, vp, i, i, i, vp]),
            ("gemm_i8_check", i, [vp, vp, vp, i, i, i, i, vp, vp]),
            ("gemm_f64_nt", i, [vp, vp, vp, i, i, i, vp]),
            ("gemm_f64_check", i, [vp, vp, vp, i, i, i, i, vp, vp]),
            ("gemm_sp_bf16_nt", i, [vp, vp, vp, vp, i, i, i, vp]),
            ("sp24_expand", i, [vp, vp, vp, i, i, vp]),
            ("gemm_f32_nt", i, [vp, vp, vp, i, i, i, vp]),
            ("gemm_f32_check", i, [vp, vp, vp, i, i, i, i, vp, vp]),
            ("readiness_f8", i, [i, u, i, i, pd])):
        fn = getattr(lib, "amdprobe_" + name)
        fn.restype = restype
        if argtypes is not None:
            fn.argtypes = argtypes


def lib() -> ctypes.CDLL:
    global _lib
    if _lib is None:
        with _lock:
            if _lib is None:
                if not os.path.exists(LIB_PATH):
                    raise ProbeUnavailable(f"{LIB_PATH} is not built; run `python -m dcos_commons_amd.ops.build`")
                l = ctypes.CDLL(LIB_PATH)
                _bind(l)
                _lib = l
    return _lib


def _stream(device=None):
    import torch

    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _check(rc: int, what: str) -> None:
    if rc == -1:
        raise ProbeError(f"{what}: shape rejected by the kernel's launch contract")
    if rc == -2:
        raise ProbeError(f"{what}: operands must be 16-byte aligned")
    if rc != 0:
        raise ProbeError(f"{what}: HIP error {rc}")


F8_TILE = 128                       # M, N and K granule of gemm_f8_nt
F8_BLOCK = 32                       # K elements per E8M0 block scale
F8_FILL_KINDS = {"e4m3": 0, "e5m2": 1, "scale": 2, "e2m1": 3, "i8": 3, "f64": 5, "meta24": 6,
                 "f32": 7}          # i8: the any-byte fill
READINESS_F8_MODES = {"fp8": 0, "bf8": 1, "mxfp8": 2, "mxfp4": 3, "int8": 4, "fp64": 5, "sparse24": 6,
                      "fp32": 7}
F4_TILE_MN = 256                    # M and N granule of gemm_f4_nt
F4_TILE_K = 256                     # K granule (elements) of gemm_f4_nt
I8_TILE_MN = 256                    # M and N granule of gemm_i8_nt
I8_TILE_K = 128                     # K granule of gemm_i8_nt
I8_MAX_K = 65536                    # its largest K: no int32 sum of K products can wrap
F64_TILE_M = 256                    # M granule of gemm_f64_nt
F64_TILE_N = 128                    # its N granule
F64_TILE_K = 16                     # its K granule (one 128-byte row of doubles)
F64_RING = 3                        # K-tiles in its LDS ring
READINESS_F64_SHAPE = (256, 256, 128)   # M, N, K of the fp64 readiness GEMM (csrc/probe_api.hip)
SP_TILE_M = 256                     # M granule of gemm_sp_bf16_nt
SP_TILE_N = 128                     # its N granule
SP_TILE_K = 128                     # its K granule, in dense K elements (64 compressed values, 16 metadata bytes)
SP_RING = 2                         # K-tiles in its LDS ring (held as four half-tile stages)
READINESS_SP_SHAPE = (256, 256, 512)    # M, N, dense K of the sparse24 readiness GEMM (csrc/probe_api.hip)
F32_TILE_M = 256                    # M granule of gemm_f32_nt
F32_TILE_N = 256                    # its N granule
F32_TILE_K = 32                     # its K granule (one 128-byte row of floats)
F32_RING = 2                        # K-tiles in its LDS ring
READINESS_F32_SHAPE = (256, 256, 128)   # M, N, K of the fp32 readiness GEMM (csrc/probe_api.hip)
_CHECK_TILE = 16                    # M and N granule of the dense checks
_CHECK_MAX_K = 1024                 # their largest K (one tile's operand rows sit in LDS)
_CHECK_F64_MAX_K = 256              # the fp64 check's: its rows are 8 * K bytes
_CHECK_F32_MAX_K = 512              # the fp32 check's: its rows are 4 * K bytes


def _operands(what: str, kind: str, a, bt, granule: int, k_granule: int, k_max=None, a_scale=None, bt_scale=None,
              out=None, c=None):
    """Validates the operands of a GEMM or check wrapper before native code sees their pointers; returns
    ``(a, bt, a_scale, bt_scale, res, m, n, k, fmt)`` with contiguous tensors. ``kind`` is ``bf16``, ``fp8``
    (``fmt`` = the two format codes of the native call, else ``()``), ``int8`` (the product is int32, not
    float32), ``fp64`` (float64 operands and product; ``granule`` may be an ``(M, N)`` pair), ``fp32`` (float32 operands and
    product) or ``fp4`` (packed: K is twice the row length; the operands come back as uint8). ``res`` is the product: ``c`` made contiguous when the caller
    has one to check, else ``out``, allocated when ``None``. Shape, granule, dtype and paired-scale errors
    are reported first; then every tensor must be on the operands' one GPU, and the product a float32
    ``(m, n)``, a caller's ``out`` contiguous as well (the kernel writes through its pointer)."""
    import torch

    fmt = ()
    if kind == "bf16":
        ok, expects = a.dtype == bt.dtype == torch.bfloat16, "bfloat16"
    elif kind == "fp8":
        codes = {torch.float8_e4m3fn: 0, torch.float8_e5m2: 1}
        ok, expects = a.dtype in codes and bt.dtype in codes, "float8_e4m3fn / float8_e5m2"
        if ok:
            fmt = (codes[a.dtype], codes[bt.dtype])
            if fmt == (1, 0):
                raise ProbeError(f"{what}: E5M2 x E4M3 is not built (swap the operands: E4M3 x E5M2 is)")
    elif kind == "int8":
        ok, expects = a.dtype == bt.dtype == torch.int8, "int8"
    elif kind == "fp64":
        ok, expects = a.dtype == bt.dtype == torch.float64, "float64"
    elif kind == "fp32":
        ok, expects = a.dtype == bt.dtype == torch.float32, "float32"
    else:
        packed = (torch.uint8, getattr(torch, "float4_e2m1fn_x2", torch.uint8))
        ok, expects = a.dtype in packed and bt.dtype in packed, "packed E2M1 (uint8 or float4_e2m1fn_x2)"
    if not ok:
        raise ProbeError(f"{what} expects {expects} operands, got {a.dtype} and {bt.dtype}")
    if a.dim() != 2 or bt.dim() != 2 or a.shape[1] != bt.shape[1]:
        raise ProbeError(f"{what} shape mismatch: {tuple(a.shape)} x {tuple(bt.shape)}^T"
                         f"{' (packed, K/2 bytes per row)' if kind == 'fp4' else ''}")
    m, n, k = a.shape[0], bt.shape[0], a.shape[1] * (2 if kind == "fp4" else 1)
    gm, gn = granule if isinstance(granule, tuple) else (granule, granule)
    if m % gm or n % gn or k % k_granule or m == 0 or n == 0 or k == 0 or (k_max and k > k_max):
        raise ProbeError(f"{what} needs M,N % {granule} == 0 and K % {k_granule} == 0"
                         f"{f' and K <= {k_max}' if k_max else ''}, got {m}x{n}x{k}")
    if (a_scale is None) != (bt_scale is None):
        raise ProbeError(f"{what}: block scales come in pairs (a_scale and bt_scale, or neither)")
    if a_scale is not None:
        for name, sc, rows in (("a_scale", a_scale, m), ("bt_scale", bt_scale, n)):
            if sc.dtype != torch.uint8 or tuple(sc.shape) != (rows, k // F8_BLOCK):
                raise ProbeError(f"{what}: {name} must be uint8 [{rows}, {k // F8_BLOCK}], got {sc.dtype} "
                                 f"{tuple(sc.shape)}")
        a_scale, bt_scale = a_scale.contiguous(), bt_scale.contiguous()
    # last, so that a wrong shape is reported as such: every tensor on one GPU (the kernel gets raw pointers)
    for name, t in (("a", a), ("bt", bt), ("a_scale", a_scale), ("bt_scale", bt_scale), ("out", out), ("c", c)):
        if t is not None and (t.device.type != "cuda" or t.device != a.device):
            raise ProbeError(f"{what}: {name} is on {t.device}; all operands must be on one GPU (a is on {a.device})")
    res_dtype = torch.int32 if kind == "int8" else torch.float64 if kind == "fp64" else torch.float32
    for name, t in (("out", out), ("c", c)):
        if t is not None and (t.dtype != res_dtype or tuple(t.shape) != (m, n) or
                              (t is out and not t.is_contiguous())):
            raise ProbeError(f"{what}: {name} must be a{' contiguous' if t is out else ''} "
                             f"{str(res_dtype).split('.')[-1]} {(m, n)}, got "
                             f"{t.dtype} {tuple(t.shape)} with strides {t.stride()}")
    if c is not None:
        res = c.contiguous()
    else:
        res = out if out is not None else torch.empty((m, n), dtype=res_dtype, device=a.device)
    a, bt = a.contiguous(), bt.contiguous()
    if kind == "fp4":
        a, bt = a.view(torch.uint8), bt.view(torch.uint8)
    return a, bt, a_scale, bt_scale, res, m, n, k, fmt


def _scale_ptrs(a_scale, bt_scale):
    """The two block-scale pointers of a native call (``None`` = null: an unscaled product)."""
    return (None, None) if a_scale is None else (a_scale.data_ptr(), bt_scale.data_ptr())


def _run_check(what: str, fn, device, *args):
    """Runs a dense-check entry point, ``fn(*args, out2, stream)``, on a zeroed result; returns ``(d2, w2)``."""
    import torch

    out = torch.zeros(4, dtype=torch.float32, device=device)
    _check(fn(*args, out.data_ptr(), _stream(device)), what)
    o = out.cpu()
    return float(o[0]), float(o[1])


GEMM_VARIANTS = {"auto": 0, "tile128": 1, "glds256": 2}


def gemm_bf16_nt(a, bt, out=None, variant: str = "auto"):
    """``a[M,K] @ bt[N,K]^T`` in fp32 on an MFMA kernel (M, N % 128 == 0, K % 64 == 0).

    ``auto`` runs the 256x256 LDS-DMA pipelined kernel when M, N % 256 == 0 and K % 128 == 0 and
    the 128x128 register-staged kernel otherwise; ``tile128`` / ``glds256`` force one."""
    if variant not in GEMM_VARIANTS:
        raise ProbeError(f"unknown GEMM variant {variant!r}: {sorted(GEMM_VARIANTS)}")
    a, bt, _, _, out, m, n, k, _ = _operands("gemm_bf16_nt", "bf16", a, bt, GEMM_TILE_M, GEMM_TILE_K, out=out)
    _check(lib().amdprobe_gemm_bf16_nt_variant(a.data_ptr(), bt.data_ptr(), out.data_ptr(), m, n, k,
                                               GEMM_VARIANTS[variant], _stream(a.device)), "gemm_bf16_nt")
    return out


def mfma_peak(device=0, blocks: int = 2048, iters: int = 2048):
    """Runs the MFMA issue-rate loop; returns (elapsed_s, flops)."""
    import torch

    out = torch.empty(blocks * 256, dtype=torch.float32, device=device)
    s = _stream(out.device)
    # warm-up launch
    _check(lib().amdprobe_mfma_peak(out.data_ptr(), blocks, 8, 1.0, s), "mfma_peak")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    _check(lib().amdprobe_mfma_peak(out.data_ptr(), blocks, iters, 1.0, s), "mfma_peak")
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / 1e3, lib().amdprobe_mfma_peak_flops(blocks, iters)


def hbm_copy(src, dst, blocks: int = 4096):
    nbytes = src.numel() * src.element_size()
    if dst.numel() * dst.element_size() < nbytes:
        raise ProbeError("hbm_copy destination too small")
    _check(lib().amdprobe_hbm_copy(src.data_ptr(), dst.data_ptr(), nbytes, blocks, _stream(src.device)), "hbm_copy")


def pattern_write(buf, seed: int, blocks: int = 2048):
    nbytes = buf.numel() * buf.element_size()
    _check(lib().amdprobe_pattern_write(buf.data_ptr(), nbytes, seed & 0xFFFFFFFF, blocks, _stream(buf.device)),
           "pattern_write")


def pattern_check(buf, seed: int, blocks: int = 2048) -> int:
    import torch

    nbytes = buf.numel() * buf.element_size()
    errs = torch.zeros(1, dtype=torch.int64, device=buf.device)
    _check(lib().amdprobe_pattern_check(buf.data_ptr(), nbytes, seed & 0xFFFFFFFF, errs.data_ptr(), blocks,
                                        _stream(buf.device)), "pattern_check")
    return int(errs.item())


def gemm_check(a, bt, c, inject: int = 0):
    """Dense check of ``c == a @ bt.T`` on the GPU (an fp32 VALU reference per element): returns
    ``(sum((c - a bt^T)^2), sum((a bt^T)^2))``. M, N % 16 == 0, K % 8 == 0, K <= 1024."""
    a, bt, _, _, c, m, n, k, _ = _operands("gemm_check", "bf16", a, bt, _CHECK_TILE, 8, _CHECK_MAX_K, c=c)
    return _run_check("gemm_check", lib().amdprobe_gemm_check, a.device, a.data_ptr(), bt.data_ptr(), c.data_ptr(),
                      m, n, k, inject)


def readiness_fill(ab, seed: int):
    """The readiness operand fill into ``ab`` (any dtype, byte size % 16)."""
    import torch

    res = torch.empty(8, dtype=torch.int32, device=ab.device)
    _check(lib().amdprobe_readiness_fill(ab.data_ptr(), ab.numel() * ab.element_size(), seed & 0xFFFFFFFF,
                                         res.data_ptr(), _stream(ab.device)), "readiness_fill")


READINESS_SHAPE = (256, 256, 512)   # M, N, K of the readiness GEMM (csrc/probe_api.hip)
READINESS_PATTERN_BYTES = 64 << 20


def readiness(device: int = 0, seed: int = 0, inject: int = 0):
    """The whole readiness check of one device in one native call (no framework ops): hashed bf16
    operands, the MFMA GEMM, a dense fp32 check of every product element and the 64 MiB HBM
    pattern test on a private stream, then one 32-byte read-back. Returns ``(gemm_rel_err, bad_words)``. ``inject`` = 1 or
    2 plants a product / memory fault, 3 / 4 skips the GEMM / pattern write (tests). Each call mixes
    a call counter into ``seed``, so stale buffers from an earlier call never verify. The GIL is released for the duration (ctypes)."""
    rel = ctypes.c_double(0.0)
    bad = ctypes.c_ulonglong(0)
    _check(lib().amdprobe_readiness(int(device), seed & 0xFFFFFFFF, int(inject), ctypes.byref(rel),
                                    ctypes.byref(bad)), "readiness")
    return rel.value, int(bad.value)


def gemm_f8_nt(a, bt, a_scale=None, bt_scale=None, out=None):
    """``a[M,K] @ bt[N,K]^T`` in fp32 on the FP8 MFMA kernel (``v_mfma_f32_16x16x128_f8f6f4``);
    M, N, K % 128 == 0. ``a`` / ``bt`` are ``float8_e4m3fn`` or ``float8_e5m2`` (E4M3 x E4M3,
    E5M2 x E5M2, E4M3 x E5M2). With ``a_scale[M, K/32]`` and ``bt_scale[N, K/32]`` (uint8 E8M0, value
    ``2^(s - 127)`` per 32 K elements) the product is MX block-scaled by the instruction's scale
    inputs (``v_mfma_scale_f32_16x16x128_f8f6f4``)."""
    a, bt, a_scale, bt_scale, out, m, n, k, fmt = _operands("gemm_f8_nt", "fp8", a, bt, F8_TILE, F8_TILE,
                                                            a_scale=a_scale, bt_scale=bt_scale, out=out)
    _check(lib().amdprobe_gemm_f8_nt(a.data_ptr(), bt.data_ptr(), out.data_ptr(), m, n, k, *fmt,
                                     *_scale_ptrs(a_scale, bt_scale), _stream(a.device)), "gemm_f8_nt")
    return out


def gemm_f8_check(a, bt, c, a_scale=None, bt_scale=None, inject: int = 0):
    """Dense check of an FP8 (or MX block-scaled) product ``c`` on the GPU, every element against an
    fp32 VALU reference that never touches the matrix pipe: returns ``(sum((c - ref)^2), sum(ref^2))``.
    M, N % 16 == 0, K % 32 == 0, K <= 1024."""
    a, bt, a_scale, bt_scale, c, m, n, k, fmt = _operands("gemm_f8_check", "fp8", a, bt, _CHECK_TILE, F8_BLOCK,
                                                          _CHECK_MAX_K, a_scale, bt_scale, c=c)
    return _run_check("gemm_f8_check", lib().amdprobe_gemm_f8_check, a.device, a.data_ptr(), bt.data_ptr(),
                      c.data_ptr(), m, n, k, *fmt, *_scale_ptrs(a_scale, bt_scale), inject)


def gemm_f4_nt(a, bt, a_scale=None, bt_scale=None, out=None):
    """``a[M,K] @ bt[N,K]^T`` in fp32 on the FP4 MFMA kernel (``v_mfma_[scale_]f32_16x16x128_f8f6f4`` with
    ``cbsz:4 blgp:4``); M, N % 256 == 0, K % 256 == 0. ``a`` / ``bt`` are packed OCP E2M1, ``[rows, K/2]``
    ``uint8`` or ``float4_e2m1fn_x2`` (element ``2j`` in bits 3:0 of byte ``j``). With ``a_scale[M, K/32]`` and
    ``bt_scale[N, K/32]`` (uint8 E8M0) the product is MXFP4, block-scaled by the instruction's scale inputs."""
    a, bt, a_scale, bt_scale, out, m, n, k, _ = _operands("gemm_f4_nt", "fp4", a, bt, F4_TILE_MN, F4_TILE_K,
                                                          a_scale=a_scale, bt_scale=bt_scale, out=out)
    _check(lib().amdprobe_gemm_f4_nt(a.data_ptr(), bt.data_ptr(), out.data_ptr(), m, n, k,
                                     *_scale_ptrs(a_scale, bt_scale), _stream(a.device)), "gemm_f4_nt")
    return out


def gemm_f4_check(a, bt, c, a_scale=None, bt_scale=None, inject: int = 0):
    """Dense check of an FP4 (or MXFP4) product ``c`` on the GPU, every element against an fp32 VALU
    reference decoded with integer arithmetic: returns ``(sum((c - ref)^2), sum(ref^2))``.
    M, N % 16 == 0, K % 32 == 0, K <= 1024."""
    a, bt, a_scale, bt_scale, c, m, n, k, _ = _operands("gemm_f4_check", "fp4", a, bt, _CHECK_TILE, F8_BLOCK,
                                                        _CHECK_MAX_K, a_scale, bt_scale, c=c)
    return _run_check("gemm_f4_check", lib().amdprobe_gemm_f4_check, a.device, a.data_ptr(), bt.data_ptr(),
                      c.data_ptr(), m, n, k, *_scale_ptrs(a_scale, bt_scale), inject)


def gemm_i8_nt(a, bt, out=None):
    """``a[M,K] @ bt[N,K]^T`` in int32 on the INT8 MFMA kernel (``v_mfma_i32_32x32x32_i8``); ``a`` / ``bt`` are
    ``int8``, M, N % 256 == 0, K % 128 == 0 and K <= 65536 (no sum of K products reaches 2^31). The result is
    exact: the instruction's int32 accumulate, nothing added in software."""
    a, bt, _, _, out, m, n, k, _ = _operands("gemm_i8_nt", "int8", a, bt, I8_TILE_MN, I8_TILE_K, I8_MAX_K, out=out)
    _check(lib().amdprobe_gemm_i8_nt(a.data_ptr(), bt.data_ptr(), out.data_ptr(), m, n, k, _stream(a.device)),
           "gemm_i8_nt")
    return out


def gemm_i8_check(a, bt, c, inject: int = 0):
    """Dense check of an INT8 product ``c`` (int32) on the GPU, every element against an int32 VALU reference
    (``v_dot4c_i32_i8``), the difference taken in integers: returns ``(sum((c - ref)^2), sum(ref^2))``, the
    first exactly 0.0 for a correct product. M, N % 16 == 0, K % 16 == 0, K <= 1024."""
    a, bt, _, _, c, m, n, k, _ = _operands("gemm_i8_check", "int8", a, bt, _CHECK_TILE, 16, _CHECK_MAX_K, c=c)
    return _run_check("gemm_i8_check", lib().amdprobe_gemm_i8_check, a.device, a.data_ptr(), bt.data_ptr(),
                      c.data_ptr(), m, n, k, inject)


def gemm_f64_nt(a, bt, out=None):
    """``a[M,K] @ bt[N,K]^T`` in fp64 on the FP64 MFMA kernel (``v_mfma_f64_16x16x4_f64``); ``a`` / ``bt`` are
    ``float64``, M % 256 == 0, N % 128 == 0, K % 16 == 0. Every product and sum is the instruction's; the
    result differs from a sequential sum only in summation order."""
    a, bt, _, _, out, m, n, k, _ = _operands("gemm_f64_nt", "fp64", a, bt, (F64_TILE_M, F64_TILE_N), F64_TILE_K,
                                             out=out)
    _check(lib().amdprobe_gemm_f64_nt(a.data_ptr(), bt.data_ptr(), out.data_ptr(), m, n, k, _stream(a.device)),
           "gemm_f64_nt")
    return out


def gemm_f64_check(a, bt, c, inject: int = 0):
    """Dense check of an FP64 product ``c`` (float64) on the GPU, every element against an fp64 VALU reference
    (``v_fma_f64``), the difference taken in fp64 before it is narrowed: returns ``(sum((c - ref)^2),
    sum(ref^2))`` as float32 sums. M, N % 16 == 0, K % 4 == 0, K <= 256."""
    a, bt, _, _, c, m, n, k, _ = _operands("gemm_f64_check", "fp64", a, bt, _CHECK_TILE, 4, _CHECK_F64_MAX_K, c=c)
    return _run_check("gemm_f64_check", lib().amdprobe_gemm_f64_check, a.device, a.data_ptr(), bt.data_ptr(),
                      c.data_ptr(), m, n, k, inject)


def gemm_f32_nt(a, bt, out=None):
    """``a[M,K] @ bt[N,K]^T`` in fp32 on the FP32 MFMA kernel (``v_mfma_f32_32x32x2_f32``); ``a`` / ``bt`` are
    ``float32``, M, N % 256 == 0, K % 32 == 0. Every product and sum is the instruction's; the result differs
    from a sequential sum only in summation order."""
    a, bt, _, _, out, m, n, k, _ = _operands("gemm_f32_nt", "fp32", a, bt, (F32_TILE_M, F32_TILE_N), F32_TILE_K,
                                             out=out)
    _check(lib().amdprobe_gemm_f32_nt(a.data_ptr(), bt.data_ptr(), out.data_ptr(), m, n, k, _stream(a.device)),
           "gemm_f32_nt")
    return out


def gemm_f32_check(a, bt, c, inject: int = 0):
    """Dense check of an FP32 product ``c`` (float32) on the GPU, every element against an fp32 VALU reference
    (``v_fma_f32``) that never touches the matrix pipe: returns ``(sum((c - ref)^2), sum(ref^2))``.
    M, N % 16 == 0, K % 8 == 0, K <= 512."""
    a, bt, _, _, c, m, n, k, _ = _operands("gemm_f32_check", "fp32", a, bt, _CHECK_TILE, 8, _CHECK_F32_MAX_K, c=c)
    return _run_check("gemm_f32_check", lib().amdprobe_gemm_f32_check, a.device, a.data_ptr(), bt.data_ptr(),
                      c.data_ptr(), m, n, k, inject)


def _sp_operands(what: str, a_vals, a_meta, others=()):
    """Validates a compressed 2:4 pair before native code sees a pointer; returns ``(a_vals, a_meta, m, k)``,
    contiguous, ``k`` the dense K. Dtypes and shapes first; then ``a_vals``, ``a_meta`` and every ``(name,
    tensor)`` of ``others`` must be on one GPU. Tensor contents are never read."""
    import torch

    if a_vals.dtype != torch.bfloat16 or a_meta.dtype != torch.uint8:
        raise ProbeError(f"{what} expects bfloat16 a_vals and uint8 a_meta, got {a_vals.dtype} and {a_meta.dtype}")
    if a_vals.dim() != 2 or a_vals.shape[0] == 0 or a_vals.shape[1] == 0 or a_vals.shape[1] % 4:
        raise ProbeError(f"{what}: a_vals must be [M, K/2] with K % 8 == 0, got {tuple(a_vals.shape)}")
    m, k = a_vals.shape[0], 2 * a_vals.shape[1]
    if tuple(a_meta.shape) != (m, k // 8):
        raise ProbeError(f"{what}: a_meta must be [M, K/8] = {(m, k // 8)} for a_vals {tuple(a_vals.shape)}, got "
                         f"{tuple(a_meta.shape)}")
    for name, t in (("a_vals", a_vals), ("a_meta", a_meta)) + tuple(others):
        if t is not None and (t.device.type != "cuda" or t.device != a_vals.device):
            raise ProbeError(f"{what}: {name} is on {t.device}; all operands must be on one GPU (a_vals is on "
                             f"{a_vals.device})")
    return a_vals.contiguous(), a_meta.contiguous(), m, k


def gemm_sp_bf16_nt(a_vals, a_meta, bt, out=None):
    """``A[M,K] @ bt[N,K]^T`` in fp32 on the 2:4 sparse MFMA kernel (``v_smfmac_f32_16x16x64_bf16``), A given
    compressed; M % 256 == 0, N % 128 == 0, K % 128 == 0. ``a_vals[M, K/2]`` (bfloat16): values ``2g`` and
    ``2g + 1`` of a row are the first and second kept element, in increasing K, of its group ``g`` of four
    consecutive K. ``a_meta[M, K/8]`` (uint8): byte ``j`` holds group ``2j`` in bits 3:0 and group ``2j + 1`` in
    bits 7:4; in a nibble bits 1:0 are the position (0..3) of the first kept element and bits 3:2 of the second,
    first < second (the legal nibbles are 4, 8, 12, 9, 13, 14; kept values may be zero). ``bt[N, K]`` is dense
    bfloat16. The wrappers do not read tensor contents, so nibble legality is not checked: an illegal nibble
    gives a wrong product, never an out-of-bounds access. ``sp24_compress`` makes the pair from a dense matrix."""
    import torch

    what = "gemm_sp_bf16_nt"
    if a_vals.dtype != torch.bfloat16 or bt.dtype != torch.bfloat16 or a_meta.dtype != torch.uint8:
        raise ProbeError(f"{what} expects bfloat16 a_vals and bt and a uint8 a_meta, got {a_vals.dtype}, {bt.dtype} "
                         f"and {a_meta.dtype}")
    if bt.dim() != 2 or a_vals.dim() != 2 or bt.shape[1] != 2 * a_vals.shape[1]:
        raise ProbeError(f"{what} shape mismatch: a_vals {tuple(a_vals.shape)} (K/2 per row) x bt {tuple(bt.shape)}^T")
    n = bt.shape[0]
    if a_vals.shape[0] % SP_TILE_M or n % SP_TILE_N or bt.shape[1] % SP_TILE_K or n == 0 or bt.shape[1] == 0:
        raise ProbeError(f"{what} needs M % {SP_TILE_M} == 0, N % {SP_TILE_N} == 0 and K % {SP_TILE_K} == 0, got "
                         f"{a_vals.shape[0]}x{n}x{bt.shape[1]}")
    if out is not None and (out.dtype != torch.float32 or tuple(out.shape) != (a_vals.shape[0], n)):
        raise ProbeError(f"{what}: out must be a contiguous float32 {(a_vals.shape[0], n)}, got {out.dtype} "
                         f"{tuple(out.shape)}")
    a_vals, a_meta, m, k = _sp_operands(what, a_vals, a_meta, (("bt", bt), ("out", out)))
    if out is None:
        out = torch.empty((m, n), dtype=torch.float32, device=a_vals.device)
    elif not out.is_contiguous():
        raise ProbeError(f"{what}: out must be contiguous, got strides {out.stride()}")
    _check(lib().amdprobe_gemm_sp_bf16_nt(a_vals.data_ptr(), a_meta.data_ptr(), bt.contiguous().data_ptr(),
                                          out.data_ptr(), m, n, k, _stream(a_vals.device)), what)
    return out


def sp24_expand(a_vals, a_meta):
    """The dense bfloat16 ``A[M, K]`` of a compressed pair (format: ``gemm_sp_bf16_nt``), on the GPU with VALU
    code only: every element that the metadata does not name is zero. Nibble legality is not checked."""
    import torch

    a_vals, a_meta, m, k = _sp_operands("sp24_expand", a_vals, a_meta)
    a = torch.empty((m, k), dtype=torch.bfloat16, device=a_vals.device)
    _check(lib().amdprobe_sp24_expand(a_vals.data_ptr(), a_meta.data_ptr(), a.data_ptr(), m, k,
                                      _stream(a_vals.device)), "sp24_expand")
    return a


def sp24_compress(a):
    """``(a_vals, a_meta)`` of a dense ``a[M, K]`` (K % 8 == 0) in the format of ``gemm_sp_bf16_nt``: of every
    group of four consecutive K the two elements of largest magnitude are kept, ties going to the lower
    position. Plain torch on ``a``'s device: plumbing for tests and tools, not a hot path."""
    import torch

    if a.dim() != 2 or a.shape[1] == 0 or a.shape[1] % 8:
        raise ProbeError(f"sp24_compress needs a [M, K] with K % 8 == 0, got {tuple(a.shape)}")
    m, k = a.shape
    g = a.reshape(m, k // 4, 4)
    # a stable descending sort of |a| keeps the lower position first among equals
    pos = g.abs().float().sort(dim=-1, descending=True, stable=True).indices[..., :2].sort(dim=-1).values
    vals = torch.gather(g, -1, pos).reshape(m, k // 2).to(torch.bfloat16)
    nib = (pos[..., 0] | (pos[..., 1] << 2)).reshape(m, k // 8, 2)
    return vals.contiguous(), (nib[..., 0] | (nib[..., 1] << 4)).to(torch.uint8).contiguous()


def f8_fill(buf, seed: int, kind: str = "e4m3"):
    """The FP8 / FP4 readiness operand fill into ``buf`` (byte size % 16): finite hashed ``e4m3`` / ``e5m2``
    bytes with |x| in [0.5, 1), E8M0 block ``scale`` bytes in [124, 131], ``e2m1`` / ``i8``: any byte (two
    finite FP4 codes, or one int8, -128 included), ``f64``: finite doubles with a hashed sign, |x| in
    [0.5, 1) and all 52 mantissa bits hashed, ``meta24``: 2:4 metadata, every nibble one of the six legal
    codes 4, 8, 12, 9, 13, 14, or ``f32``: finite floats with a hashed sign, |x| in [0.5, 1) and all 23 mantissa
    bits hashed."""
    if kind not in F8_FILL_KINDS:
        raise ProbeError(f"unknown f8 fill {kind!r}: {sorted(F8_FILL_KINDS)}")
    _check(lib().amdprobe_f8_fill(buf.data_ptr(), buf.numel() * buf.element_size(), seed & 0xFFFFFFFF,
                                  F8_FILL_KINDS[kind], None, _stream(buf.device)), "f8_fill")


def readiness_f8(device: int = 0, seed: int = 0, mode: str = "fp8", inject: int = 0) -> float:
    """The FP8 matrix path of one device in one native call: hashed operands, the f8 MFMA GEMM (``fp8`` =
    E4M3, ``bf8`` = E5M2, ``mxfp8`` = E4M3 with E8M0 block scales through the MFMA scale inputs; ``mxfp4`` = packed E2M1 with
    block scales on the f4 GEMM; ``int8`` = any-byte int8 operands on the i8 GEMM, whose check is exact: a healthy
    device returns 0.0;
    ``fp64`` = hashed doubles on the f64 GEMM at 256 x 256 x 128, checked in fp64: judge it by
    ``gpu_health.MAX_GEMM_F64_REL_ERR``; ``sparse24`` = hashed compressed bf16 values, hashed legal 2:4 metadata
    and a dense hashed bt on the sparse GEMM at ``READINESS_SP_SHAPE``, checked by the dense bf16 check against
    the VALU expansion of the compressed A; ``fp32`` = hashed floats on the f32 GEMM at ``READINESS_F32_SHAPE``,
    checked against an fp32 VALU reference: judge it by ``gpu_health.MAX_GEMM_F32_REL_ERR``), the dense
    VALU check of every element, one read-back on a private stream. Returns ``gemm_rel_err``. ``inject`` = 1
    loses a product tile, 3 skips the GEMM (tests). The GIL is released for the duration (ctypes)."""
    if mode not in READINESS_F8_MODES:
        raise ProbeError(f"unknown f8 readiness mode {mode!r}: {sorted(READINESS_F8_MODES)}")
    rel = ctypes.c_double(0.0)
    _check(lib().amdprobe_readiness_f8(int(device), seed & 0xFFFFFFFF, READINESS_F8_MODES[mode], int(inject),
                                       ctypes.byref(rel)), "readiness_f8")
    return rel.value


def require_native_on_gpu() -> None:
    """Raise if a GPU is present but the HIP extension is not loadable (no silent fallback)."""
    import torch

    if torch.cuda.is_available():
        lib()
