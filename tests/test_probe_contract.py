"""What the bf16 and FP8 op wrappers reject in Python, before a pointer reaches native code (the FP4 twin is
tests/test_gpu_f4_ops.py::test_contract). The first test needs no GPU and must not load the library."""
import pytest

torch = pytest.importorskip("torch")

from dcos_commons_amd import ops  # noqa: E402

M, N, K = 128, 256, 128
E4 = torch.float8_e4m3fn


def calls(dev, other):
    """(id, thunk) per rejected call: every wrapper with operands of valid shape on ``dev``, and one of
    ``out`` / ``c`` / ``a_scale`` wrong. ``other`` is a device that is not ``dev``."""
    z = lambda rows, dt, d=dev: torch.zeros((rows, K), device=d).to(dt)
    a16, b16, a8, b8 = z(M, torch.bfloat16), z(N, torch.bfloat16), z(M, E4), z(N, E4)
    sa, sb = (torch.full((rows, K // 32), 127, dtype=torch.uint8, device=dev) for rows in (M, N))
    gemms = (("gemm_bf16_nt", lambda out: ops.gemm_bf16_nt(a16, b16, out)),
             ("gemm_f8_nt", lambda out: ops.gemm_f8_nt(a8, b8, out=out)))
    checks = (("gemm_check", lambda c: ops.gemm_check(a16, b16, c)),
              ("gemm_f8_check", lambda c: ops.gemm_f8_check(a8, b8, c)))
    good = lambda d=dev: torch.zeros((M, N), device=d)
    bad = {"dtype": lambda: good().double(), "shape": lambda: torch.zeros((M, N + 16), device=dev),
           "transposed": lambda: torch.zeros((N, M), device=dev).t(), "device": lambda: good(other)}
    for name, fn in gemms + checks:
        for what, make in bad.items():
            if what == "transposed" and (name, fn) in checks:
                continue            # a check only reads c: it takes a contiguous copy
            yield f"{name}-{what}", (lambda fn=fn, make=make: fn(make()))
    yield "gemm_f8_nt-scale_device", lambda: ops.gemm_f8_nt(a8, b8, sa.to(other), sb)
    yield "gemm_f8_check-scale_device", lambda: ops.gemm_f8_check(a8, b8, good(), sa.to(other), sb)


def test_cpu_operands_are_rejected_before_the_library_loads():
    loaded = ops._lib is not None
    z = lambda rows, dt: torch.zeros((rows, K)).to(dt)
    out = torch.zeros((M, N))
    for thunk in (lambda: ops.gemm_bf16_nt(z(M, torch.bfloat16), z(N, torch.bfloat16)),
                  lambda: ops.gemm_check(z(M, torch.bfloat16), z(N, torch.bfloat16), out),
                  lambda: ops.gemm_f8_nt(z(M, E4), z(N, E4)),
                  lambda: ops.gemm_f8_check(z(M, E4), z(N, E4), out)):
        with pytest.raises(ops.ProbeError, match="is on cpu"):
            thunk()
    for name, thunk in calls(torch.device("cpu"), torch.device("meta")):
        with pytest.raises(ops.ProbeError, match=name.split("-")[0]):
            thunk()
    assert loaded or ops._lib is None


@pytest.mark.gpu
def test_gpu_operands_with_a_bad_product_or_scale_are_rejected():
    """The calls the bf16 and FP8 wrappers used to pass on: a write through the pointer of an ``out`` that
    is elsewhere, of another dtype or shape, or transposed; scales on another device than ``a``."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    dev = torch.device("cuda", 0)
    for name, thunk in calls(dev, torch.device("cpu")):
        with pytest.raises(ops.ProbeError, match=name.split("-")[0]):
            thunk()
    # and the same operands pass with a good product
    c = ops.gemm_bf16_nt(torch.zeros((M, K), device=dev).bfloat16(), torch.zeros((N, K), device=dev).bfloat16(),
                         torch.ones((M, N), device=dev))
    assert not c.any()
