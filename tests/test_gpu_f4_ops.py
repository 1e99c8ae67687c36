"""FP4 / MXFP4 MFMA probe kernels vs fp64 references of the decoded operands (MI355X only, except the
contract test). Operands are built on the CPU from nibble codes: nothing depends on device-side casts."""
import functools

import pytest

torch = pytest.importorskip("torch")

from dcos_commons_amd import ops  # noqa: E402
from dcos_commons_amd.ops import gpu_health  # noqa: E402

E2M1 = torch.tensor([0, .5, 1, 1.5, 2, 3, 4, 6, -0., -.5, -1, -1.5, -2, -3, -4, -6], dtype=torch.float64)
T, TK = ops.F4_TILE_MN, ops.F4_TILE_K
# Relative Frobenius bound of the random-operand and readiness tests: 4x the worst value measured on
# MI355X over the four test_random_operands cases: unscaled 0 and 0 (sums of E2M1 products are exact
# in fp32), MXFP4 6.751e-8 (512x768x1024) and 1.321e-7 (1024x256x4096). See profiles/gemm_f4.md.
F4_REL_BOUND = 4 * 1.321e-7


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.lib()  # must load: a GPU box without the extension is a failure, not a skip
    return torch.device("cuda", 0)


def decode(codes, scale=None):
    x = E2M1[codes.long()]
    return x if scale is None else x * torch.pow(2.0, scale.double() - 127).repeat_interleave(32, dim=1)


@functools.lru_cache(maxsize=None)
def case(kind, m, n, k, mx):
    """(packed a, packed bt, a_scale, bt_scale, fp64 reference) on the CPU; ``kind`` is 'int' (codes and
    scales from the index formulas: every fp32 partial sum exact, asserted) or 'rand'."""
    rows = lambda r: torch.arange(r).view(r, 1)
    kk, kb = torch.arange(k).view(1, k), torch.arange(k // 32).view(1, k // 32)
    sa = sb = None
    if kind == "int":
        a, bt = (5 * rows(m) + kk + kk // 7) % 16, (3 * rows(n) + 5 * kk + kk // 11) % 16
        if mx:
            sa = (127 + (rows(m) + 2 * kb) % 4 - 1).to(torch.uint8)
            sb = (127 + (3 * rows(n) + kb) % 4 - 2).to(torch.uint8)
    else:
        g = torch.Generator().manual_seed(m * 31 + n * 7 + k)
        a, bt = torch.randint(0, 16, (m, k), generator=g), torch.randint(0, 16, (n, k), generator=g)
        if mx:
            sa = torch.randint(120, 135, (m, k // 32), generator=g, dtype=torch.uint8)
            sb = torch.randint(120, 135, (n, k // 32), generator=g, dtype=torch.uint8)
    ref = decode(a, sa) @ decode(bt, sb).t()
    cpu32 = (decode(a, sa).float() @ decode(bt, sb).float().t()).double()
    if kind == "int":
        assert torch.equal(cpu32, ref)  # exact in fp32: what makes torch.equal against the kernel fair
    else:
        assert torch.linalg.norm(cpu32 - ref) / torch.linalg.norm(ref) < 1e-5
    pack = lambda c: (c[:, 0::2] | c[:, 1::2] << 4).to(torch.uint8)
    return pack(a), pack(bt), sa, sb, ref


def on(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def rel_err(c, ref):
    return (torch.linalg.norm(c.double().cpu() - ref) / torch.linalg.norm(ref)).item()


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(T, T, TK), (T, 2 * T, 2 * TK), (3 * T, T, 3 * TK), (T, T, 5 * TK), (9 * T, T, TK)])
def test_exact_layout(dev, m, n, k):
    """K-tiles 1, 2, 3, 5 around the 2-stage ring; 9 row tiles: short last band of grouped_tile."""
    a, bt, _, _, ref = case("int", m, n, k, False)
    assert torch.equal(ops.gemm_f4_nt(*on(dev, a, bt)).cpu().double(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(T, T, TK), (2 * T, T, 3 * TK), (T, 3 * T, 5 * TK)])
def test_mx_exact(dev, m, n, k):
    """Distinct power-of-two scales per row and K-block: a wrong nibble order, lane-to-block mapping, or a
    scale from the wrong row, block or byte lane shows."""
    a, bt, sa, sb, ref = case("int", m, n, k, True)
    assert torch.equal(ops.gemm_f4_nt(*on(dev, a, bt, sa, sb)).cpu().double(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("mx", [False, True], ids=["f4", "mxfp4"])
@pytest.mark.parametrize("m,n,k", [(2 * T, 3 * T, 4 * TK), (4 * T, T, 16 * TK)])
def test_random_operands(dev, m, n, k, mx):
    a, bt, sa, sb, ref = case("rand", m, n, k, mx)
    rel = rel_err(ops.gemm_f4_nt(*on(dev, a, bt, sa, sb)), ref)
    print(f"f4 rel_err {m}x{n}x{k} mx={mx}: {rel:.3e}")
    assert rel < F4_REL_BOUND, rel


@pytest.mark.gpu
@pytest.mark.parametrize("mx", [False, True], ids=["plain", "mx"])
@pytest.mark.parametrize("m,n,k", [(16, 48, 128), (256, 256, 512)])
def test_check_kernel(dev, m, n, k, mx):
    a, bt, sa, sb, ref = case("rand", m, n, k, mx)
    da, dbt, dsa, dsb, c = on(dev, a, bt, sa, sb, ref.float())
    d2, w2 = ops.gemm_f4_check(da, dbt, c, dsa, dsb)
    assert (d2 / w2) ** 0.5 < 1e-5
    assert w2 == pytest.approx(float((ref ** 2).sum()), rel=1e-4)
    lost = c.clone()
    lost[0:16, 16:32] = 0
    d2, _ = ops.gemm_f4_check(da, dbt, lost, dsa, dsb)
    assert d2 == pytest.approx(float((ref[0:16, 16:32] ** 2).sum()), rel=1e-3)
    d2, _ = ops.gemm_f4_check(da, dbt, c, dsa, dsb, inject=1)
    assert d2 == pytest.approx(float((ref[0:16, 0:16] ** 2).sum()), rel=1e-3)


@pytest.mark.gpu
def test_readiness_mxfp4(dev):
    before = torch.cuda.current_device()
    assert ops.readiness_f8(0, 77, "mxfp4") < F4_REL_BOUND
    assert ops.readiness_f8(0, 77, "mxfp4") < F4_REL_BOUND
    assert ops.readiness_f8(0, 77, "mxfp4", inject=1) > gpu_health.MAX_GEMM_REL_ERR
    assert ops.readiness_f8(0, 77, "mxfp4", inject=3) > gpu_health.MAX_GEMM_REL_ERR
    assert ops.readiness_f8(0, 77, "mxfp4") < F4_REL_BOUND
    assert torch.cuda.current_device() == before
    rep = gpu_health.readiness_probe(0, matrix=("bf16", "mxfp4"))
    assert rep["healthy"] and rep["gemm_mxfp4_rel_err"] < gpu_health.MAX_GEMM_REL_ERR, rep


@pytest.mark.parametrize("what", ["m128", "k384", "k_mismatch", "e4m3", "one_scale", "scale_shape", "cpu"])
def test_contract(what):
    """Rejected in Python before the native library is touched: runs without a GPU."""
    z = lambda m, k, dt=torch.uint8: torch.zeros((m, k // 2)).to(dt)
    s = lambda m, kb: torch.full((m, kb), 127, dtype=torch.uint8)
    args = {"m128": (z(128, 256), z(256, 256)), "k384": (z(256, 384), z(256, 384)),
            "k_mismatch": (z(256, 256), z(256, 512)), "e4m3": (z(256, 256, torch.float8_e4m3fn), z(256, 256)),
            "one_scale": (z(256, 256), z(256, 256), s(256, 8), None),
            "scale_shape": (z(256, 256), z(256, 256), s(256, 8), s(8, 256)),
            "cpu": (z(256, 256), z(256, 256))}[what]  # valid shapes, but not on a GPU
    with pytest.raises(ops.ProbeError):
        ops.gemm_f4_nt(*args)
    assert gpu_health._f8_modes(("bf16", "mxfp4")) == ["mxfp4"]
