"""INT8 MFMA probe kernels vs CPU int64 matmuls (MI355X only, except the contract test). Every check is
exact: the int32 accumulate has no rounding, so there is no tolerance to tune."""
import functools

import pytest

torch = pytest.importorskip("torch")

from dcos_commons_amd import ops  # noqa: E402
from dcos_commons_amd.ops import gpu_health  # noqa: E402

T, TK = ops.I8_TILE_MN, ops.I8_TILE_K


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.lib()  # must load: a GPU box without the extension is a failure, not a skip
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def case(kind, m, n, k):
    """(a, bt, int64 reference) on the CPU. 'index': row / column formulas that reach -128 and 127, distinct
    per row and K position; 'rand': uniform int8; 'big': -128 everywhere but one row of alternating 127 / -128
    in each operand (sums reach 2^25: not representable through fp32 rounding of partial sums)."""
    rows, kk = (lambda r: torch.arange(r).view(r, 1)), torch.arange(k).view(1, k)
    if kind == "index":
        a, bt = (5 * rows(m) + kk + kk // 7) % 256 - 128, (3 * rows(n) + 5 * kk + kk // 11) % 256 - 128
        assert a.min() == bt.min() == -128 and a.max() == bt.max() == 127
    elif kind == "rand":
        g = torch.Generator().manual_seed(m * 31 + n * 7 + k)
        a, bt = torch.randint(-128, 128, (m, k), generator=g), torch.randint(-128, 128, (n, k), generator=g)
    else:
        a, bt = torch.full((m, k), -128), torch.full((n, k), -128)
        a[37] = bt[101] = torch.where(kk[0] % 2 == 0, 127, -128)
    return a.to(torch.int8), bt.to(torch.int8), a @ bt.t()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,m,n,k", [
    ("index", T, T, TK), ("index", T, 2 * T, 2 * TK), ("index", 2 * T, T, 3 * TK), ("index", T, T, 5 * TK),
    ("index", 9 * T, T, TK), ("rand", 2 * T, 3 * T, 4 * TK), ("big", T, T, 2048)])
def test_exact(dev, kind, m, n, k):
    """K-tiles 1, 2, 3, 5 around the 2-stage ring; 9 row tiles: short last band of grouped_tile; 'big': the
    accumulate is an integer one and the epilogue never passes through fp32."""
    a, bt, ref = case(kind, m, n, k)
    if kind == "big":
        assert int(ref.abs().max()) >= 2 ** 25
    out = ops.gemm_i8_nt(a.to(dev), bt.to(dev))
    assert out.dtype == torch.int32
    assert torch.equal(out.cpu().long(), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(16, 48, 128), (256, 256, 512)])
def test_check_kernel(dev, m, n, k):
    a, bt, ref = case("rand", m, n, k)
    da, dbt, c = a.to(dev), bt.to(dev), ref.to(torch.int32).to(dev)
    sq = lambda x: float((x.double() ** 2).sum())
    d2, w2 = ops.gemm_i8_check(da, dbt, c)
    assert d2 == 0.0
    assert w2 == pytest.approx(sq(ref), rel=1e-4)
    lost = c.clone()
    lost[0:16, 16:32] = 0
    d2, _ = ops.gemm_i8_check(da, dbt, lost)
    assert d2 == pytest.approx(sq(ref[0:16, 16:32]), rel=1e-3)
    d2, _ = ops.gemm_i8_check(da, dbt, c, inject=1)
    assert d2 == pytest.approx(sq(ref[0:16, 0:16]), rel=1e-3)
    with pytest.raises(ops.ProbeError, match="int32"):
        ops.gemm_i8_check(da, dbt, c.float())


@pytest.mark.gpu
def test_readiness_int8(dev):
    before = torch.cuda.current_device()
    assert ops.readiness_f8(0, 77, "int8") == 0.0
    assert ops.readiness_f8(0, 77, "int8") == 0.0
    assert ops.readiness_f8(0, 77, "int8", inject=1) > gpu_health.MAX_GEMM_REL_ERR
    assert ops.readiness_f8(0, 77, "int8", inject=3) > gpu_health.MAX_GEMM_REL_ERR
    assert torch.cuda.current_device() == before
    rep = gpu_health.readiness_probe(0, matrix=("bf16", "int8"))
    assert rep["healthy"] and rep["gemm_int8_rel_err"] == 0.0, rep


@pytest.mark.parametrize("what", ["m128", "k192", "k_mismatch", "uint8", "e4m3", "f32_out", "k_big", "cpu"])
def test_contract(what):
    """Rejected in Python before the native library is touched: runs without a GPU."""
    z = lambda m, k, dt=torch.int8: torch.zeros((m, k)).to(dt)
    args, kw = {"m128": (z(128, 128), z(256, 128)), "k192": (z(256, 192), z(256, 192)),
                "k_mismatch": (z(256, 128), z(256, 256)), "uint8": (z(256, 128, torch.uint8), z(256, 128)),
                "e4m3": (z(256, 128, torch.float8_e4m3fn), z(256, 128, torch.float8_e4m3fn)),
                "f32_out": (z(256, 128), z(256, 128)), "k_big": (z(256, 65536 + 128), z(256, 65536 + 128)),
                "cpu": (z(256, 128), z(256, 128))}[what], {}  # cpu: valid shapes, but not on a GPU
    if what == "f32_out":
        kw["out"] = torch.zeros((256, 256), dtype=torch.float32)
    with pytest.raises(ops.ProbeError):
        ops.gemm_i8_nt(*args, **kw)
    assert gpu_health._f8_modes(("bf16", "int8")) == ["int8"]
