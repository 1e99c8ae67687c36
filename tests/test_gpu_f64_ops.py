"""FP64 MFMA probe kernels vs CPU float64 matmuls (MI355X only, except the contract test). The exact cases use
integer-valued doubles, for which every summation order gives the same bits; the random case is held to the
forward error bound of two fp64 sums of K terms."""
import functools

import pytest

torch = pytest.importorskip("torch")

from dcos_commons_amd import ops  # noqa: E402
from dcos_commons_amd.ops import gpu_health  # noqa: E402

TM, TN, TK, R = ops.F64_TILE_M, ops.F64_TILE_N, ops.F64_TILE_K, ops.F64_RING


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.lib()  # must load: a GPU box without the extension is a failure, not a skip
    return torch.device("cuda", 0)


@functools.lru_cache(maxsize=None)
def case(kind, m, n, k):
    """(a, bt, float64 reference a @ bt.t()) on the CPU. 'index': integer formulas of (row, k), distinct per row
    and K position, of both signs, |a| and |b| in (2^20 - 1024, 2^20]. The K products of an element share the sign
    (-1)^(row + col), so |ref| >= 2^40; every partial sum in any order is an integer below 2^52 for K <= 1024, so
    the product is exact whatever the summation order. 'rand': randn."""
    rows, kk = (lambda r: torch.arange(r).view(r, 1)), torch.arange(k).view(1, k)
    if kind == "index":
        a = (1 - 2 * ((rows(m) + kk) % 2)) * (2 ** 20 - (5 * rows(m) + kk + kk // 7) % 1021)
        bt = (1 - 2 * ((rows(n) + kk) % 2)) * (2 ** 20 - (3 * rows(n) + 5 * kk + kk // 11) % 1019)
        assert a.min() < 0 < a.max() == 2 ** 20 and bt.min() < 0 < bt.max() == 2 ** 20
        a, bt = a.double(), bt.double()
    else:
        g = torch.Generator().manual_seed(m * 31 + n * 7 + k)
        a, bt = (torch.randn((r, k), generator=g, dtype=torch.float64) for r in (m, n))
    return a, bt, a @ bt.t()


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(TM, TN, TK), (TM, 2 * TN, 2 * TK), (2 * TM, TN, 3 * TK), (TM, TN, (R + 2) * TK),
                                   (9 * TM, TN, TK)])
def test_exact(dev, m, n, k):
    """K-tiles 1, 2, 3, R + 2 around the ring; 9 row tiles: the short last band of grouped_tile. Bit-equal, with
    sums of 2^40 and above: a wrong lane, register or K pairing shows, and no stage passed through fp32."""
    a, bt, ref = case("index", m, n, k)
    assert float(ref.abs().max()) >= 2 ** 40
    out = ops.gemm_f64_nt(a.to(dev), bt.to(dev))
    assert out.dtype == torch.float64 and out.is_contiguous()
    assert torch.equal(out.cpu(), ref)


@pytest.mark.gpu
def test_random(dev):
    """Each of the two sums is within K * 2^-53 * sum|a||b| of exact, so they differ by at most K * 2^-52 * that."""
    m, n, k = 2 * TM, 3 * TN, 4 * TK
    a, bt, ref = case("rand", m, n, k)
    out = ops.gemm_f64_nt(a.to(dev), bt.to(dev)).cpu()
    assert bool(((out - ref).abs() <= k * 2.0 ** -52 * (a.abs() @ bt.abs().t())).all())


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(16, 48, 4 * TK), ops.READINESS_F64_SHAPE])
def test_check_kernel(dev, m, n, k):
    a, bt, ref = case("index", m, n, k)
    da, dbt, c = a.to(dev), bt.to(dev), ref.to(dev)
    sq = lambda x: float((x ** 2).sum())
    d2, w2 = ops.gemm_f64_check(da, dbt, c)
    assert d2 == 0.0
    assert w2 == pytest.approx(sq(ref), rel=1e-4)
    off = c.clone()
    assert abs(float(off[3, 21])) >= 2 ** 40
    off[3, 21] += 1.0                                  # 2^-40 of its value: only an fp64 subtraction sees it
    d2, _ = ops.gemm_f64_check(da, dbt, off)
    assert d2 == 1.0
    lost = c.clone()
    lost[0:16, 16:32] = 0
    d2, _ = ops.gemm_f64_check(da, dbt, lost)
    assert d2 == pytest.approx(sq(ref[0:16, 16:32]), rel=1e-3)
    d2, _ = ops.gemm_f64_check(da, dbt, c, inject=1)
    assert d2 == pytest.approx(sq(ref[0:16, 0:16]), rel=1e-3)
    with pytest.raises(ops.ProbeError, match="float64"):
        ops.gemm_f64_check(da, dbt, c.float())


@pytest.mark.gpu
def test_readiness_fp64(dev):
    before = torch.cuda.current_device()
    assert ops.readiness_f8(0, 77, "fp64") < gpu_health.MAX_GEMM_F64_REL_ERR
    assert ops.readiness_f8(0, 77, "fp64") < gpu_health.MAX_GEMM_F64_REL_ERR
    assert ops.readiness_f8(0, 77, "fp64", inject=1) > gpu_health.MAX_GEMM_REL_ERR
    assert ops.readiness_f8(0, 77, "fp64", inject=3) > gpu_health.MAX_GEMM_REL_ERR
    assert torch.cuda.current_device() == before
    rep = gpu_health.readiness_probe(0, matrix=("bf16", "fp64"))
    assert rep["healthy"] and rep["gemm_fp64_rel_err"] < gpu_health.MAX_GEMM_F64_REL_ERR, rep


@pytest.mark.parametrize("what", ["m128", "k24", "k_mismatch", "f32", "f32_out", "cpu"])
def test_contract(what):
    """Rejected in Python before the native library is touched: runs without a GPU."""
    z = lambda m, k, dt=torch.float64: torch.zeros((m, k), dtype=dt)
    args, kw = {"m128": (z(128, 16), z(128, 16)), "k24": (z(256, 24), z(128, 24)),
                "k_mismatch": (z(256, 16), z(128, 32)), "f32": (z(256, 16, torch.float32), z(128, 16, torch.float32)),
                "f32_out": (z(256, 16), z(128, 16)), "cpu": (z(256, 16), z(128, 16))}[what], {}  # cpu: valid, no GPU
    if what == "f32_out":
        kw["out"] = torch.zeros((256, 128), dtype=torch.float32)
    with pytest.raises(ops.ProbeError):
        ops.gemm_f64_nt(*args, **kw)
    assert gpu_health._f8_modes(("bf16", "fp64")) == ["fp64"]
