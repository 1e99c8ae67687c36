"""FP32 MFMA probe kernels vs CPU float64 matmuls (MI355X only, except the contract test). The exact cases use
integer-valued floats whose partial sums stay below 2^24 in any order, so every summation order gives the same
bits; the random case is held to two roundings per term against the exact product."""
import functools

import pytest

torch = pytest.importorskip("torch")

from dcos_commons_amd import ops  # noqa: E402
from dcos_commons_amd.ops import gpu_health  # noqa: E402

TM, TN, TK, R = ops.F32_TILE_M, ops.F32_TILE_N, ops.F32_TILE_K, ops.F32_RING


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.lib()  # must load: a GPU box without the extension is a failure, not a skip
    return torch.device("cuda", 0)


def round_sig(x, bits):
    """x (float64) rounded to `bits` significant bits, half to even: what a narrower operand path would feed."""
    m, e = torch.frexp(x)
    return torch.ldexp(torch.round(m * 2.0 ** bits), e - bits)


@functools.lru_cache(maxsize=None)
def case(kind, m, n, k):
    """(a, bt, float64 reference a @ bt.t()) on the CPU, a and bt float32. 'index': integer formulas of (row, k),
    distinct per row and K position, of both signs. At even k |a| is odd in (2^11, 2^12), so it needs 12 significant
    bits, and |b| is 2..4; at odd k the roles are swapped. The K products of an element share the sign
    (-1)^(row + col), so at K = 128 |ref| reaches 2^20. 'rand': randn."""
    rows, kk = (lambda r: torch.arange(r).view(r, 1)), torch.arange(k).view(1, k)
    if kind == "index":
        big = lambda r, p, q: 2049 + 2 * ((p * rows(r) + q * kk + kk // 7) % 1021)
        small = lambda r, p: 2 + (p * rows(r) + kk + kk // 5) % 3
        even = kk % 2 == 0
        a = (1 - 2 * ((rows(m) + kk) % 2)) * torch.where(even, big(m, 5, 3), small(m, 2))
        bt = (1 - 2 * ((rows(n) + kk) % 2)) * torch.where(even, small(n, 1), big(n, 7, 11))
        a, bt = a.double(), bt.double()
        assert a.min() < 0 < a.max() and bt.min() < 0 < bt.max()
        # every partial sum, in any order, is an integer below 2^24: exact in fp32
        assert float((a.abs() @ bt.abs().t()).max()) < 2 ** 24
        # a path narrower than fp32 changes the product: 11-bit operands move nearly every element
        assert float(((round_sig(a, 11) @ round_sig(bt, 11).t()) != a @ bt.t()).double().mean()) > 0.9
    else:
        g = torch.Generator().manual_seed(m * 31 + n * 7 + k)
        a, bt = (torch.randn((r, k), generator=g, dtype=torch.float32).double() for r in (m, n))
    return a.float(), bt.float(), a @ bt.t()


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(TM, TN, TK), (TM, 2 * TN, 2 * TK), (2 * TM, TN, 3 * TK), (TM, TN, (R + 2) * TK),
                                   (9 * TM, TN, TK)])
def test_exact(dev, m, n, k):
    """K-tiles 1, 2, 3, R + 2 around the ring; 9 row tiles: the short last band of grouped_tile. Bit-equal: a wrong
    lane, register or K pairing shows, and so does an operand path narrower than fp32."""
    a, bt, ref = case("index", m, n, k)
    out = ops.gemm_f32_nt(a.to(dev), bt.to(dev))
    assert out.dtype == torch.float32 and out.is_contiguous()
    assert torch.equal(out.cpu().double(), ref)


@pytest.mark.gpu
def test_random(dev):
    """Two roundings per term (an unfused multiply, then the add) against the exact product."""
    m, n, k = 2 * TM, 3 * TN, 4 * TK
    a, bt, ref = case("rand", m, n, k)
    out = ops.gemm_f32_nt(a.to(dev), bt.to(dev)).cpu().double()
    assert bool(((out - ref).abs() <= k * 2.0 ** -23 * (a.double().abs() @ bt.double().abs().t())).all())


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(16, 48, 4 * TK), ops.READINESS_F32_SHAPE])
def test_check_kernel(dev, m, n, k):
    a, bt, ref = case("index", m, n, k)
    da, dbt, c = a.to(dev), bt.to(dev), ref.float().to(dev)
    sq = lambda x: float((x ** 2).sum())
    d2, w2 = ops.gemm_f32_check(da, dbt, c)
    assert d2 == 0.0
    assert w2 == pytest.approx(sq(ref), rel=1e-4)
    off = c.clone()
    r, col = (int(x) for x in (ref.abs() >= 2 ** 20).nonzero()[0])
    off[r, col] += 1.0                                 # 2^-20 of its value or less
    d2, _ = ops.gemm_f32_check(da, dbt, off)
    assert d2 == 1.0
    lost = c.clone()
    lost[0:16, 16:32] = 0
    d2, _ = ops.gemm_f32_check(da, dbt, lost)
    assert d2 == pytest.approx(sq(ref[0:16, 16:32]), rel=1e-3)
    d2, _ = ops.gemm_f32_check(da, dbt, c, inject=1)
    assert d2 == pytest.approx(sq(ref[0:16, 0:16]), rel=1e-3)
    with pytest.raises(ops.ProbeError, match="float32"):
        ops.gemm_f32_check(da, dbt, c.double())
    # the hashed fill, and on it a product whose operands went through an 11-bit path: above the fp32 bound,
    # below the shared one (why the mode has a bound of its own)
    ab = torch.empty((m + n, k), dtype=torch.float32, device=dev)
    ops.f8_fill(ab, seed=5, kind="f32")
    h = ab.cpu()
    assert bool(torch.isfinite(h).all()) and h.min() < 0 < h.max()
    assert 0.5 <= float(h.abs().min()) and float(h.abs().max()) < 1.0
    assert len(set((h.view(torch.int32) & 0xFF).flatten().tolist())) > 200
    narrow = round_sig(h[:m].double(), 11) @ round_sig(h[m:].double(), 11).t()
    d2, w2 = ops.gemm_f32_check(ab[:m], ab[m:], narrow.float().to(dev))
    assert gpu_health.MAX_GEMM_F32_REL_ERR < (d2 / w2) ** 0.5 < gpu_health.MAX_GEMM_REL_ERR


@pytest.mark.gpu
def test_readiness_fp32(dev):
    before = torch.cuda.current_device()
    assert ops.readiness_f8(0, 77, "fp32") < gpu_health.MAX_GEMM_F32_REL_ERR
    assert ops.readiness_f8(0, 77, "fp32") < gpu_health.MAX_GEMM_F32_REL_ERR
    assert ops.readiness_f8(0, 77, "fp32", inject=1) > gpu_health.MAX_GEMM_REL_ERR
    assert ops.readiness_f8(0, 77, "fp32", inject=3) > gpu_health.MAX_GEMM_REL_ERR
    assert torch.cuda.current_device() == before
    rep = gpu_health.readiness_probe(0, matrix=("bf16", "fp32"))
    assert rep["healthy"] and rep["gemm_fp32_rel_err"] < gpu_health.MAX_GEMM_F32_REL_ERR, rep


@pytest.mark.parametrize("what", ["m128", "k24", "k_mismatch", "bf16", "f64_out", "cpu"])
def test_contract(what):
    """Rejected in Python before the native library is touched: runs without a GPU."""
    z = lambda m, k, dt=torch.float32: torch.zeros((m, k), dtype=dt)
    args, kw = {"m128": (z(128, 32), z(256, 32)), "k24": (z(256, 24), z(256, 24)),
                "k_mismatch": (z(256, 32), z(256, 64)), "bf16": (z(256, 32, torch.bfloat16), z(256, 32, torch.bfloat16)),
                "f64_out": (z(256, 32), z(256, 32)), "cpu": (z(256, 32), z(256, 32))}[what], {}  # cpu: valid, no GPU
    if what == "f64_out":
        kw["out"] = torch.zeros((256, 256), dtype=torch.float64)
    with pytest.raises(ops.ProbeError):
        ops.gemm_f32_nt(*args, **kw)
    assert gpu_health._f8_modes(("bf16", "fp32")) == ["fp32"]
    assert ops.F8_FILL_KINDS["f32"] == ops.READINESS_F8_MODES["fp32"] == 7
