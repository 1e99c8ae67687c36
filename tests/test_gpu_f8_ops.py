"""FP8 / MXFP8 MFMA probe kernels vs fp64 references of the decoded operands (MI355X only).
Operands are built on the CPU and moved over: nothing here depends on device-side fp8 casts."""
import functools

import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

E4, E5 = torch.float8_e4m3fn, torch.float8_e5m2
PAIRS = [(E4, E4), (E5, E5), (E4, E5)]
# Relative Frobenius bound of the random-operand and readiness tests. The fp32 CPU matmul of the same
# operands meets the bf16 tests' 1e-5 (asserted below); the f8 MFMA's internal accumulation does not:
# measured on MI355X over the six test_random_operands cases, worst 1.332e-5 (E4M3 1.32e-5 / 1.33e-5,
# MXFP8 1.31e-5 / 1.33e-5, E5M2 8.9e-6 / 9.1e-6). The bound is 4x the worst measured value.
F8_REL_BOUND = 4 * 1.332e-5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from dcos_commons_amd import ops

    ops.lib()  # must load: a GPU box without the extension is a failure, not a skip
    return torch.device("cuda", 0)


def decode(x, scale=None):
    x = x.float().double()
    return x if scale is None else x * torch.pow(2.0, scale.double() - 127).repeat_interleave(32, dim=1)


@functools.lru_cache(maxsize=None)
def case(kind, m, n, k, da, db, mx):
    """(a, bt, a_scale, bt_scale, fp64 reference) on the CPU; ``kind`` is 'int' (values -3..3 from two
    different index formulas, scales of the issue's formulas: every partial sum exact) or 'rand'."""
    rows = lambda r: torch.arange(r).view(r, 1)
    kk, kb = torch.arange(k).view(1, k), torch.arange(k // 32).view(1, k // 32)
    sa = sb = None
    if kind == "int":
        a = ((rows(m) * 5 + kk) % 7 - 3).float().to(da)
        bt = ((rows(n) * 3 + kk * 5) % 7 - 3).float().to(db)
        if mx:
            sa = (127 + (rows(m) + 2 * kb) % 4 - 1).to(torch.uint8)
            sb = (127 + (3 * rows(n) + kb) % 4 - 2).to(torch.uint8)
    else:
        g = torch.Generator().manual_seed(m * 31 + n * 7 + k)
        a = torch.randn((m, k), generator=g).to(da)
        bt = torch.randn((n, k), generator=g).to(db)
        if mx:
            sa = torch.randint(120, 135, (m, k // 32), generator=g, dtype=torch.uint8)
            sb = torch.randint(120, 135, (n, k // 32), generator=g, dtype=torch.uint8)
    return a, bt, sa, sb, decode(a, sa) @ decode(bt, sb).t()


def on(dev, *ts):
    return [None if t is None else t.to(dev) for t in ts]


def rel_err(c, ref):
    return (torch.linalg.norm(c.double().cpu() - ref) / torch.linalg.norm(ref)).item()


@pytest.mark.parametrize("da,db", PAIRS, ids=["e4m3", "e5m2", "e4m3xe5m2"])
@pytest.mark.parametrize("m,n,k", [(128, 128, 128), (128, 256, 256), (384, 128, 384), (256, 384, 640),
                                   (1152, 128, 128), (128, 128, 512)])
def test_exact_layout(dev, m, n, k, da, db):
    """K-tiles 1, 2, 3, 4, 5 around the 2-deep ring (3 tiles in flight); 9 row tiles: short last band."""
    from dcos_commons_amd import ops

    a, bt, _, _, ref = case("int", m, n, k, da, db, False)
    assert torch.equal(ops.gemm_f8_nt(*on(dev, a, bt)).cpu().double(), ref)


@pytest.mark.parametrize("m,n,k", [(128, 128, 128), (256, 128, 384), (128, 384, 640)])
def test_mx_exact(dev, m, n, k):
    """Distinct power-of-two scales per row and K-block: a scale from the wrong row, block or byte lane shows."""
    from dcos_commons_amd import ops

    a, bt, sa, sb, ref = case("int", m, n, k, E4, E4, True)
    assert torch.equal(ops.gemm_f8_nt(*on(dev, a, bt, sa, sb)).cpu().double(), ref)


@pytest.mark.parametrize("da,mx", [(E4, False), (E5, False), (E4, True)], ids=["e4m3", "e5m2", "mxfp8"])
@pytest.mark.parametrize("m,n,k", [(256, 384, 512), (512, 128, 2048)])
def test_random_operands(dev, m, n, k, da, mx):
    from dcos_commons_amd import ops

    a, bt, sa, sb, ref = case("rand", m, n, k, da, da, mx)
    cpu32 = decode(a, sa).float() @ decode(bt, sb).float().t()
    assert rel_err(cpu32, ref) < 1e-5
    rel = rel_err(ops.gemm_f8_nt(*on(dev, a, bt, sa, sb)), ref)
    print(f"f8 rel_err {m}x{n}x{k} {da} mx={mx}: {rel:.3e}")
    assert rel < F8_REL_BOUND, rel


@pytest.mark.parametrize("mx", [False, True], ids=["plain", "mx"])
@pytest.mark.parametrize("m,n,k", [(16, 48, 128), (256, 256, 512)])
def test_check_kernel(dev, m, n, k, mx):
    from dcos_commons_amd import ops

    a, bt, sa, sb, ref = case("rand", m, n, k, E4, E4, mx)
    da, dbt, dsa, dsb, c = on(dev, a, bt, sa, sb, ref.float())
    d2, w2 = ops.gemm_f8_check(da, dbt, c, dsa, dsb)
    assert (d2 / w2) ** 0.5 < 1e-5
    assert w2 == pytest.approx(float((ref ** 2).sum()), rel=1e-4)
    lost = c.clone()
    lost[0:16, 16:32] = 0
    d2, _ = ops.gemm_f8_check(da, dbt, lost, dsa, dsb)
    assert d2 == pytest.approx(float((ref[0:16, 16:32] ** 2).sum()), rel=1e-3)
    d2, _ = ops.gemm_f8_check(da, dbt, c, dsa, dsb, inject=1)
    assert d2 == pytest.approx(float((ref[0:16, 0:16] ** 2).sum()), rel=1e-3)


@pytest.mark.parametrize("mode", ["fp8", "bf8", "mxfp8"])
def test_readiness_f8(dev, mode):
    from dcos_commons_amd import ops
    from dcos_commons_amd.ops.gpu_health import MAX_GEMM_REL_ERR

    before = torch.cuda.current_device()
    assert ops.readiness_f8(0, 77, mode) < F8_REL_BOUND
    assert ops.readiness_f8(0, 77, mode) < F8_REL_BOUND
    assert ops.readiness_f8(0, 77, mode, inject=1) > MAX_GEMM_REL_ERR
    assert ops.readiness_f8(0, 77, mode, inject=3) > MAX_GEMM_REL_ERR
    assert ops.readiness_f8(0, 77, mode) < F8_REL_BOUND
    assert torch.cuda.current_device() == before


def test_readiness_probe_with_f8_matrix(dev):
    from dcos_commons_amd.ops import gpu_health

    rep = gpu_health.readiness_probe(0, matrix=("bf16", "fp8", "bf8", "mxfp8"))
    assert rep["healthy"], rep
    assert all(rep[f"gemm_{m}_rel_err"] < gpu_health.MAX_GEMM_REL_ERR for m in ("fp8", "bf8", "mxfp8"))


@pytest.mark.parametrize("what", ["m100", "k192", "k_mismatch", "bf16", "one_scale", "scale_shape"])
def test_contract(dev, what):
    from dcos_commons_amd import ops

    z = lambda m, k, dt=E4: torch.zeros((m, k)).to(dt).to(dev)
    s = lambda m, kb: torch.full((m, kb), 127, dtype=torch.uint8, device=dev)
    args = {"m100": (z(100, 128), z(128, 128)), "k192": (z(128, 192), z(128, 192)),
            "k_mismatch": (z(128, 128), z(128, 256)), "bf16": (z(128, 128, torch.bfloat16), z(128, 128)),
            "one_scale": (z(128, 128), z(128, 128), s(128, 4), None),
            "scale_shape": (z(128, 128), z(128, 128), s(128, 4), s(4, 128))}[what]
    with pytest.raises(ops.ProbeError):
        ops.gemm_f8_nt(*args)
