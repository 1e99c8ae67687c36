"""2:4 sparse bf16 MFMA probe kernel vs CPU float64 matmuls of the expanded A (MI355X only, except the contract
test). The exact cases use small integers, for which every summation order gives the same bits, and metadata
that walks all six legal nibbles: a wrong lane, register, K pairing, index bit order or abid half changes a sum."""
import functools

import pytest

torch = pytest.importorskip("torch")

from dcos_commons_amd import ops  # noqa: E402
from dcos_commons_amd.ops import gpu_health  # noqa: E402

TM, TN, TK, R = ops.SP_TILE_M, ops.SP_TILE_N, ops.SP_TILE_K, ops.SP_RING
CODES = (4, 8, 12, 9, 13, 14)      # (first, second) = (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), first in bits 1:0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ops.lib()  # must load: a GPU box without the extension is a failure, not a skip
    return torch.device("cuda", 0)


def expand_cpu(vals, meta):
    """The storage format, read back: group g of a row puts values 2g, 2g + 1 at the two positions of its nibble."""
    m, k = vals.shape[0], 2 * vals.shape[1]
    nib = torch.stack((meta & 15, meta >> 4), -1).reshape(m, k // 4).long()
    a = torch.zeros((m, k // 4, 4), dtype=vals.dtype)
    a.scatter_(-1, torch.stack((nib & 3, nib >> 2), -1), vals.reshape(m, k // 4, 2))
    return a.reshape(m, k)


@functools.lru_cache(maxsize=None)
def case(kind, m, n, k):
    """(a_vals, a_meta, bt, float64 reference expand(a) @ bt.t()) on the CPU. 'index': integers of both signs,
    |a| <= 7 and |b| <= 16, exact in bf16; the four K positions of a group hold four distinct b values, so a wrong
    mux choice changes the sum; the nibble of group g of row r is CODES[(r + 2g + g // 8) % 6], which differs
    between neighbouring rows and neighbouring groups. 'rand': sp24_compress of randn."""
    rows, col = (lambda r: torch.arange(r).view(r, 1)), (lambda c: torch.arange(c).view(1, c))
    if kind == "index":
        vals = ((7 * rows(m) + 3 * col(k // 2)) % 15 - 7).to(torch.bfloat16)
        bt = (col(k) % 4 + 1 + 4 * ((rows(n) + col(k) // 4) % 7) - 12).to(torch.bfloat16)
        nib = torch.tensor(CODES)[(rows(m) + 2 * col(k // 4) + col(k // 4) // 8) % 6].reshape(m, k // 8, 2)
        meta = (nib[..., 0] | (nib[..., 1] << 4)).to(torch.uint8)
        assert set(nib.unique().tolist()) == set(CODES)
        assert vals.min() < 0 < vals.max() and bt.min() < 0 < bt.max()
    else:
        g = torch.Generator().manual_seed(m * 31 + n * 7 + k)
        vals, meta = ops.sp24_compress(torch.randn((m, k), generator=g).to(torch.bfloat16))
        bt = torch.randn((n, k), generator=g).to(torch.bfloat16)
    a = expand_cpu(vals, meta)
    if kind == "index":   # every partial sum, in any order, is an integer below 2^24: exact in fp32
        assert float((a.double().abs() @ bt.double().abs().t()).max()) < 2 ** 24
    return vals, meta, bt, a.double() @ bt.double().t()


@pytest.mark.gpu
@pytest.mark.parametrize("m,n,k", [(TM, TN, TK), (TM, TN, 2 * TK), (TM, TN, 3 * TK), (TM, TN, (R + 2) * TK),
                                   (TM, 2 * TN, TK), (2 * TM, TN, TK), (9 * TM, TN, TK)])
def test_exact(dev, m, n, k):
    """K-tiles 1, 2, 3, R + 2 around the ring; two N tiles; two M tiles; 9 M tiles: the short last band of
    grouped_tile. Bit-equal."""
    vals, meta, bt, ref = case("index", m, n, k)
    out = ops.gemm_sp_bf16_nt(vals.to(dev), meta.to(dev), bt.to(dev))
    assert out.dtype == torch.float32 and out.is_contiguous()
    assert torch.equal(out.cpu(), ref.float())


@pytest.mark.gpu
def test_random(dev):
    """The bound tests/test_gpu_ops.py holds the dense bf16 kernels to: the same terms, summed in fp32."""
    vals, meta, bt, ref = case("rand", 2 * TM, 3 * TN, 4 * TK)
    out = ops.gemm_sp_bf16_nt(vals.to(dev), meta.to(dev), bt.to(dev)).cpu().double()
    rel = float(torch.linalg.norm(out - ref) / torch.linalg.norm(ref))
    print(f"rel {rel:.3e}")
    assert rel < 1e-5


@pytest.mark.gpu
def test_expand_and_compress(dev):
    vals, meta, _, _ = case("index", TM, TN, 2 * TK)
    x = expand_cpu(vals, meta)
    assert torch.equal(ops.sp24_expand(vals.to(dev), meta.to(dev)).cpu(), x)
    assert torch.equal(ops.sp24_expand(*ops.sp24_compress(x.to(dev))).cpu(), x)     # x is already 2:4
    assert torch.equal(expand_cpu(*ops.sp24_compress(x)), x)
    filled = torch.zeros((TM, 64), dtype=torch.uint8, device=dev)
    ops.f8_fill(filled, seed=5, kind="meta24")
    assert set(torch.cat((filled & 15, filled >> 4)).unique().tolist()) == set(CODES)


@pytest.mark.gpu
def test_readiness_sparse24(dev):
    before = torch.cuda.current_device()
    assert ops.readiness_f8(0, 77, "sparse24") < gpu_health.MAX_GEMM_REL_ERR
    assert ops.readiness_f8(0, 77, "sparse24") < gpu_health.MAX_GEMM_REL_ERR
    assert ops.readiness_f8(0, 77, "sparse24", inject=1) > gpu_health.MAX_GEMM_REL_ERR
    assert ops.readiness_f8(0, 77, "sparse24", inject=3) > gpu_health.MAX_GEMM_REL_ERR
    assert torch.cuda.current_device() == before
    rep = gpu_health.readiness_probe(0, matrix=("bf16", "sparse24"))
    assert rep["healthy"] and rep["gemm_sparse24_rel_err"] < gpu_health.MAX_GEMM_REL_ERR, rep


@pytest.mark.parametrize("what,match", [("m128", "M % 256"), ("k64", "K % 128"), ("meta_shape", r"a_meta must be"),
                                        ("meta_dtype", "uint8"), ("f32", "bfloat16"), ("f64_out", "float32"),
                                        ("cpu", "one GPU")])
def test_contract(what, match):
    """Rejected in Python before the native library is touched: runs without a GPU."""
    m, k = (128 if what == "m128" else TM), (64 if what == "k64" else TK)
    dt = torch.float32 if what == "f32" else torch.bfloat16
    vals, bt = torch.zeros((m, k // 2), dtype=dt), torch.zeros((TN, k), dtype=dt)
    meta = torch.zeros((m, k // 4 if what == "meta_shape" else k // 8),
                       dtype=torch.int8 if what == "meta_dtype" else torch.uint8)
    out = torch.zeros((m, TN), dtype=torch.float64) if what == "f64_out" else None
    with pytest.raises(ops.ProbeError, match=match):
        ops.gemm_sp_bf16_nt(vals, meta, bt, out=out)          # "cpu": valid operands, no GPU
    assert gpu_health._f8_modes(("bf16", "sparse24")) == ["sparse24"]
    assert ops.SP_TILE_K % 8 == 0 and ops.F8_FILL_KINDS["meta24"] == 6 and ops.READINESS_F8_MODES["sparse24"] == 6
