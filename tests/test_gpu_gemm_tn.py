"""gemm_tn (C = a^T b, wgrad) and gemm_nn (C = a b, dgrad) of
csrc/gemm_nt.hip, called through the extension entries.

Exact cases use small-integer bf16 operands: every product and every
partial sum is an integer below 2^24, so fp32 accumulation is exact in any
order and the result has to match the fp64 reference bit for bit (fp32
output) or that reference rounded once (bf16 output). The random-data
cases are bounded by the library's own error on the same inputs (constants
measured on MI355X, table in profiles/gemm_tn_r08.md)."""
import pytest
import torch

from chinesener_amd import ops

pytestmark = pytest.mark.gpu

BF16_ULP = 2.0 ** -7          # spacing of bf16 relative to the binade


def _ext():
    return ops.get_ext()


def _pattern(rows, cols, mul_r, mul_c, div, dev="cuda"):
    """Integers in [-3, 3], a different non-symmetric pattern per
    (mul_r, mul_c, div) so that a row/column or A/B mix-up shows."""
    r = torch.arange(rows, device=dev, dtype=torch.int64)[:, None]
    c = torch.arange(cols, device=dev, dtype=torch.int64)[None, :]
    v = (r * mul_r + c * mul_c + (r // div) * c + (c // 5)) % 7 - 3
    return v.to(torch.bfloat16)


def _ref_tn(a, b):
    return (a.double().T @ b.double()).float()


def _ref_nn(a, b):
    return (a.double() @ b.double()).float()


TN_CASES = [  # (T, M, N, split)
    (64, 128, 128, 1),        # one stage, no loop
    (128, 128, 128, 1),       # buffer swap
    (192, 128, 128, 2),       # uneven split of 3 stages
    (320, 128, 128, 3),
    (128, 256, 128, 1),       # M != N: swapped operands, tile indexing
    (128, 128, 384, 1),
    (128, 384, 384, 1),       # 9 workgroups: XCD remap with remainder
    (128, 384, 384, 2),       # 18 workgroups over two slabs
    (8192, 128, 128, 0),      # flagship depth, host split rule
]


@pytest.mark.parametrize("T,M,N,split", TN_CASES)
def test_gemm_tn_exact(T, M, N, split):
    a = _pattern(T, M, 7, 3, 3)
    b = _pattern(T, N, 5, 11, 4)
    ref = _ref_tn(a, b)
    assert ref.abs().max().item() > 0
    got32 = _ext().gemm_tn(a, b, split, True)
    assert got32.dtype == torch.float32 and got32.shape == (M, N)
    assert torch.equal(got32, ref)
    got16 = _ext().gemm_tn(a, b, split, False)
    assert got16.dtype == torch.bfloat16
    assert torch.equal(got16, ref.to(torch.bfloat16))


NN_CASES = [(128, 64, 128), (128, 192, 256), (384, 128, 384),
            (256, 768, 128)]


@pytest.mark.parametrize("M,K,N", NN_CASES)
def test_gemm_nn_exact(M, K, N):
    a = _pattern(M, K, 7, 3, 3)
    b = _pattern(K, N, 5, 11, 4)
    ref = _ref_nn(a, b)
    assert ref.abs().max().item() > 0
    got32 = _ext().gemm_nn(a, b, True)
    assert got32.dtype == torch.float32 and got32.shape == (M, N)
    assert torch.equal(got32, ref)
    got16 = _ext().gemm_nn(a, b, False)
    assert torch.equal(got16, ref.to(torch.bfloat16))


@pytest.mark.parametrize("split", [1, 3])
def test_gemm_tn_reproducible(split):
    torch.manual_seed(3)
    a = torch.randn(512, 256, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(512, 128, device="cuda", dtype=torch.bfloat16)
    c1 = _ext().gemm_tn(a, b, split, True)
    c2 = _ext().gemm_tn(a, b, split, True)
    assert torch.equal(c1, c2)


def test_gemm_nn_reproducible():
    torch.manual_seed(4)
    a = torch.randn(256, 192, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(192, 128, device="cuda", dtype=torch.bfloat16)
    assert torch.equal(_ext().gemm_nn(a, b, False), _ext().gemm_nn(a, b, False))


def test_ineligible_shapes_raise():
    def z(*s):
        return torch.zeros(*s, device="cuda", dtype=torch.bfloat16)
    ext = _ext()
    with pytest.raises(RuntimeError):
        ext.gemm_tn(z(96, 128), z(96, 128), 1, False)      # T % 64
    with pytest.raises(RuntimeError):
        ext.gemm_tn(z(64, 192), z(64, 128), 1, False)      # M % 128
    with pytest.raises(RuntimeError):
        ext.gemm_tn(z(64, 128), z(64, 64), 1, False)       # N % 128
    with pytest.raises(RuntimeError):
        ext.gemm_tn(z(64, 128), z(128, 128), 1, False)     # T mismatch
    with pytest.raises(RuntimeError):
        ext.gemm_tn(z(64, 128), z(64, 128), 2, False)      # split > stages
    with pytest.raises(RuntimeError):
        ext.gemm_tn(z(64, 128).float(), z(64, 128).float(), 1, False)
    with pytest.raises(RuntimeError):
        ext.gemm_nn(z(192, 64), z(64, 128), False)         # M % 128
    with pytest.raises(RuntimeError):
        ext.gemm_nn(z(128, 96), z(96, 128), False)         # K % 64
    with pytest.raises(RuntimeError):
        ext.gemm_nn(z(128, 64), z(128, 128), False)        # K mismatch


# Library error on the same inputs (seeds below), bf16 output against the
# fp64 reference, measured on MI355X: largest |err| and largest |err|/|ref|
# over the elements with |ref| >= 1.
LIB_TN_ABS, LIB_TN_REL = 0.9973, 0.00383476
LIB_NN_ABS, LIB_NN_REL = 0.497815, 0.00387895


def _errors(got, ref64):
    err = (got.double() - ref64).abs()
    big = ref64.abs() >= 1.0
    return err.max().item(), (err[big] / ref64.abs()[big]).max().item()


def _check_random(name, got, lib, ref64, lib_abs, lib_rel):
    e_abs, e_rel = _errors(got, ref64)
    l_abs, l_rel = _errors(lib, ref64)
    ref_max = ref64.abs().max().item()
    # one bf16 ulp of the largest reference value / of any value
    ulp_abs = BF16_ULP * 2.0 ** torch.tensor(ref_max).log2().floor().item()
    print(f"[{name}] ours abs {e_abs:.6g} rel {e_rel:.6g} | library abs "
          f"{l_abs:.6g} rel {l_rel:.6g} | ref max {ref_max:.6g} "
          f"ulp {ulp_abs:.6g}")
    assert e_abs <= max(2.0 * lib_abs, ulp_abs)
    assert e_rel <= max(2.0 * lib_rel, BF16_ULP)


def test_gemm_tn_random():
    torch.manual_seed(11)
    a = torch.randn(8192, 128, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(8192, 256, device="cuda", dtype=torch.bfloat16)
    ref64 = a.double().T @ b.double()
    _check_random("tn 8192x128x256", _ext().gemm_tn(a, b, 0, False),
                  a.T @ b, ref64, LIB_TN_ABS, LIB_TN_REL)


def test_gemm_nn_random():
    torch.manual_seed(12)
    a = torch.randn(256, 3072, device="cuda", dtype=torch.bfloat16)
    b = torch.randn(3072, 128, device="cuda", dtype=torch.bfloat16)
    ref64 = a.double() @ b.double()
    _check_random("nn 256x3072x128", _ext().gemm_nn(a, b, False),
                  a @ b, ref64, LIB_NN_ABS, LIB_NN_REL)
