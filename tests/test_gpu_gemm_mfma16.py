"""The split-f16 GEMM family on the 16x16x32 MFMA shape (gemm_f16x3.hip): a new fragment map, a new accumulator map and
a new park step in every kernel the launcher can pick.  Everything goes through rlcf_gemm_f16x3 on interleaved operand pairs; the
shapes are chosen so that the launcher's own rules select each form (which kernel ran is not asserted).  The tests do not depend
on the MFMA shape: they held on the 32x32x16 form of the family as well."""
import pytest
import torch

from rlcf_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    from rlcf_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


def pairs(L, t):
    """f32 [R, K] -> interleaved operand pairs [R, 2K] halves (32 hi | 32 lo per K block), held as an f32 [R, K] buffer"""
    p = torch.empty(t.shape[0], t.shape[1], device=t.device)
    L.check(L.lib().rlcf_split_pairs(t.contiguous().data_ptr(), p.data_ptr(), t.numel(), L.PREC_F16X3, st()))
    return p


def gemm(L, a2, w2, bias, M, N, K, epi=0, res=None, pair=False, r0=0, entry="rlcf_gemm_f16x3"):
    """rows [r0, r0 + M) of the pair matrix a2 against w2; returns (C,) or (Chi, Clo)"""
    dev = a2.device
    c = None if pair else torch.empty(M, N, device=dev)
    ch = torch.empty(M, N, dtype=torch.float16, device=dev) if pair else None
    cl = torch.empty_like(ch) if pair else None
    ap = a2.data_ptr() + r0 * K * 4
    L.check(getattr(L.lib(), entry)(ap, ap + 64, 2 * K, w2.data_ptr(), w2.data_ptr() + 64, 2 * K, bias.data_ptr(),
                                    res.data_ptr() if res is not None else None, N, None, 0, c.data_ptr() if c is not None else None, N,
                                    ch.data_ptr() if pair else None, cl.data_ptr() if pair else None, N, M, N, K, 1.0, epi, st()))
    torch.cuda.synchronize()
    return (ch, cl) if pair else (c,)


# ------------------------------------------------------------------------------------------------ exact-integer product
def int_operands(M, N, K, dev):
    """Integers in [-8, 8]; W depends asymmetrically on (n, k), A on (m, k) with a cross term: a fragment map that permutes rows, columns
    or k, or swaps the operands, changes the sums.  The lo halves of both come out zero."""
    m = torch.arange(M, device=dev, dtype=torch.int64)[:, None]
    n = torch.arange(N, device=dev, dtype=torch.int64)[:, None]
    k = torch.arange(K, device=dev, dtype=torch.int64)[None, :]
    a = (7 * m + 3 * k + (m * k) % 13) % 17 - 8
    w = (3 * n + 5 * k) % 17 - 8
    b = torch.arange(N, device=dev, dtype=torch.int64) % 11 - 5
    return a, w, b


INT_SHAPES = [
    (8000, 2048, 32), (8000, 2048, 64), (8000, 2048, 96),       # 256 x 256 tiles: one K tile (no prefetch), both ring stages, ring wrap; ragged last M tile
    (8000, 2040, 64),                                             # partial last N tile
    (4100, 2048, 64),                                             # 192-row tiles
    (2500, 2048, 64), (1182, 768, 64), (700, 512, 128), (300, 768, 3072),     # 256 x 128, eight-wave 128 x 128, 64 x 128, K-sliced forms
]


def check_int(L, dev, M, N, K, entry):
    a, w, b = int_operands(M, N, K, dev)
    a2, w2 = pairs(L, a.float()), pairs(L, w.float())
    # |sum| <= 64 K + 5 < 2^24: every product and every partial sum is exact in f32, whatever the summation order — and exact in the
    # float64 matrix product that stands in for the int64 one (torch has no integer matmul on the GPU); compared as int64
    ref = (a.double() @ w.double().t() + b.double()).to(torch.int64)
    (c,) = gemm(L, a2, w2, b.float(), M, N, K, entry=entry)
    got = c.to(torch.int64)
    assert torch.equal(c, got.float())                  # integers came out
    bad = (got != ref)
    assert not bool(bad.any()), (int(bad.sum()), bad.nonzero()[:4].tolist())


@pytest.mark.parametrize("M,N,K", INT_SHAPES)
def test_exact_integer_product_equals_the_int64_product(L, dev, M, N, K):
    """Bias integer, epilogue NONE, f32 output: the result must EQUAL the integer product, element for element."""
    check_int(L, dev, M, N, K, "rlcf_gemm_f16x3")


def test_exact_integer_product_two_pass_form(L, dev):
    """The same with W announced as lying on the f16 grid (its lo halves ARE zero here): the two-pass kernels."""
    check_int(L, dev, 8000, 2048, 128, "rlcf_gemm_f16x3_grid_w")


# ------------------------------------------------------------------------------------------------ random data against float64
_RAND = {}


def rand_case(L, dev, M, N, K):
    """operands, their pairs and the float64 product on sampled rows: computed once per shape, shared by the epilogue kinds, never modified"""
    key = (M, N, K)
    if key not in _RAND:
        a = synth.normal(21, f"m16.a.{M}.{K}", (M, K), device=dev)
        w = synth.normal(21, f"m16.w.{N}.{K}", (N, K), device=dev) * K ** -0.5
        b = synth.normal(21, f"m16.b.{N}", (N,), device=dev) * 0.1
        x = synth.normal(21, f"m16.x.{M}.{N}", (M, N), device=dev)
        rows = torch.arange(0, M, 53, device=dev)
        ref = a[rows].double() @ w.double().t() + b.double()
        _RAND[key] = dict(a2=pairs(L, a), w2=pairs(L, w), b=b, x=x, rows=rows, ref=ref)
    return _RAND[key]


@pytest.mark.parametrize("kind", [1, 2, 3, 4])           # f32; f32 + residual; QuickGELU -> pairs; pairs
@pytest.mark.parametrize("M,N,K", [(8000, 2048, 768), (4100, 768, 3072)])
def test_random_product_against_float64(L, dev, M, N, K, kind):
    """synth.normal operands, the four compile-time epilogues of the forward towers; bar: 3e-4 on sampled rows, the bar of
    test_gemm_192_row_tiles_bit_identical_to_the_other_tile_shapes.  Max and mean |error| are printed (profiles/r7_notes.md keeps them
    for both MFMA shapes)."""
    d = rand_case(L, dev, M, N, K)
    epi, res, pair = (1 if kind == 3 else 0), (d["x"] if kind == 2 else None), kind >= 3
    out = gemm(L, d["a2"], d["w2"], d["b"], M, N, K, epi=epi, res=res, pair=pair)
    got = (out[0].float() + out[1].float()) if pair else out[0]
    ref = d["ref"]
    if epi == 1:
        ref = ref * torch.sigmoid(1.702 * ref)
    if res is not None:
        ref = ref + res[d["rows"]].double()
    err = (got[d["rows"]].double() - ref).abs()
    print(f"[mfma16 random] M={M} N={N} K={K} kind={kind}: max|err|={float(err.max()):.3e} mean|err|={float(err.mean()):.3e}")
    assert torch.isfinite(got).all()
    assert float(err.max()) < 3e-4


# ------------------------------------------------------------------------------------------------ cross-form identity
@pytest.mark.parametrize("pair", [False, True])
def test_one_call_bit_identical_to_four_calls_of_2000_rows(L, dev, pair):
    """[8000, 2048, 768] in one call (256 x 256 tiles) against the same product as four calls of 2000 rows (the 256 x 128 / 128 x 128
    kernels): the same sum of the same products in the same order whatever the kernel, so the outputs must be bit-identical."""
    M, N, K = 8000, 2048, 768
    d = rand_case(L, dev, M, N, K)
    whole = gemm(L, d["a2"], d["w2"], d["b"], M, N, K, pair=pair)
    parts = [gemm(L, d["a2"], d["w2"], d["b"], 2000, N, K, pair=pair, r0=r0) for r0 in range(0, M, 2000)]
    for i, t in enumerate(whole):
        assert torch.equal(t, torch.cat([p[i] for p in parts]))
