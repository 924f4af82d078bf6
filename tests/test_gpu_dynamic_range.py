"""GPU: the kernels on data with the dynamic range of trained CLIP weights (rlcf_amd/synth.py, profile "trained"), each against a
float64 CPU computation of the same operation.  The bars are stated against the operation's own conditioning (for products:
sum_k |a_ik w_jk|, not |c_ij|), so a row that cancels to ~0 from large terms is held to the same bar as any other.

Split-f16 error model (RLCF_PREC_F16X3): x = hi + lo with hi = f16(x), lo = f16(x - hi) represents x to 22 bits when lo is a normal
f16 number; a_hi w_hi + a_hi w_lo + a_lo w_hi drops a_lo w_lo (<= 2^-22 |a||w|) and the lo roundings (<= 2^-22 |a||w| each), f32
accumulation adds ~sqrt(K / 16) * 2^-24 of the running sums.  Bound used: 2^-17 sum|a||w| (K <= 3072) — 64x below the 2^-11 sum|a||w|
a product that lost one lo half would show.  The f32 path (RLCF_PREC_F32) is held to the same bar."""
import functools
import math

import pytest
import torch

from oracle import rlcf_ref as RR
from rlcf_amd import synth

pytestmark = pytest.mark.gpu

TOL = 2.0 ** -17


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


def sample_rows(M):
    """the rows checked against float64: the first and last 64 (tile edges, the tail tile) and 128 spread over the middle"""
    mid = torch.linspace(64, max(M - 65, 64), 128).long()
    return torch.unique(torch.cat([torch.arange(min(64, M)), mid, torch.arange(max(M - 64, 0), M)]).clamp(0, M - 1))


def operand_a(kind, M, K, dev):
    a = synth.normal(31, f"dr.a.{M}.{K}", (M, K), device=dev)
    if kind == "massive":                      # residual-stream-like: a few channels x300 .. x1000
        a[:, 7] *= 300.0
        a[:, K // 3] *= -500.0
        a[:, K - 5] *= 1000.0
    elif kind == "small":                      # every entry in [1e-4, 1e-2]: lo halves subnormal without a pre-scale
        u = synth.raw_u32(31, f"dr.u.{M}.{K}", M * K, 0, device=dev).reshape(M, K).double() / 2 ** 32
        a = (torch.sign(a) * torch.pow(10.0, -4.0 + 2.0 * u)).float()
    elif kind == "large":                      # up to ~3e4 (inside f16, 2^15 > 3e4)
        a = (a * 6000.0).clamp(-3.2e4, 3.2e4)
    elif kind == "cancel":                     # rows whose products cancel exactly: a = [h, h], w = [v, -v]
        a = a * 100.0
        a[:, K // 2:] = a[:, :K // 2]
    return a.contiguous()


@functools.lru_cache(maxsize=8)
def operand_w(N, K, grid, cancel):
    w = synth._student_t(31, f"dr.w.{N}.{K}", (N, K), K ** -0.5)
    if cancel:
        w[:, K // 2:] = -w[:, :K // 2]
    return (w.half().float() if grid else w).contiguous()


def gemm_ref(a, w, alpha, bias):
    """float64 product and its conditioning sum_k |a||w| on the sampled rows"""
    v = alpha * (a.double() @ w.double().t())
    s = abs(alpha) * (a.double().abs() @ w.double().abs().t())
    if bias is not None:
        v = v + bias.double()
        s = s + bias.double().abs()
    return v, s


# shapes of the engine: the ViT-B/16 N = 64 step (12 608 token rows, the four products of a block), the text tower (4 095 rows) and an
# odd M (1 001) — large, mid-sized and ragged grids of the split-f16 and f32 kernels (which tile form each takes is not asserted here)
GEMM_SHAPES = [(12608, 2304, 768), (12608, 768, 768), (12608, 3072, 768), (12608, 768, 3072), (4095, 1536, 512), (1001, 768, 3072)]


@pytest.mark.parametrize("M,N,K", GEMM_SHAPES)
@pytest.mark.parametrize("kind", ["massive", "small", "large", "cancel"])
@pytest.mark.parametrize("prec", [0, 2])
def test_gemm_nt_trained_range(L, dev, M, N, K, kind, prec):
    """rlcf_gemm_nt against float64 on the sampled rows: |c - ref| <= 2^-17 (sum|a||w| + |b|); Student-t weights, raw for the
    split-f16 path with 'massive' / 'cancel' data and on the fp16 grid otherwise"""
    grid = kind in ("small", "large")
    a = operand_a(kind, M, K, dev)
    w = operand_w(N, K, grid, kind == "cancel")
    b = None if kind == "cancel" else synth._student_t(31, f"dr.b.{N}", (N,), 1.0)
    wd = w.to(dev)
    bd = b.to(dev) if b is not None else None
    c = torch.full((M, N), float("nan"), device=dev)
    L.check(L.lib().rlcf_gemm_nt(a.data_ptr(), K, wd.data_ptr(), K, bd.data_ptr() if bd is not None else None, None, N, None, N,
                                 c.data_ptr(), N, M, N, K, 1.0, 0, prec, st()))
    rows = sample_rows(M)
    ref, s = gemm_ref(a[rows.to(dev)].cpu(), w, 1.0, b)
    got = c[rows.to(dev)].cpu().double()
    assert torch.isfinite(got).all()
    err = (got - ref).abs() / s.clamp_min(1e-30)
    assert err.max().item() <= TOL, (err.max().item(), kind)


@pytest.mark.parametrize("M,N,K", [(12608, 3072, 768), (4095, 2048, 512)])
@pytest.mark.parametrize("epi", [1, 2])
@pytest.mark.parametrize("prec", [0, 2])
def test_gemm_nt_quickgelu_epilogues_at_overflow(L, dev, M, N, K, epi, prec):
    """epilogues 1 (QuickGELU) and 2 (its backward) with pre-activations and aux in +-100 and beyond: the fast exp2 / rcp forms reach
    their overflow (|1.702 x log2 e| > 128) and denormal ranges; results must stay finite and within the bar propagated through
    |QuickGELU'| <= 1.13, plus 2^-20 of the value for the fast forms (of |v| for the backward form, whose factor g(aux) is an f32
    difference near its zero)."""
    a = synth.normal(32, f"ge.a.{M}.{K}", (M, K), device=dev)
    w = synth._student_t(32, f"ge.w.{N}.{K}", (N, K), 60.0 * K ** -0.5)
    b = synth.normal(32, f"ge.b.{N}", (N,), 20.0)
    aux = (synth.normal(32, f"ge.x.{M}.{N}", (M, N), 60.0, device=dev)).contiguous()
    wd, bd = w.to(dev), b.to(dev)
    c = torch.full((M, N), float("nan"), device=dev)
    L.check(L.lib().rlcf_gemm_nt(a.data_ptr(), K, wd.data_ptr(), K, bd.data_ptr(), None, N, aux.data_ptr() if epi == 2 else None, N,
                                 c.data_ptr(), N, M, N, K, 1.0, epi, prec, st()))
    rows = sample_rows(M)
    v, s = gemm_ref(a[rows.to(dev)].cpu(), w, 1.0, b)
    got = c[rows.to(dev)].cpu().double()
    assert torch.isfinite(got).all()
    if epi == 1:
        assert v.abs().max().item() > 100 and (v.abs() > 80).double().mean().item() > 0.05
        ref = v * torch.sigmoid(1.702 * v)
        bar = 1.13 * TOL * s + 2.0 ** -20 * ref.abs()
    else:
        f = aux[rows.to(dev)].cpu().double()
        assert f.abs().max().item() > 200
        sg = torch.sigmoid(1.702 * f)
        g = sg * (1 + 1.702 * f * (1 - sg))
        ref = v * g
        bar = TOL * s * g.abs() + 2.0 ** -20 * v.abs()       # f32 g(f) is known to ~2^-21 absolute (it cancels at its zero, f ~ -1.28)
    assert ((got - ref).abs() <= bar + 1e-30).all(), ((got - ref).abs() / (bar + 1e-30)).max().item()


def test_gemm_nt_operands_outside_the_f16_range(L, dev):
    """split-f16 path: an operand above 65504 still gives the float64 result (the op-level call pre-scales each operand by a power of
    two); an infinite operand is refused with an error instead of an inf / NaN product; a NaN element is pinned to propagate into its
    own row, as in the f32 path"""
    M, N, K = 1001, 768, 768
    a = synth.normal(33, "oor.a", (M, K), device=dev)
    a[3, 5] = 2.0e5
    a[700, 100] = -9.0e4
    w = synth._student_t(33, "oor.w", (N, K), K ** -0.5)
    wd = w.to(dev)
    c = torch.full((M, N), float("nan"), device=dev)
    L.check(L.lib().rlcf_gemm_nt(a.data_ptr(), K, wd.data_ptr(), K, None, None, N, None, N, c.data_ptr(), N, M, N, K, 1.0, 0, 2, st()))
    rows = torch.tensor([0, 3, 500, 700, 1000])
    ref, s = gemm_ref(a[rows.to(dev)].cpu(), w, 1.0, None)
    err = (c[rows.to(dev)].cpu().double() - ref).abs() / s
    assert err.max().item() <= TOL, err.max().item()
    a[9, 9] = float("nan")                                          # NaN: not refused, propagates into its row only (as in f32)
    L.check(L.lib().rlcf_gemm_nt(a.data_ptr(), K, wd.data_ptr(), K, None, None, N, None, N, c.data_ptr(), N, M, N, K, 1.0, 0, 2, st()))
    cc = c.cpu()
    assert torch.isnan(cc[9]).all() and torch.isfinite(cc[torch.arange(M) != 9]).all()
    a[9, 9] = float("inf")
    with pytest.raises(L.RlcfError):
        L.check(L.lib().rlcf_gemm_nt(a.data_ptr(), K, wd.data_ptr(), K, None, None, N, None, N, c.data_ptr(), N, M, N, K, 1.0, 0, 2, st()))


def _pairs(L, x, dev):
    p = torch.empty(x.shape[0], x.shape[1], device=dev)           # interleaved (hi | lo) per 32 columns: 4 bytes per element
    L.check(L.lib().rlcf_split_pairs(x.data_ptr(), p.data_ptr(), x.numel(), L.PREC_F16X3, st()))
    return p


@pytest.mark.parametrize("M,N,K", [(12608, 2304, 768), (4095, 512, 2048), (1001, 768, 3072)])
@pytest.mark.parametrize("grid", [False, True])
def test_gemm_f16x3_pre_split_pairs(L, dev, M, N, K, grid):
    """rlcf_gemm_f16x3 on operands split as the engine splits them: the activation at scale 1 (massive channels, O(1) bulk), the
    Student-t weight pre-scaled by the power of two that lifts max|w| into [2^9, 2^10) (make_split), undone in alpha; f32 output and
    the split-pair output (hi + lo read back in float64: 2^-22 |c| more)"""
    a = operand_a("massive", M, K, dev)
    w = operand_w(N, K, grid, False)
    sh = 9 - math.floor(math.log2(w.abs().max().item()))
    ws = (w * 2.0 ** sh).to(dev)
    b = synth._student_t(34, f"x3.b.{N}", (N,), 1.0)
    bd = b.to(dev)
    ap, wp = _pairs(L, a, dev), _pairs(L, ws, dev)
    lo = lambda t: t.data_ptr() + 64
    c = torch.full((M, N), float("nan"), device=dev)
    chi = torch.zeros(M, N, dtype=torch.float16, device=dev)
    clo = torch.zeros(M, N, dtype=torch.float16, device=dev)
    alpha = 2.0 ** -sh
    L.check(L.lib().rlcf_gemm_f16x3(ap.data_ptr(), lo(ap), 2 * K, wp.data_ptr(), lo(wp), 2 * K, bd.data_ptr(), None, 0, None, 0,
                                    c.data_ptr(), N, None, None, 0, M, N, K, alpha, 0, st()))
    L.check(L.lib().rlcf_gemm_f16x3(ap.data_ptr(), lo(ap), 2 * K, wp.data_ptr(), lo(wp), 2 * K, bd.data_ptr(), None, 0, None, 0,
                                    None, 0, chi.data_ptr(), clo.data_ptr(), N, M, N, K, alpha, 0, st()))
    rows = sample_rows(M)
    rd = rows.to(dev)
    ref, s = gemm_ref(a[rd].cpu(), w, 1.0, b)
    got = c[rd].cpu().double()
    assert torch.isfinite(got).all()
    assert ((got - ref).abs() / s).max().item() <= TOL
    pair = chi[rd].cpu().double() + clo[rd].cpu().double()
    assert ((pair - ref).abs() <= TOL * s + 2.0 ** -22 * ref.abs()).all()


@pytest.mark.parametrize("M,N,K", [(239, 2048, 512), (77, 512, 2048), (256, 1536, 768)])
@pytest.mark.parametrize("mode", ["scale1", "amax_in"])
def test_gemm_skinny_trained_range(L, dev, M, N, K, mode):
    """rlcf_gemm_skinny (few-row products of the one-image path) on residual-stream-like rows with massive channels and a Student-t
    weight on the fp16 grid; the operand scale 1 (forward activations) and from max|A|"""
    a = operand_a("massive", M, K, dev)
    w = operand_w(N, K, True, False)
    b = synth._student_t(35, f"sk.b.{N}", (N,), 1.0)
    wd, bd = w.to(dev), b.to(dev)
    wp = _pairs(L, wd, dev)
    amax = a.abs().max().reshape(1).contiguous()
    c = torch.full((M, N), float("nan"), device=dev)
    L.check(L.lib().rlcf_gemm_skinny(a.data_ptr(), K, wp.data_ptr(), bd.data_ptr(), None, N, None, 0, c.data_ptr(), N, M, N, K, 1.0, 0,
                                     amax.data_ptr() if mode == "amax_in" else None, 0, st()))
    ref, s = gemm_ref(a.cpu(), w, 1.0, b)
    got = c.cpu().double()
    assert torch.isfinite(got).all()
    assert ((got - ref).abs() / s).max().item() <= TOL


# ------------------------------------------------------------------------------ LayerNorm
def ln_rows(kind, rows, width, dev):
    x = synth.normal(36, f"ln.{kind}.{width}", (rows, width), 1.0)
    if kind == "offset":              # common offset: mean 1e3, std 0.1
        x = 1000.0 + 0.1 * x
    elif kind == "spike":             # one channel at 300, the rest O(1)
        x[:, width // 5] = 300.0
    elif kind == "constant":          # var = 0
        x = torch.full((rows, width), 3.0) + torch.arange(rows).float()[:, None] * 0.25
    elif kind == "offset8":           # |mean| / std = 8: the top of what a trained tower's residual rows reach (test_trained_profile)
        x = 8.0 + x
    return x.contiguous()


def ln_gain(width):
    g = synth._gain(36, f"ln.g.{width}", width, ())
    b = synth._bias(36, f"ln.b.{width}", width, 0.05, 16)
    return g, b


@pytest.mark.parametrize("width", [512, 768, 1024, 776])
@pytest.mark.parametrize("kind", ["offset", "spike", "constant", "offset8"])
def test_layernorm_trained_range(L, dev, width, kind):
    """rlcf_layernorm_fwd / _bwd against float64 on rows with a large common offset, a spike channel, constant rows (var = 0) and
    gains log-uniform over [0.02, 30] with zeros.  Forward bar per element: |gamma| 2^-18 (|x_hat| + |mean| / sqrt(var + eps)) +
    2^-22 |beta| (the mean of f32 inputs is known to 2^-24 |mean| per term: an offset row is ill-conditioned, and a one-pass
    variance would be off by orders of magnitude more).  Backward bars normwise per row with the same conditioning factor."""
    rows = 300
    x = ln_rows(kind, rows, width, dev)
    g, b = ln_gain(width)
    dy = synth.normal(36, f"ln.dy.{width}", (rows, width), 1.0)
    xd, gd, bd, dyd = x.to(dev), g.to(dev), b.to(dev), dy.to(dev)
    y = torch.full_like(xd, float("nan"))
    L.check(L.lib().rlcf_layernorm_fwd(xd.data_ptr(), gd.data_ptr(), bd.data_ptr(), y.data_ptr(), rows, width, st()))
    x64 = x.double().requires_grad_(True)
    g64 = g.double().requires_grad_(True)
    b64 = b.double().requires_grad_(True)
    ref = torch.nn.functional.layer_norm(x64, (width,), g64, b64, 1e-5)
    mu = x.double().mean(1, keepdim=True)
    sd = (x.double().var(1, unbiased=False, keepdim=True) + 1e-5).sqrt()
    cond = 1.0 + mu.abs() / sd
    xh = (x.double() - mu) / sd
    bar = g.double().abs() * 2.0 ** -18 * (xh.abs() + cond) + 2.0 ** -22 * b.double().abs()
    err = (y.cpu().double() - ref.detach()).abs()
    assert (err <= bar + 1e-30).all(), (err / (bar + 1e-30)).max().item()
    (ref * dy.double()).sum().backward()
    dx = torch.full_like(xd, float("nan"))
    dg = torch.zeros_like(gd)
    db = torch.zeros_like(bd)
    L.check(L.lib().rlcf_layernorm_bwd(xd.data_ptr(), gd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), rows,
                                       width, st()))
    gdy = (g.double() * dy.double()).abs()
    dx_bar = 2.0 ** -16 * cond * gdy.amax(1, keepdim=True) / sd * (1 + xh.abs().amax(1, keepdim=True))
    assert ((dx.cpu().double() - x64.grad).abs() <= dx_bar).all()
    assert ((db.cpu().double() - b64.grad).abs() <= 2.0 ** -18 * dy.double().abs().sum(0) + 1e-30).all()
    dg_bar = 2.0 ** -16 * (dy.double().abs() * (xh.abs() + cond)).sum(0)
    assert ((dg.cpu().double() - g64.grad).abs() <= dg_bar + 1e-30).all()


@pytest.mark.parametrize("form,width", [("resid16", 512), ("resid16", 768), ("resid16", 1024), ("resid16", 776),
                                        ("mode2", 512), ("mode2", 768), ("mode2", 1024)])
@pytest.mark.parametrize("kind", ["spike", "offset8", "centred", "constant0"])
def test_fold_row_statistics_in_the_reachable_range(L, dev, form, width, kind):
    """The f16 LayerNorm fold's row statistics, one-pass (sum, sum of squares) in f32: rlcf_resid16_init (whole rows, one wave each) and
    rlcf_gemm_f16_ln mode 2 (64-column partials written by the GEMM epilogue; the update here adds exact zeros, so the stored rows are
    the input's) followed by rlcf_ln_stats_final.  (mean, rstd) against the float64 statistics OF THE STORED f16 ROWS.  The one-pass
    variance q / n - mean^2 loses (mean / std)^2 2^-24 relative: the range pinned here is what a trained tower's residual rows reach
    (|mean| / std <= 8, test_trained_profile; massive channels make rows spiky, not offset) — rows with a large common offset
    (mean 1e3, std 0.1) are outside it, see include/rlcf_hip.h."""
    rows = 300
    if kind == "centred":
        x = synth.normal(37, f"r16.{width}", (rows, width), 2.0)
    elif kind == "constant0":         # exactly representable constant rows: the sums are exact, var = 0 exactly
        x = torch.full((rows, width), 0.5)
    else:
        x = ln_rows(kind, rows, width, dev)
    mr = torch.full((rows, 2), float("nan"), device=dev)
    if form == "resid16":
        xd = x.to(dev).contiguous()
        x16 = torch.empty(rows, width, dtype=torch.float16, device=dev)
        L.check(L.lib().rlcf_resid16_init(xd.data_ptr(), x16.data_ptr(), mr.data_ptr(), rows, width, st()))
    else:
        K = 256
        x16 = x.half().to(dev).contiguous()
        a16 = torch.zeros(rows, K, dtype=torch.float16, device=dev)
        w16 = torch.zeros(width, K, dtype=torch.float16, device=dev)
        b = torch.zeros(width, device=dev)
        P = width // 64
        part = torch.full((P, rows, 2), float("nan"), device=dev)
        L.check(L.lib().rlcf_gemm_f16_ln(a16.data_ptr(), K, w16.data_ptr(), K, b.data_ptr(), x16.data_ptr(), width, rows, width, K, 1.0,
                                         L.EPI_NONE, 2, None, None, part.data_ptr(), st()))
        L.check(L.lib().rlcf_ln_stats_final(part.data_ptr(), P, rows, width, mr.data_ptr(), st()))
    s16 = x16.cpu().double()
    assert torch.equal(s16, x.half().double())
    mu = s16.mean(1)
    var = s16.var(1, unbiased=False)
    rstd = (var + 1e-5).rsqrt()
    got = mr.cpu().double()
    assert ((got[:, 0] - mu).abs() <= 2.0 ** -20 * s16.abs().mean(1) + 1e-30).all()
    assert ((got[:, 1] - rstd).abs() <= 2.0 ** -16 * rstd).all(), ((got[:, 1] - rstd).abs() / rstd).max().item()


# ------------------------------------------------------------------------------ entropy / selection at logit_scale 100
def saturated_logits(n, C):
    """x100 logits: near-one-hot rows (entropies that underflow), exact duplicates (ties, some straddling the cut), near-uniform rows"""
    base = synth.normal(38, f"es.{n}.{C}", (n, C), 0.05) * 100.0
    hot = synth.randint(38, f"es.hot.{n}.{C}", n, 0, C)
    for i in range(0, n, 3):
        base[i, int(hot[i])] += 100.0 * (0.3 + 0.1 * (i % 7))       # one class ahead by 30 .. 90
    for i in range(1, n, 8):                                         # exact duplicates of the previous row: entropy ties
        base[i] = base[i - 1]
    return base.contiguous()


def straddle_logits(n, C, n_sel):
    """x100 logits ordered from one-hot (class ahead by 95) to flatter rows, with rows n_sel - 1 and n_sel identical: an exact
    entropy tie across the int(N p) cut"""
    base = synth.normal(38, f"es.st.{n}.{C}", (n, C), 0.05) * 100.0
    for i in range(n):
        base[i, i % C] += 95.0 - 9.0 * i
    base[n_sel] = base[n_sel - 1]
    return base.contiguous()


@pytest.mark.parametrize("n,C,p,shape", [(64, 1000, 0.1, "mixed"), (64, 16, 0.1, "mixed"), (32, 200, 0.5, "mixed"), (8, 1000, 0.3, "mixed"),
                                         (10, 16, 0.3, "straddle"), (10, 1000, 0.3, "straddle")])
def test_entropy_select_saturated(L, dev, n, C, p, shape):
    """rlcf_entropy_select on x100 logits against oracle/rlcf_ref.py in float64: entropies to 2e-6 absolute (underflowing ones
    included, never NaN); the selected rows are the int(N p) lowest — compared as a multiset of float64 entropies
    where ties make the reference's order ambiguous; the selection is in ascending order of the kernel's own entropies"""
    n_sel = int(n * p)
    lg = saturated_logits(n, C) if shape == "mixed" else straddle_logits(n, C, n_sel)
    ent = torch.full((n,), float("nan"), device=dev)
    idx = torch.full((n_sel,), -1, dtype=torch.int32, device=dev)
    L.check(L.lib().rlcf_entropy_select(lg.to(dev).data_ptr(), n, C, n_sel, ent.data_ptr(), idx.data_ptr(), st()))
    e64 = RR.entropy_rows(lg.double())
    e = ent.cpu().double()
    assert torch.isfinite(e).all()
    assert (e - e64).abs().max().item() <= 2e-6
    assert (e64 < 1e-12).any()                                      # the regime: some entropies underflow
    sel = idx.cpu().long()
    assert len(set(sel.tolist())) == n_sel and sel.min() >= 0 and sel.max() < n
    assert (e[sel][1:] >= e[sel][:-1]).all()
    srt = e64.sort().values
    if shape == "straddle":                                         # the tie straddles the cut: the reference's order is ambiguous there
        assert srt[n_sel - 1] == srt[n_sel]
    want = srt[:n_sel]
    assert (e64[sel].sort().values - want).abs().max().item() <= 4e-6


@pytest.mark.parametrize("n,C", [(64, 1000), (16, 16)])
def test_avg_entropy_saturated(L, dev, n, C):
    """rlcf_avg_entropy on x100 logits (mean of near-one-hot softmaxes) against float64"""
    lg = saturated_logits(n, C)
    out = torch.full((1,), float("nan"), device=dev)
    L.check(L.lib().rlcf_avg_entropy(lg.to(dev).data_ptr(), n, C, out.data_ptr(), st()))
    ref = RR.avg_entropy(lg.double()).item()
    assert abs(out.item() - ref) <= 2e-6 + 1e-5 * abs(ref)
