"""GPU: CoCoOp prompt generation and its TPT step (TPT/clip/cocoop.py, the --cocoop branch of TPT/tpt_cls.py) on the HIP path — the
rlcf_cocoop_ctx kernel against the reference's float64 prompts (tests/golden/cocoop_ops.npz), the fused per-image entry
rlcf_tta_sample_cocoop against the reference's own runs (tests/golden/cocoop_*.npz, tests/golden/make_cocoop_golden.py), its equality
with the two-call composition, the zero-step and mean forms, the refusals, the step skip and the mirror (rlcf_amd.cocoop,
rlcf_amd.tpt_cls)."""
import ctypes as C
import types

import pytest
import torch

from rlcf_amd import synth

import cocoop_ref as CR

pytestmark = pytest.mark.gpu

E2E = ["cocoop_tiny_s0", "cocoop_tiny_s1", "cocoop_small_s1", "cocoop_tinyrn_s1"]
OPS, OPS_META = CR.op_cases()
# max |device - fixture| of the two quantities no other suite of the project bounds, measured on the four end-to-end cases in both
# precisions and written down in profiles/cocoop_notes.md; the bars are 4 x the larger of the two precisions' figures (the margin
# covers the ~22-bit operands of the split-f16 products against the F32 run; nothing else varies between runs)
CTX_GEN_MEASURED = {0: 5.77e-08, 2: 5.59e-08}
FEATURES_MEASURED = {0: 3.58e-06, 2: 3.58e-06}
CTX_GEN_BAR, FEATURES_BAR = 4 * max(CTX_GEN_MEASURED.values()), 4 * max(FEATURES_MEASURED.values())


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


# ------------------------------------------------------------------------------ op level
def _device_feats(name, feats, dev):
    """the case's feature rows on the device; the strided case as rows of a wider matrix (row stride D + 3, the padding poisoned)"""
    if not name.startswith("strided"):
        return feats.to(dev)
    pad = int(OPS_META["strided_pad"])
    wide = torch.full((feats.shape[0], feats.shape[1] + pad), float("nan"), device=dev)
    wide[:, : feats.shape[1]] = feats.to(dev)
    return wide[:, : feats.shape[1]]


def _one_ulp(out, expected):
    """|out - expected| <= 2^-23 |expected| + 1e-30: a double accumulation rounded to float once sits within one float32 ulp"""
    err = (out.cpu().double() - expected).abs()
    bar = 2.0 ** -23 * expected.abs() + 1e-30
    return bool((err <= bar).all()), float((err / bar).max())


@pytest.mark.parametrize("name,shape,x,g", OPS, ids=[c[0] for c in OPS])
def test_cocoop_ctx_op_matches_reference_float64(L, dev, name, shape, x, g):
    from rlcf_amd.engine import cocoop_ctx_op
    D, H, W, n_ctx, n = shape
    feats = _device_feats(name, x["feats"], dev)
    p = [x[k].to(dev) for k in ("ctx", "w1", "b1", "w2", "b2")]
    rows, mean = cocoop_ctx_op(feats, *p), cocoop_ctx_op(feats, *p, mean=True)
    torch.cuda.synchronize()
    assert tuple(rows.shape) == (n, n_ctx, W) and tuple(mean.shape) == (1, n_ctx, W)
    ok_r, worst_r = _one_ulp(rows[g["keep"].to(dev)], g["rows64"])
    ok_m, worst_m = _one_ulp(mean, g["mean64"])
    # (the rows the fixture does not keep are held to the float64 restatement, which the CPU suite holds to the fixture)
    ok_a, worst_a = _one_ulp(rows, torch.from_numpy(CR.meta_net_f64(x)))
    print(f"[{name}] worst |err| / bar: kept rows {worst_r:.3g}  mean form {worst_m:.3g}  all rows vs restatement {worst_a:.3g}")
    assert ok_r and ok_m and ok_a
    rows2, mean2 = cocoop_ctx_op(feats, *p), cocoop_ctx_op(feats, *p, mean=True)
    assert torch.equal(rows, rows2) and torch.equal(mean, mean2)                     # two calls: the same bits
    for r in sorted({0, n // 2, n - 1}):                                             # a row alone: the bits it has inside the batch
        assert torch.equal(cocoop_ctx_op(feats[r: r + 1], *p)[0], rows[r]), r
    if n == 1:
        assert torch.equal(mean, rows)


def test_cocoop_ctx_op_bad_arguments(L, dev):
    lib = L.lib()
    D, H, W, n_ctx, n = 64, 4, 64, 4, 2
    f, ctx = torch.zeros(n, D, device=dev), torch.zeros(n_ctx, W, device=dev)
    w1, b1, w2, b2 = torch.zeros(H, D, device=dev), torch.zeros(H, device=dev), torch.zeros(W, H, device=dev), torch.zeros(W, device=dev)
    out = torch.full((n, n_ctx, W), 7.0, device=dev)
    ptrs = [t.data_ptr() for t in (f, ctx, w1, b1, w2, b2, out)]

    def call(ld=D, n_=n, h=H, d=D, w=W, c=n_ctx, null=None):
        q = [None if i == null else v for i, v in enumerate(ptrs)]
        return lib.rlcf_cocoop_ctx(q[0], ld, n_, 0, q[1], c, q[2], q[3], q[4], q[5], d, h, w, q[6], st())

    assert call() == 0
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0.0
    out.fill_(7.0)
    for kw in (dict(h=0), dict(n_=0), dict(ld=D - 1), dict(d=0), dict(w=0), dict(c=0), dict(n_=70000)) + tuple(dict(null=i) for i in range(7)):
        assert call(**kw) == -1, kw
        assert b"cocoop_ctx" in lib.rlcf_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                        # nothing was launched


# ------------------------------------------------------------------------------ engine calls
def _state(meta, dev):
    s = synth.make_cocoop_state(synth.GEOMETRIES[meta["student"]], meta["cocoop_seed"], meta["n_ctx"])
    return {k: v.to(dev) for k, v in s.items()}


def _engine(L, dev, meta, prec, meta_net=True, view_seed=None, n_views=None):
    from rlcf_amd.engine import Engine
    sg = synth.GEOMETRIES[meta["student"]]
    eng = Engine(sg, None, n_views or meta["n_views"], meta["n_cls"], prec)
    eng.load_state_dict(L.STUDENT, synth.make_state_dict(sg, meta["student_seed"], device=dev))
    eng.finalize()
    state = _state(meta, dev)
    eng.set_class_bank(synth.make_token_bank(sg, meta["n_cls"], seed=meta["bank_seed"], n_ctx=meta["n_ctx"]), meta["n_ctx"], state["ctx"], L.TEXT_SHARED)
    if meta_net:
        eng.set_meta_net(*[state["meta_net." + k] for k in ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias")])
    views = synth.make_views(view_seed or meta["view_seed"], n_views or meta["n_views"], sg.image_resolution, device=dev)
    return eng, state, views


def _cfg(meta, **over):
    from rlcf_amd.engine import TTAConfig
    kw = dict(selection_p=meta["selection_p"], tta_steps=meta["tta_steps"], lr=meta["lr"], weight_decay=meta["weight_decay"], tpt=True)
    kw.update(over)
    return TTAConfig(**kw)


def _check_e2e(o, g, meta, prec):
    """the bars of tests/test_gpu_tpt.py::_check_e2e (lines 143-166, the prompt kind) on the same quantities, the two new quantities at
    the bars above"""
    rn = synth.GEOMETRIES[meta["student"]].is_resnet
    c = lambda k: o[k].cpu()
    d_ctx, d_feat = (c("ctx_gen") - g["ctx_gen"]).abs().max().item(), (c("image_features") - g["image_features"]).abs().max().item()
    print(f"[{meta['student']} steps {meta['tta_steps']} prec {prec}] max|ctx_gen - ref| {d_ctx:.3g} (bar {CTX_GEN_BAR:.3g})  "
          f"max|image_features - ref| {d_feat:.3g} (bar {FEATURES_BAR:.3g})  max|final_logits - ref| {(c('final_logits') - g['final_logits']).abs().max().item():.3g}")
    assert c("top5").tolist() == g["top5"].tolist()                                                   # test_gpu_tpt.py:149
    torch.testing.assert_close(c("final_logits"), g["final_logits"], atol=1e-3, rtol=0)               # test_gpu_tpt.py:154
    assert d_ctx <= CTX_GEN_BAR and d_feat <= FEATURES_BAR                                            # profiles/cocoop_notes.md
    if meta["tta_steps"] == 0:
        assert torch.equal(o["ctx_after"], o["ctx_gen"]) and o["step_skipped"].tolist() == [0] and "loss" not in o
        return
    assert c("selected_idx").tolist() == g["selected_idx"].tolist()                                   # test_gpu_tpt.py:148
    assert not {"topk_idx", "clip_score", "rewards", "reward_image_features"} & set(o)                # test_gpu_tpt.py:150
    torch.testing.assert_close(c("logits"), g["logits"], atol=3e-4 if rn else 1e-3, rtol=0)           # test_gpu_tpt.py:151
    torch.testing.assert_close(c("loss"), g["loss"], rtol=1e-4, atol=1e-4)                            # test_gpu_tpt.py:152
    assert ((c("dlogits") - g["dlogits"]).norm() / g["dlogits"].norm()).item() < 2e-3                 # test_gpu_tpt.py:153
    gr, og = g["ctx_grad"], c("ctx_grad")
    assert (og - gr).norm() / gr.norm() < 1e-3                                                        # test_gpu_tpt.py:159
    differing = (c("ctx_after") - g["ctx_after"]).abs() > 1e-4
    fragile = gr.abs() <= 1e-3 * gr.abs().max()
    assert not (differing & ~fragile).any()                                                           # test_gpu_tpt.py:160-163
    assert o["step_skipped"].tolist() == [0] and not torch.equal(o["ctx_after"], o["ctx_gen"])


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("case", E2E)
def test_cocoop_sample_matches_reference_fixture(L, dev, case, prec):
    """rlcf_tta_sample_cocoop — gen_ctx(aug), the step, the final logits in one call — against the loop body TPT/tpt_cls.py:280-297 run
    by the reference itself"""
    g, meta = CR.load_golden(case)
    eng, state, views = _engine(L, dev, meta, prec)
    o = eng.tta_sample_cocoop(views, _cfg(meta))
    torch.cuda.synchronize()
    _check_e2e(o, g, meta, prec)
    eng.close()


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("case", ["cocoop_tiny_s1", "cocoop_tinyrn_s1"])
def test_cocoop_fused_equals_two_calls_bitwise(L, dev, case, prec):
    """rlcf_tta_sample_cocoop == rlcf_cocoop_gen_ctx + rlcf_tta_sample_feats, bit for bit (the same kernels on the same shapes in the same
    order), in either order of the calls on one engine"""
    g, meta = CR.load_golden(case)
    eng, state, views = _engine(L, dev, meta, prec)
    cfg = _cfg(meta)
    fused = eng.tta_sample_cocoop(views, cfg)
    feats, ctx_gen = eng.cocoop_gen_ctx(views, aug=True)
    two = eng.tta_sample_feats(feats, ctx_gen, cfg)
    again = eng.tta_sample_cocoop(views, cfg)
    torch.cuda.synchronize()
    assert torch.equal(fused["image_features"], feats) and torch.equal(fused["ctx_gen"], ctx_gen)
    for k in ("ctx_after", "final_logits", "top5", "logits", "selected_idx", "loss", "dlogits", "ctx_grad", "step_skipped"):
        assert torch.equal(fused[k], two[k]), k
        assert torch.equal(fused[k], again[k]), k
    # the step entry alone with skip_final (what the mirror's test_time_tuning calls): the same tuned prompt, no final logits
    only = eng.tta_sample_feats(feats, ctx_gen, cfg, want_intermediates=False, skip_final=True)
    assert torch.equal(only["ctx_after"], fused["ctx_after"]) and "final_logits" not in only
    eng.close()


@pytest.mark.parametrize("prec", [0, 2])
def test_cocoop_zero_steps_is_inference_with_the_generated_prompt(L, dev, prec):
    from rlcf_amd.engine import l2norm_rows
    g, meta = CR.load_golden("cocoop_tiny_s0")
    eng, state, views = _engine(L, dev, meta, prec)
    o = eng.tta_sample_cocoop(views, _cfg(meta))
    img0 = l2norm_rows(o["image_features"][:1])
    by_hand = eng.logits(img0, eng.text_features(o["ctx_gen"]))
    plain = eng.logits(img0, eng.text_features(state["ctx"]))
    torch.cuda.synchronize()
    assert torch.equal(o["final_logits"], by_hand)
    assert (by_hand - plain).abs().max().item() >= 0.05          # a build that ignores the meta-net cannot pass the fixture's bar
    eng.close()


@pytest.mark.parametrize("case", ["cocoop_tiny_s1", "cocoop_tinyrn_s1"])
def test_cocoop_gen_ctx_mean_form(L, dev, case):
    """gen_ctx(aug=False) on 3 views: the prompt of the MEAN un-normalised feature — the kernel's mean form on the returned features"""
    from rlcf_amd.engine import cocoop_ctx_op
    g, meta = CR.load_golden(case)
    eng, state, views = _engine(L, dev, meta, 2)
    feats, ctx = eng.cocoop_gen_ctx(views[:3], aug=False)
    p = [state[k] for k in ("ctx", "meta_net.linear1.weight", "meta_net.linear1.bias", "meta_net.linear2.weight", "meta_net.linear2.bias")]
    assert torch.equal(ctx, cocoop_ctx_op(feats, *p, mean=True)[0])
    feats_a, ctx_a = eng.cocoop_gen_ctx(views[:3], aug=True)
    assert torch.equal(feats_a, feats) and torch.equal(ctx_a, cocoop_ctx_op(feats[:1], *p)[0]) and not torch.equal(ctx_a, ctx)
    eng.close()


def test_cocoop_nan_pixel_skips_the_step(L, dev):
    """a NaN pixel in a selected view (a NaN entropy sorts last, so every view is selected here): step_skipped set, the prompt stays the
    generated one (view 0 is clean); the next clean sample is the fixture's"""
    g, meta = CR.load_golden("cocoop_tiny_s1")
    eng, state, views = _engine(L, dev, meta, 2)
    bad = views.clone()
    bad[3, 1, 5, 7] = float("nan")
    o = eng.tta_sample_cocoop(bad, _cfg(meta, selection_p=1.0))
    assert o["step_skipped"].tolist() == [1] and not torch.isfinite(o["loss"]).any()
    assert torch.equal(o["ctx_after"], o["ctx_gen"]) and torch.isfinite(o["ctx_gen"]).all()
    ok = eng.tta_sample_cocoop(views, _cfg(meta))
    assert ok["step_skipped"].tolist() == [0]
    torch.testing.assert_close(ok["final_logits"].cpu(), g["final_logits"], atol=1e-3, rtol=0)
    eng.close()


def test_cocoop_refusals(L, dev):
    g, meta = CR.load_golden("cocoop_tiny_s1")
    lib = L.lib()
    N, D = meta["n_views"], synth.GEOMETRIES[meta["student"]].embed_dim
    out = L.TTAOut()
    feats, ctx = torch.ones(N, D, device=dev), torch.zeros(meta["n_ctx"], 128, device=dev)
    bare, _, views = _engine(L, dev, meta, 2, meta_net=False)
    a = _cfg(meta).c_args(N)
    assert lib.rlcf_cocoop_gen_ctx(bare.h, views.data_ptr(), N, 1, None, None, st()) == -3
    assert b"meta-net" in lib.rlcf_last_error()
    assert lib.rlcf_tta_sample_cocoop(bare.h, views.data_ptr(), N, C.byref(a), C.byref(out), None, None, st()) == -3
    assert b"meta-net" in lib.rlcf_last_error()
    bare.close()
    eng, state, views = _engine(L, dev, meta, 2)
    fused = lambda args: lib.rlcf_tta_sample_cocoop(eng.h, views.data_ptr(), N, C.byref(args), C.byref(out), None, None, st())
    step = lambda args: lib.rlcf_tta_sample_feats(eng.h, feats.data_ptr(), N, C.byref(args), C.byref(out), st())
    two = _cfg(meta, tta_steps=2)
    for fn, args in ((fused, two.c_args(N)), (step, two.c_args(N, ctx_in=ctx))):
        assert fn(args) == -1
        assert b"tpt_cls.py:60" in lib.rlcf_last_error()
    assert fused(_cfg(meta).c_args(N, ctx_in=ctx)) == -1 and b"ctx_in" in lib.rlcf_last_error()
    assert step(_cfg(meta).c_args(N)) == -1 and b"ctx_in" in lib.rlcf_last_error()
    for fn, args in ((fused, _cfg(meta, tpt=False).c_args(N)), (step, _cfg(meta, tpt=False).c_args(N, ctx_in=ctx))):
        assert fn(args) == -1
        assert b"RLCF_F_TPT" in lib.rlcf_last_error()
    for extra in (L.F_KD, L.F_MIN_ENTROPY, 16):
        args = _cfg(meta).c_args(N)
        args.flags |= extra
        assert fused(args) == -1, extra
    assert lib.rlcf_engine_set_meta_net(eng.h, ctx.data_ptr(), ctx.data_ptr(), ctx.data_ptr(), ctx.data_ptr(), 0, st()) == -1
    assert lib.rlcf_engine_set_meta_net(eng.h, None, ctx.data_ptr(), ctx.data_ptr(), ctx.data_ptr(), 8, st()) == -1
    o = eng.tta_sample_cocoop(views, _cfg(meta))                                     # the refusals leave the engine working
    torch.cuda.synchronize()
    _check_e2e(o, g, meta, 2)
    eng.close()


# ------------------------------------------------------------------------------ the mirror
def _mirror(meta, dev):
    from rlcf_amd import clip_store, cocoop, runtime
    runtime.reset_session()
    runtime.SESSION.max_views = meta["n_views"]
    sg = synth.GEOMETRIES[meta["student"]]
    clip_store.register_checkpoint(meta["student"], sg, synth.make_state_dict(sg, meta["student_seed"]))
    bank = clip_store.SyntheticBank(sg, meta["n_cls"], meta["n_ctx"], meta["bank_seed"])
    clip_store.set_tokenizer(bank.tokenize)
    model = cocoop.get_cocoop(meta["student"], "I", "cpu", meta["n_ctx"])
    cocoop.load_cocoop_weights({"state_dict": synth.make_cocoop_state(sg, meta["cocoop_seed"], meta["n_ctx"]), "epoch": 0}, model)
    for name, p in model.named_parameters():                     # TPT/tpt_cls.py:116-121
        if "text_encoder" not in name:
            p.requires_grad_(False)
    model = model.cuda(0)
    model.prompt_generator.reset_classnames(bank.classnames, meta["student"])          # tpt_cls.py:198-199
    return model, sg


def _mirror_args(meta, **kw):
    return types.SimpleNamespace(tta_steps=meta["tta_steps"], selection_p=meta["selection_p"], lr=meta["lr"], gpu=0, tpt=True, print_freq=1000,
                                 cocoop=True, **kw)


def test_tpt_cls_cocoop_eval_loop_matches_reference(L, dev, monkeypatch):
    """get_cocoop + load_cocoop_weights + tpt_cls.test_time_adapt_eval (TPT/tpt_cls.py:242-314 with --cocoop) through the mirror: the
    per-sample final logits and top-5 of cocoop_eval_tiny and the hit percentages"""
    from rlcf_amd import engine, runtime, tpt_cls
    g, meta = CR.load_golden("cocoop_eval_tiny")
    model, sg = _mirror(meta, dev)
    n = meta["n_samples"]
    loader = []
    for i in range(n):
        views = synth.make_views(int(g["view_seeds"][i]), meta["n_views"], sg.image_resolution)
        target = int(g["top5"][i, 0]) if i % 2 == 0 else int(g["top5"][i, 4])
        loader.append(([views[j: j + 1] for j in range(meta["n_views"])], torch.tensor([target])))
    seen = []
    fused = engine.Engine.tta_sample_cocoop

    def record(self, views, cfg, want_intermediates=True):
        o = fused(self, views, cfg, want_intermediates)
        seen.append(o)
        return o

    monkeypatch.setattr(engine.Engine, "tta_sample_cocoop", record)
    top1, top5 = tpt_cls.test_time_adapt_eval(loader, model, None, None, None, None, _mirror_args(meta))
    assert len(seen) == n and not runtime.SESSION.rewards
    for i, o in enumerate(seen):
        assert o["top5"].cpu().tolist() == g["top5"][i].tolist()
        torch.testing.assert_close(o["final_logits"][0].cpu(), g["final_logits"][i], atol=1e-3, rtol=0)
    assert abs(top1 - 100.0 * ((n + 1) // 2) / n) < 1e-2 and abs(top5 - 100.0) < 1e-2
    runtime.reset_session()


def test_reference_shaped_step_through_the_mirror(L, dev):
    """what the reference's own test_time_tuning does after an import swap (TPT/tpt_cls.py:49-78): gen_ctx, model((features, ctx)) with
    ctx requiring grad, selection, avg_entropy(...).backward() — the ctx_grad bar of tests/test_gpu_tpt.py:159 against cocoop_tiny_s1;
    and the mirror's own test_time_tuning / final call against ctx_after / final_logits"""
    from rlcf_amd import runtime, tpt_cls
    g, meta = CR.load_golden("cocoop_tiny_s1")
    model, sg = _mirror(meta, dev)
    views = synth.make_views(meta["view_seed"], meta["n_views"], sg.image_resolution).to(dev)
    feats, pgen_ctx = model.gen_ctx(views, True)
    assert tuple(pgen_ctx.shape) == (1, meta["n_ctx"], sg.transformer_width) and not pgen_ctx.requires_grad
    torch.testing.assert_close(pgen_ctx[0].cpu(), g["ctx_gen"], atol=CTX_GEN_BAR, rtol=0)
    ctx = pgen_ctx.clone().requires_grad_(True)
    output = model((feats, ctx))
    torch.testing.assert_close(output.detach().cpu(), g["logits"], atol=1e-3, rtol=0)
    sel, idx = tpt_cls.select_confident_samples(output, meta["selection_p"])
    assert idx.cpu().tolist() == g["selected_idx"].tolist()
    loss = tpt_cls.avg_entropy(sel)
    loss.backward()
    torch.testing.assert_close(loss.detach().cpu().reshape(1), g["loss"], rtol=1e-4, atol=1e-4)
    assert ((ctx.grad[0].cpu() - g["ctx_grad"]).norm() / g["ctx_grad"].norm()).item() < 1e-3           # tests/test_gpu_tpt.py:159
    tuned = tpt_cls.test_time_tuning(model, (feats, pgen_ctx), None, None, _mirror_args(meta))
    assert tuned.shape == pgen_ctx.shape
    differing = (tuned[0].cpu() - g["ctx_after"]).abs() > 1e-4
    assert not (differing & ~(g["ctx_grad"].abs() <= 1e-3 * g["ctx_grad"].abs().max())).any()           # tests/test_gpu_tpt.py:160-163
    with torch.no_grad():
        final = model((feats[0:1], tuned))
    torch.testing.assert_close(final.cpu(), g["final_logits"], atol=1e-3, rtol=0)
    # inference(images): every image under the prompt generated from its own normalised features (cocoop.py:153-170)
    with torch.no_grad():
        per_image = model(views[:2])
    assert tuple(per_image.shape) == (2, meta["n_cls"]) and torch.isfinite(per_image).all()
    runtime.reset_session()
