"""GPU: zero-shot evaluation and the ensemble classifier (TPT/zero_shot.py, CLIPCLS_TTA_Multiple of TPT/clip/custom_clip.py) on the HIP
path — the rlcf_ensemble_logits kernel against the reference expression in float64 (tests/golden/zeroshot_ops.npz), the engine entry
rlcf_zero_shot_batch against the reference's own classes (tests/golden/zeroshot_*.npz, tests/golden/make_zeroshot_golden.py), its
equality with the call-by-call composition, the accumulating hit counts, the refusals, its leaving the tuning calls alone, and the mirrors
(rlcf_amd.custom_clip.CLIPCLS_TTA_Multiple, rlcf_amd.zero_shot)."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from rlcf_amd import synth

import zeroshot_ref as ZR

pytestmark = pytest.mark.gpu

OPS, OPS_META = ZR.op_cases()
TUPLES = ["zeroshot_tiny", "zeroshot_tinyrn", "zeroshot_ens2", "zeroshot_ens3res", "zeroshot_ens_student_res"]
LOGIT_BAR = ZR.LOGIT_BAR
FEAT_ATOL, FEAT_RTOL = 5e-6, 1e-4      # the bar of tests/test_gpu_parity.py::test_encode_image_vs_oracle on rlcf_encode_image


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
def _padded(x, pad, dev):
    """rows of a wider matrix (row stride width + pad, the padding poisoned)"""
    if not pad:
        return x.to(dev)
    wide = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=dev)
    wide[:, : x.shape[1]] = x.to(dev)
    return wide[:, : x.shape[1]]


def _one_ulp(out, expected):
    """|out - float32(expected)| <= one float32 ulp of it: a double accumulation rounded to float once lands ON float32(expected)
    unless the double sum and the float64 reference straddle a rounding boundary, then one ulp away"""
    e32 = torch.from_numpy(np.asarray(expected, dtype=np.float64).astype(np.float32))
    ulp = torch.from_numpy(np.spacing(np.abs(e32.numpy())))
    err = (out.cpu().double() - e32.double()).abs()
    return bool((err <= ulp.double()).all()), float((err / ulp.double()).max())


def _top5_device(L, logits):
    n, Cn = logits.shape
    lg = logits.contiguous()
    t5 = torch.full((n, 5), -1, dtype=torch.int32, device=logits.device)
    tg = torch.zeros(n, dtype=torch.int64, device=logits.device)
    res = torch.zeros(2, device=logits.device)
    L.check(L.lib().rlcf_accuracy(lg.data_ptr(), tg.data_ptr(), n, Cn, t5.data_ptr(), res.data_ptr(), st()), "accuracy")      # top5_kernel, one block per row
    return t5.cpu()[:, : min(5, Cn)].to(torch.int64).numpy()


@pytest.mark.parametrize("name,shape,g", OPS, ids=[c[0] for c in OPS])
def test_ensemble_logits_matches_reference_float64(L, dev, name, shape, g):
    from rlcf_amd.engine import ensemble_logits
    widths, n, Cn = shape
    imgs, txts, scales = ZR.op_inputs(widths, n, Cn, int(g["seed"]), tie=name.startswith("tie"))
    strided = name.startswith("strided")
    pad, lpad = (int(OPS_META["strided_pad"]), int(OPS_META["logits_pad"])) if strided else (0, 0)
    di, dt = [_padded(a, pad, dev) for a in imgs], [_padded(t, pad, dev) for t in txts]

    def run(rows=slice(None)):
        ii = [a[rows] for a in di]
        out = torch.full((ii[0].shape[0], Cn + lpad), 7.0, device=dev)
        ensemble_logits(ii, dt, scales, out=out[:, :Cn])
        return out

    full = run()
    torch.cuda.synchronize()
    out = full[:, :Cn]
    assert (full[:, Cn:] == 7.0).all()                                               # nothing written past a row's C entries
    ok_k, worst_k = _one_ulp(out[g["keep"].to(dev)], g["logits64"].numpy())
    # (the rows the fixture does not keep are held to the float64 restatement, which the CPU suite holds to the fixture)
    mix = ZR.mix_f64(imgs, txts, scales)
    ok_a, worst_a = _one_ulp(out, mix)
    print(f"[{name}] worst |err| in ulps: kept rows vs fixture {worst_k:.3g}  all rows vs restatement {worst_a:.3g}")
    assert ok_k and ok_a
    # top-5 of the device logits by the engine's top-5 kernel: the restatement's on the float64 values, ties to the lower index
    assert np.array_equal(_top5_device(L, out), ZR.top5(mix))
    if name.startswith("tie"):
        assert torch.equal(out[:, 2], out[:, 5]) and _top5_device(L, out)[:, :2].tolist() == [[2, 5]] * n
    assert torch.equal(run(), full)                                                  # two calls: the same bits
    for r in sorted({0, n // 2, n - 1}):                                             # a row alone: the bits it has inside the batch
        assert torch.equal(run(slice(r, r + 1))[0, :Cn], out[r]), r


def test_ensemble_logits_bad_arguments(L, dev):
    lib = L.lib()
    n, Cn, D = 3, 7, 64
    img, txt = torch.zeros(n, D + 4, device=dev), torch.zeros(Cn, D + 4, device=dev)
    out = torch.full((n, Cn), 7.0, device=dev)

    def call(M=1, n_=n, c=Cn, ld=Cn, d=D, ldi=D + 4, ldt=D + 4, img_p=None, txt_p=None, out_p=out.data_ptr(), null_desc=False):
        desc = L.EnsDesc()
        desc.M = M
        for m in range(min(max(M, 0), L.ENS_MAX_MODELS)):
            desc.m[m] = L.EnsModel(img.data_ptr() if img_p is None else img_p, ldi, txt.data_ptr() if txt_p is None else txt_p, ldt, d, 1.0)
        return lib.rlcf_ensemble_logits(None if null_desc else C.byref(desc), n_, c, out_p, ld, st())

    assert call() == 0
    torch.cuda.synchronize()
    assert out.abs().max().item() == 0.0
    out.fill_(7.0)
    bad = (dict(M=0), dict(M=6), dict(n_=0), dict(c=0), dict(d=0), dict(d=2), dict(d=6), dict(ldi=D - 4, d=D), dict(ldi=D + 2), dict(ldt=D - 4),
           dict(ldt=D + 1), dict(ld=Cn - 1), dict(img_p=0), dict(txt_p=0), dict(out_p=None), dict(null_desc=True), dict(img_p=img.data_ptr() + 4),
           dict(n_=16 * 65535 + 1))
    for kw in bad:
        assert call(**kw) == -1, kw
        assert b"ensemble_logits" in lib.rlcf_last_error(), kw
    torch.cuda.synchronize()
    assert (out == 7.0).all()                                                        # nothing was launched


# ------------------------------------------------------------------------------ the engine entry
def _engine(L, dev, meta, prec, max_views=None):
    from rlcf_amd.engine import Engine
    archs, seeds = meta["archs"].split(","), [int(s) for s in meta["model_seeds"].split(",")]
    geos = [synth.GEOMETRIES[a] for a in archs]
    sds = [synth.make_state_dict(g, s, device=dev) for g, s in zip(geos, seeds)]
    n_cls = int(meta["n_cls"])
    eng = Engine(geos[0], geos[1:] or None, max_views or int(meta["n_img"]), n_cls, prec)
    for w, sd in enumerate(sds):
        eng.load_state_dict(w, sd)
    eng.finalize()
    tokens = synth.make_token_bank(geos[0], n_cls, seed=int(meta["bank_seed"]), n_ctx=4)
    # as the mirrors publish it: one "learnable" row, the first prompt token's embedding
    ctx = sds[0]["token_embedding.weight"][tokens[0][1:2].to(dev)].clone()
    eng.set_class_bank(tokens, 1, ctx, L.TEXT_SHARED)
    return eng, geos, ctx


def _images(meta, dev, n=None):
    return synth.make_views(int(meta["image_seed"]), n or int(meta["n_img"]), int(meta["in_res"]), device=dev)


def _compose(eng, geos, ctx, images):
    """the call by call composition: a tower pass per model, the class features, rlcf_ensemble_logits"""
    feats = [eng.encode_image(w, images) for w in range(len(geos))]
    cls = [eng.text_features(ctx)] + [eng.reward_class_features(m) for m in range(len(geos) - 1)]
    return feats, cls, eng.ensemble_logits(feats, cls)


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("case", TUPLES)
def test_zero_shot_batch_matches_reference_and_composition(L, dev, case, prec):
    """rlcf_zero_shot_batch on five images against the reference's CLIPCLS_TTA / CLIPCLS_TTA_Multiple forward: logits within LOGIT_BAR,
    top-5 identical, the per-model image features within the module bar — and bit for bit the composition rlcf_encode_image(_resized)
    per model, rlcf_text_features / rlcf_reward_class_features, rlcf_ensemble_logits"""
    g, meta = ZR.load_golden(case)
    eng, geos, ctx = _engine(L, dev, meta, prec)
    images = _images(meta, dev)
    ens = len(geos) > 1
    o = eng.zero_shot_batch(images, ensemble=ens)
    feats, cls, logits = _compose(eng, geos, ctx, images)
    again = eng.zero_shot_batch(images, ensemble=ens)
    torch.cuda.synchronize()
    d = (o["logits"].cpu() - g["logits"]).abs().max().item()
    print(f"[{case} prec {prec}] max|logits - ref| {d:.3g} (bar {LOGIT_BAR:g})  " +
          "  ".join(f"max|feat{m} - ref| {(f.cpu() - g[f'feat{m}']).abs().max().item():.3g}" for m, f in enumerate(feats)))
    assert d <= LOGIT_BAR
    assert o["top5"].cpu().tolist() == g["top5"].tolist()
    for m, (f, c) in enumerate(zip(feats, cls)):
        torch.testing.assert_close(f.cpu(), g[f"feat{m}"], atol=FEAT_ATOL, rtol=FEAT_RTOL)
        torch.testing.assert_close(c.cpu(), g[f"cls{m}"], atol=FEAT_ATOL, rtol=FEAT_RTOL)
    assert torch.equal(o["logits"], logits) and torch.equal(again["logits"], logits) and torch.equal(again["top5"], o["top5"])
    if ens:            # the student alone on the same engine: its own logits, not the mix
        alone = eng.zero_shot_batch(images, ensemble=False)["logits"]
        assert torch.equal(alone, eng.ensemble_logits(feats[:1], cls[:1])) and not torch.equal(alone, logits)
    eng.close()


def test_zero_shot_batch_f16_runs_and_is_finite(L, dev):
    g, meta = ZR.load_golden("zeroshot_ens2")
    eng, geos, ctx = _engine(L, dev, meta, L.PREC_F16)
    o = eng.zero_shot_batch(_images(meta, dev), ensemble=True)
    torch.cuda.synchronize()
    assert torch.isfinite(o["logits"]).all() and tuple(o["logits"].shape) == (5, 16) and tuple(o["top5"].shape) == (5, 5)
    eng.close()


@pytest.mark.parametrize("tag", ["single", "ens2"])
def test_zero_shot_hits_accumulate_over_batches(L, dev, tag):
    """three calls (4 + 4 + 3 images) on one float[2]: the fixture's hit counts; target = NULL leaves the counts untouched"""
    g, meta = ZR.load_golden("zeroshot_eval_tiny")
    m = dict(meta, archs=meta["archs_" + tag], image_seed=int(g["image_seed"]))
    eng, geos, ctx = _engine(L, dev, m, 2, max_views=4)
    images, targets = _images(m, dev), g["targets"].to(dev)
    hits = torch.zeros(2, device=dev)
    top5 = []
    for i in range(0, int(meta["n_img"]), int(meta["batch"])):
        o = eng.zero_shot_batch(images[i: i + 4], ensemble=tag == "ens2", target=targets[i: i + 4], hits=hits, want_logits=False)
        top5.append(o["top5"])
    before = hits.clone()
    eng.zero_shot_batch(images[:4], ensemble=tag == "ens2")            # no target: the counts stay
    torch.cuda.synchronize()
    assert torch.cat(top5).cpu().tolist() == g[f"top5_{tag}"].tolist()
    assert hits.cpu().tolist() == [float(x) for x in g[f"hits_{tag}"].tolist()] and torch.equal(hits, before)
    eng.close()


def test_zero_shot_batch_refusals(L, dev):
    g, meta = ZR.load_golden("zeroshot_tiny")
    lib = L.lib()
    eng, geos, ctx = _engine(L, dev, meta, 0)
    images = _images(meta, dev)
    n, Cn = images.shape[0], int(meta["n_cls"])
    logits = torch.full((n + 1, Cn), 7.0, device=dev)
    target, hits = torch.zeros(n + 1, dtype=torch.int64, device=dev), torch.full((2,), 3.0, device=dev)

    def call(e=eng, n_=n, res=32, ens=0, tg=None, ht=None, im=images.data_ptr()):
        return lib.rlcf_zero_shot_batch(e.h, im, n_, res, ens, tg, logits.data_ptr(), None, ht, st())

    assert call() == 0 and call(tg=target.data_ptr(), ht=hits.data_ptr()) == 0
    torch.cuda.synchronize()
    assert (logits[:n] != 7.0).all() and float(hits.sum()) >= 6.0
    logits.fill_(7.0)
    hits.fill_(3.0)
    for kw in (dict(n_=n + 1), dict(n_=0), dict(res=0), dict(tg=target.data_ptr()), dict(ht=hits.data_ptr()), dict(im=None)):
        assert call(**kw) == -1, kw                                                  # RLCF_ERR_ARG
    assert call(ens=1) == -3 and b"without a further model" in lib.rlcf_last_error()         # RLCF_ERR_STATE
    assert call(ens=1, n_=n + 1) == -1                                               # the argument rules come before the state rules
    from rlcf_amd.engine import Engine
    bare = Engine(geos[0], None, n, Cn, 0)                                           # no class bank
    bare.load_state_dict(L.STUDENT, synth.make_state_dict(geos[0], 11, device=dev))
    bare.finalize()
    assert call(e=bare) == -3 and b"class bank" in lib.rlcf_last_error()
    torch.cuda.synchronize()
    assert (logits == 7.0).all() and (hits == 3.0).all()                             # nothing was launched
    bare.close()
    eng.close()


def test_tta_sample_ln_is_untouched_by_a_zero_shot_batch(L, dev):
    """rlcf_tta_sample_ln between two of whose calls a rlcf_zero_shot_batch ran gives the bits it gives without it (the inputs of the
    ln_tiny_s1 fixture: tiny student, tiny-r reward model, 8 views, 16 classes)"""
    from rlcf_amd.engine import Engine, TTAConfig
    g, meta = ZR.load_golden("ln_tiny_s1")
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    ssd = synth.make_state_dict(sg, meta["student_seed"], device=dev)
    eng = Engine(sg, rg, meta["n_views"], meta["n_cls"], 2)
    eng.load_state_dict(L.STUDENT, ssd)
    eng.load_state_dict(L.REWARD, synth.make_state_dict(rg, meta["reward_seed"], device=dev))
    eng.finalize()
    tokens = synth.make_token_bank(sg, meta["n_cls"], seed=meta["bank_seed"], n_ctx=meta["n_ctx"])
    ctx0 = ssd["token_embedding.weight"][torch.tensor(synth.ctx_token_ids_default(sg, meta["n_ctx"]), device=dev)].clone()
    eng.set_class_bank(tokens, meta["n_ctx"], ctx0, L.TEXT_SHARED)
    views = synth.make_views(meta["view_seed"], meta["n_views"], sg.image_resolution, device=dev)
    cfg = TTAConfig(selection_p=meta["selection_p"], tta_steps=meta["tta_steps"], sample_k=meta["sample_k"], lr=meta["lr"], weight_decay=meta["weight_decay"])
    eng.tta_sample_ln(views, cfg)
    without = {k: v.clone() for k, v in eng.tta_sample_ln(views, cfg).items()}
    other = synth.make_views(77, meta["n_views"], sg.image_resolution, device=dev)
    for ens in (False, True):
        z = eng.zero_shot_batch(other, ensemble=ens, target=torch.zeros(meta["n_views"], dtype=torch.int64, device=dev), hits=torch.zeros(2, device=dev))
        assert torch.isfinite(z["logits"]).all()
        after = eng.tta_sample_ln(views, cfg)
        torch.cuda.synchronize()
        assert without.keys() == after.keys()
        for k in without:
            assert isinstance(without[k], torch.Tensor) and torch.equal(without[k], after[k]), (ens, k)
    eng.close()


# ------------------------------------------------------------------------------ the mirrors
def _mirror(meta, dev, n_img=None):
    from rlcf_amd import clip_store, custom_clip, runtime
    runtime.reset_session()
    runtime.SESSION.max_views = n_img or int(meta["n_img"])
    archs = meta["archs"].split(",")
    for a, s in zip(archs, meta["model_seeds"].split(",")):
        clip_store.register_checkpoint(a, synth.GEOMETRIES[a], synth.make_state_dict(synth.GEOMETRIES[a], int(s)))
    bank = clip_store.SyntheticBank(synth.GEOMETRIES[archs[0]], int(meta["n_cls"]), 4, int(meta["bank_seed"]))
    clip_store.set_tokenizer(bank.tokenize)
    if int(meta.get("default_resolutions", 0)):
        return custom_clip.CLIPCLS_TTA_Multiple("cpu", bank.classnames, arch=archs, prompt_prefix=meta["prefix"], default_resolutions=int(meta["default_resolutions"])), bank
    return custom_clip.CLIPCLS_TTA("cpu", bank.classnames, arch=archs[0], prompt_prefix=meta["prefix"]), bank


@pytest.mark.parametrize("case", ["zeroshot_ens2", "zeroshot_ens3res", "zeroshot_ens_student_res"])
def test_multiple_mirror_matches_reference(L, dev, case):
    """CLIPCLS_TTA_Multiple.forward, .class_features, .extract_image_features against the reference's; reset_classnames_and_state with
    a second class list (ens2)"""
    from rlcf_amd import runtime
    g, meta = ZR.load_golden(case)
    model, bank = _mirror(meta, dev)
    archs = meta["archs"].split(",")
    assert model.n_model == len(archs) and model.resolutions == [synth.GEOMETRIES[a].image_resolution for a in archs]
    assert model.default_resolutions == int(meta["default_resolutions"]) and torch.equal(model.tokenized_prompts.cpu(), bank.tokens)
    assert len(runtime.SESSION.rewards) == len(archs) - 1 and runtime.SESSION.reward_mix is None
    images = _images(meta, dev)
    logits = model(images)
    feats, cls = model.extract_image_features(images), model.class_features
    torch.cuda.synchronize()
    torch.testing.assert_close(logits.cpu(), g["logits"], atol=LOGIT_BAR, rtol=0)
    assert ZR.top5(logits.cpu().numpy()).tolist() == g["top5"].tolist()
    for m in range(len(archs)):
        torch.testing.assert_close(feats[m].cpu(), g[f"feat{m}"], atol=FEAT_ATOL, rtol=FEAT_RTOL)
        torch.testing.assert_close(cls[m].cpu(), g[f"cls{m}"], atol=FEAT_ATOL, rtol=FEAT_RTOL)
    assert all(torch.equal(a, b) for a, b in zip(model.get_class_features(model.tokenized_prompts), cls))
    model.freeze_parameters(), model.reset(), model.momentum_update_model()
    if case == "zeroshot_ens2":
        names2 = [f"c{i}" for i in meta["classes_reset"].split(",")]
        model.reset_classnames_and_state(names2, archs)
        logits2 = model(images)
        torch.cuda.synchronize()
        assert model.n_cls == len(names2) and model.classnames == names2
        torch.testing.assert_close(logits2.cpu(), g["logits_reset"], atol=LOGIT_BAR, rtol=0)
        assert ZR.top5(logits2.cpu().numpy()).tolist() == g["top5_reset"].tolist()
        for m, c in enumerate(model.class_features):
            torch.testing.assert_close(c.cpu(), g[f"cls{m}_reset"], atol=FEAT_ATOL, rtol=FEAT_RTOL)
    runtime.reset_session()


@pytest.mark.parametrize("tag", ["single", "ens2"])
def test_eval_loop_through_the_mirror(L, dev, tag, monkeypatch):
    """zero_shot.test_time_adapt_eval over a list loader of the 11 images (4 + 4 + 3): the reference's [acc1, acc5], one fused engine
    call per batch and exactly one device-to-host read"""
    from rlcf_amd import engine, runtime, zero_shot
    g, meta = ZR.load_golden("zeroshot_eval_tiny")
    m = dict(meta, archs=meta["archs_" + tag], default_resolutions=32 if tag == "ens2" else 0)
    model, bank = _mirror(m, dev, n_img=4)
    images = synth.make_views(int(g["image_seed"]), int(meta["n_img"]), int(meta["in_res"]))
    b = int(meta["batch"])
    loader = [([images[i: i + b].clone(), images[i: i + b].flip(0)], g["targets"][i: i + b].clone()) for i in range(0, images.shape[0], b)]
    runtime.SESSION.engine(b)                                    # (built before the reads are counted: loading weights is not the loop's)
    calls, reads = [], []
    fused, cpu, item, tolist = engine.Engine.zero_shot_batch, torch.Tensor.cpu, torch.Tensor.item, torch.Tensor.tolist
    monkeypatch.setattr(engine.Engine, "zero_shot_batch", lambda self, im, **kw: (calls.append(im.shape[0]), fused(self, im, **kw))[1])
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: (reads.append("cpu") if self.is_cuda else None, cpu(self, *a, **k))[1])
    monkeypatch.setattr(torch.Tensor, "item", lambda self: (reads.append("item") if self.is_cuda else None, item(self))[1])
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.append("tolist") if self.is_cuda else None, tolist(self))[1])
    acc = zero_shot.test_time_adapt_eval(loader, model, None, None, None, types.SimpleNamespace(gpu=0, print_freq=1000))
    monkeypatch.undo()
    assert calls == [4, 4, 3] and reads == ["cpu"]
    assert acc == g[f"acc_{tag}"].tolist()
    runtime.reset_session()
