"""GPU: the TPT entropy-minimisation baseline (TPT/tpt_cls.py, TPT/tune_cls_tpt.py) on the HIP path — the rlcf_tpt_loss kernel against
the reference's float64 avg_entropy and gradient (tests/golden/tpt_ops.npz), the engine's prompt / LayerNorm / every-parameter /
ResNet tuning calls with RLCF_F_TPT against the reference's own runs (tests/golden/tpt_*.npz, tests/golden/make_tpt_golden.py), an
engine built without a reward model, the batched calls, the refusals, the step skip and the two mirrors."""
import copy
import ctypes as C
import types

import pytest
import torch

from oracle import rlcf_ref as RR
from rlcf_amd import synth

import tpt_ref as T

pytestmark = pytest.mark.gpu

E2E = ["tpt_tiny_s1", "tpt_tiny_s3", "tpt_tiny_ln_s1", "tpt_tiny_ln_s3", "tpt_tiny_vis_s1", "tpt_tiny_rn_s1"]
OPS, OPS_META = T.op_cases()
REWARD, REWARD_SEED = "tiny-r", 23


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
def _device_rows(name, x, dev):
    """the case's rows on the device; the strided case as rows of a wider matrix (row stride C + 3, the padding poisoned)"""
    if not name.startswith("strided"):
        return x.to(dev)
    pad = int(OPS_META["strided_pad"])
    wide = torch.full((x.shape[0], x.shape[1] + pad), float("nan"), device=dev)
    wide[:, : x.shape[1]] = x.to(dev)
    return wide[:, : x.shape[1]]


@pytest.mark.parametrize("name,x,groups,g", OPS, ids=[c[0] for c in OPS])
def test_tpt_loss_op_matches_reference_float64(L, dev, name, x, groups, g):
    """per case max|kernel - f64| <= max|ref32 - f64| + 2^-23 max|f64| for the loss and for dlogits (never worse than the reference's
    own float32 result, plus one rounding); every dlogits row sums to zero to the same allowance; two calls are bit-identical; a
    grouped call equals the per-group calls bit for bit"""
    from rlcf_amd.engine import tpt_loss_op
    rows = _device_rows(name, x, dev)
    loss, dlog = tpt_loss_op(rows, groups)
    torch.cuda.synchronize()
    l_err = (loss.cpu().double() - g["loss64"].reshape(groups)).abs().max().item()
    d_err = (dlog.cpu().double() - g["dlog64"]).abs().max().item()
    s_err = dlog.cpu().double().sum(dim=1).abs().max().item()
    l_bar, d_bar = T.allowance(g["loss"], g["loss64"]), T.allowance(g["dlog"], g["dlog64"])
    print(f"[{name}] loss err {l_err:.3g} (bar {l_bar:.3g})  dlogits err {d_err:.3g} (bar {d_bar:.3g})  row sums {s_err:.3g}")
    assert l_err <= l_bar and d_err <= d_bar and s_err <= d_bar
    if x.shape[1] == 1:
        assert loss.abs().max().item() == 0.0 and dlog.abs().max().item() == 0.0
    loss2, dlog2 = tpt_loss_op(rows, groups)
    assert torch.equal(loss, loss2) and torch.equal(dlog, dlog2)
    n = x.shape[0] // groups
    for i in range(groups):
        li, di = tpt_loss_op(rows[i * n: (i + 1) * n], 1)
        assert torch.equal(li[0], loss[i]) and torch.equal(di, dlog[i * n: (i + 1) * n])
    only_loss, none = tpt_loss_op(rows, groups, want_dlogits=False)
    assert none is None and torch.equal(only_loss, loss)


def test_tpt_loss_op_nonfinite_rows_and_bad_arguments(L, dev):
    from rlcf_amd.engine import tpt_loss_op
    x = dict((c[0], c[1]) for c in OPS)["g3_n6_c200"].clone()
    for bad in (float("nan"), float("inf")):
        y = x.clone()
        y[7, 11] = bad                                    # a row of group 1
        loss, dlog = tpt_loss_op(y.to(dev), 3)
        fin_l, fin_d = torch.isfinite(loss).cpu(), torch.isfinite(dlog).cpu()
        assert fin_l.tolist() == [True, False, True]
        assert not fin_d[6:12].any() and fin_d[:6].all() and fin_d[12:].all()
    lib = L.lib()
    s = torch.zeros(4, 8, device=dev)
    out, d = torch.empty(2, device=dev), torch.empty(4, 8, device=dev)
    call = lambda ld, groups, n, c: lib.rlcf_tpt_loss(s.data_ptr(), ld, groups, n, c, out.data_ptr(), d.data_ptr(), None, st())
    assert call(8, 2, 2, 8) == 0
    for a in ((8, 0, 2, 8), (8, 2, 0, 8), (8, 2, 2, 0), (7, 2, 2, 8), (8, 1, 1, L.KD_MAX_CLASSES + 1)):
        assert call(*a) == -1, a
        assert lib.rlcf_last_error()
    assert lib.rlcf_tpt_loss(s.data_ptr(), 8, 2, 2, 8, None, None, None, st()) == -1
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ engine calls
def _engine(L, dev, meta, prec, reward=True, max_views=None, n_cls=None):
    from rlcf_amd.engine import Engine
    sg = synth.GEOMETRIES[meta["student"]]
    ssd = synth.make_state_dict(sg, meta["student_seed"], device=dev)
    n_cls = n_cls or meta["n_cls"]
    eng = Engine(sg, synth.GEOMETRIES[REWARD] if reward else None, max_views or meta["n_views"], n_cls, prec)
    eng.load_state_dict(L.STUDENT, ssd)
    if reward:
        eng.load_state_dict(L.REWARD, synth.make_state_dict(synth.GEOMETRIES[REWARD], REWARD_SEED, device=dev))
    eng.finalize()
    tokens = synth.make_token_bank(sg, n_cls, seed=meta["bank_seed"], n_ctx=meta["n_ctx"])
    ctx0 = ssd["token_embedding.weight"][torch.tensor(synth.ctx_token_ids_default(sg, meta["n_ctx"]), device=dev)].clone()
    eng.set_class_bank(tokens, meta["n_ctx"], ctx0, L.TEXT_SHARED)
    views = synth.make_views(meta["view_seed"], meta["n_views"], sg.image_resolution, device=dev)
    return eng, ssd, views


def _cfg(meta, tpt=True, **over):
    from rlcf_amd.engine import TTAConfig
    kw = dict(selection_p=meta["selection_p"], tta_steps=meta["tta_steps"], lr=meta["lr"], weight_decay=meta["weight_decay"], tpt=tpt)
    kw.update(over)
    return TTAConfig(**kw)


def _call(eng, meta):
    return {"prompt": eng.tta_sample, "ln": eng.tta_sample_ln, "vis": eng.tta_sample_visual}[meta["kind"]]


def _tensor_norms(sd, keys, vec, base=None):
    out, off = [], 0
    for k in keys:
        n = sd[k].numel()
        v = vec[off: off + n].double()
        if base is not None:
            v = v - base[k].reshape(-1).double().to(v.device)
        out.append(v.norm())
        off += n
    assert off == vec.numel()
    return torch.stack(out).float().cpu()


def _check_e2e(eng, o, g, meta, ssd):
    """the bars tests/test_gpu_kd.py (_check_e2e, lines 189-241) and tests/test_gpu_parity.py (_check_against, lines 390-420) apply to
    the same quantity on the same tiny geometry"""
    rn = synth.GEOMETRIES[meta["student"]].is_resnet
    c = lambda k: o[k].cpu()
    assert c("selected_idx").tolist() == g["selected_idx"].tolist()
    assert c("top5").tolist()[: g["top5"].numel()] == g["top5"].tolist()
    assert not {"topk_idx", "clip_score", "rewards", "reward_image_features"} & set(o)      # no sampled classes, no reward pass
    torch.testing.assert_close(c("logits"), g["logits"], atol=3e-4 if rn else 1e-3, rtol=0)      # test_gpu_kd.py:198, test_gpu_parity.py:395
    torch.testing.assert_close(c("loss"), g["loss"], rtol=1e-4, atol=1e-4)                       # test_gpu_kd.py:204
    assert ((c("dlogits") - g["dlogits"]).norm() / g["dlogits"].norm()).item() < 2e-3            # test_gpu_kd.py:210
    torch.testing.assert_close(c("final_logits"), g["final_logits"], atol=1e-3, rtol=0)          # test_gpu_kd.py:212, test_gpu_parity.py:399
    multi = meta["tta_steps"] > 1
    if meta["kind"] == "prompt":
        d = (c("ctx_after") - g["ctx_after"]).abs()
        gr, og = g["ctx_grad"], c("ctx_grad")
        assert (og - gr).norm() / gr.norm() < 1e-3                                               # test_gpu_parity.py:405
        differing = d > 1e-4
        if not multi:
            fragile = gr.abs() <= 1e-3 * gr.abs().max()
            assert not (differing & ~fragile).any()                                              # test_gpu_parity.py:411-416
        else:
            assert int(differing.sum()) <= max(2, differing.numel() // 100)                      # test_gpu_parity.py:418
        return
    if meta["only_norm"]:
        if not multi:
            gr, og = g["ln_grad"], c("ln_grad")
            assert gr.norm() > 0 and (og - gr).norm() / gr.norm() < 2e-3                         # test_gpu_kd.py:215-216
        d = (c("ln_after") - g["ln_after"]).abs()
        assert (d > 0.1 * meta["lr"]).float().mean() < 0.01                                      # test_gpu_kd.py:217-218
        return
    keys = RR.visual_param_keys(ssd)
    grad, after = eng.merge_visual(o["ln_grad"], o["vis_grad"]), eng.merge_visual(o["ln_after"], o["vis_after"])
    gn, gref = _tensor_norms(ssd, keys, grad), g["vis_grad_l2"]
    keep = torch.ones(len(keys), dtype=torch.bool)
    if rn:                         # attnpool.k_proj.bias: zero gradient in exact arithmetic (test_gpu_kd.py:224-227)
        kb = keys.index("visual.attnpool.k_proj.bias")
        keep[kb] = False
        assert gn[kb] < 1e-6 * gref.max()
    torch.testing.assert_close(gn[keep], gref[keep], rtol=3e-3, atol=1e-8)                       # test_gpu_kd.py:228
    dn, dref = _tensor_norms(ssd, keys, after, ssd), g["vis_delta_l2"]
    kbias = torch.tensor([k.endswith("attn.in_proj_bias") for k in keys])
    torch.testing.assert_close(dn[keep & ~kbias], dref[keep & ~kbias], rtol=0.01, atol=1e-7)     # test_gpu_kd.py:233
    if kbias.any():
        wv = synth.GEOMETRIES[meta["student"]].vision_width
        assert ((dn[kbias] - dref[kbias]).abs() <= 0.01 * dref[kbias] + meta["lr"] * wv ** 0.5).all()   # test_gpu_kd.py:234-236
    if "vis_grad_sample" in g:
        gr, og = g["vis_grad_sample"], grad[::7].cpu()
        assert (og - gr).norm() / gr.norm() < 2e-3                                               # test_gpu_kd.py:238-239
        d = (after[::7].cpu() - g["vis_after_sample"]).abs()
        assert (d > 0.1 * meta["lr"]).float().mean() < 0.01                                      # test_gpu_kd.py:240-241


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("case", E2E)
def test_tpt_tuning_matches_reference_fixture(L, dev, case, prec):
    """rlcf_tta_sample / rlcf_tta_sample_ln / rlcf_tta_sample_visual under RLCF_F_TPT, on an engine WITHOUT a reward model, against the
    reference's own tpt_cls / tune_cls_tpt test_time_tuning; an engine that holds a reward model gives the same bits"""
    g, meta = T.load_golden(case)
    eng, ssd, views = _engine(L, dev, meta, prec, reward=False)
    o = _call(eng, meta)(views, _cfg(meta))
    torch.cuda.synchronize()
    _check_e2e(eng, o, g, meta, ssd)
    with pytest.raises(L.RlcfError, match="reward model not set"):      # the RL loss still needs its reward model
        _call(eng, meta)(views, _cfg(meta, tpt=False))
    eng.close()
    eng2, _, _ = _engine(L, dev, meta, prec, reward=True)
    o2 = _call(eng2, meta)(views, _cfg(meta))
    torch.cuda.synchronize()
    for k in o:
        assert torch.equal(o[k], o2[k]), k
    eng2.close()


@pytest.mark.parametrize("kind", ["prompt", "ln", "vis"])
def test_tpt_zero_steps_is_plain_inference(L, dev, kind):
    g, meta = T.load_golden({"prompt": "tpt_tiny_s1", "ln": "tpt_tiny_ln_s1", "vis": "tpt_tiny_vis_s1"}[kind])
    eng, ssd, views = _engine(L, dev, meta, 2, reward=True)
    a = _call(eng, meta)(views, _cfg(meta, tta_steps=0))
    b = _call(eng, meta)(views, _cfg(meta, tpt=False, tta_steps=0))
    assert torch.equal(a["final_logits"], b["final_logits"]) and torch.equal(a["top5"], b["top5"])
    eng.close()
    bare, _, _ = _engine(L, dev, meta, 2, reward=False)
    c = _call(bare, meta)(views, _cfg(meta, tta_steps=0))
    assert torch.equal(a["final_logits"], c["final_logits"])
    bare.close()


def test_tpt_one_class_bank_and_sample_k_ignored(L, dev):
    """sample_k <= C must not reject a one-class bank under the flag (sample_k is ignored); loss and gradients are zero there"""
    g, meta = T.load_golden("tpt_tiny_ln_s1")
    eng, ssd, views = _engine(L, dev, meta, 2, reward=False, n_cls=1)
    o = eng.tta_sample_ln(views, _cfg(meta, sample_k=3))
    assert o["loss"].item() == 0.0 and o["dlogits"].abs().max().item() == 0.0 and o["step_skipped"].tolist() == [0]
    eng.close()
    eng, ssd, views = _engine(L, dev, meta, 2, reward=False)
    a, b = eng.tta_sample_ln(views, _cfg(meta, sample_k=3)), eng.tta_sample_ln(views, _cfg(meta, sample_k=0))
    assert torch.equal(a["dlogits"], b["dlogits"]) and torch.equal(a["loss"], b["loss"])
    eng.close()


@pytest.mark.parametrize("steps", [1, 3])
@pytest.mark.parametrize("prec", [0, 2])
def test_tpt_batch_ln_equals_per_sample(L, dev, prec, steps):
    """rlcf_tta_batch_ln on 3 samples (one fused pass, the grouped loss kernel with groups = 3) against 3 rlcf_tta_sample_ln calls, at
    the bar of test_ln_tuning_sample_batch_equals_per_sample (tests/test_gpu_parity.py:1128-1132)"""
    g, meta = T.load_golden("tpt_tiny_ln_s1" if steps == 1 else "tpt_tiny_ln_s3")
    N, B = meta["n_views"], 3
    R = synth.GEOMETRIES[meta["student"]].image_resolution
    vs = torch.stack([synth.make_views(meta["view_seed"] + i, N, R) for i in range(B)]).to(dev)
    cfg = _cfg(meta)
    one, _, _ = _engine(L, dev, meta, prec, reward=False)
    ref = [one.tta_sample_ln(vs[i], cfg) for i in range(B)]
    one.close()
    big, _, _ = _engine(L, dev, meta, prec, reward=False, max_views=N * B)
    top5, fl = big.tta_batch_ln(vs, cfg, want_logits=True)
    for i in range(B):
        if steps == 1:
            assert top5[i].tolist() == ref[i]["top5"].tolist()
        else:
            assert top5[i][0].item() == ref[i]["top5"][0].item()
        torch.testing.assert_close(fl[i], ref[i]["final_logits"][0], atol=5e-4 if steps == 1 else 1e-3, rtol=0)
    torch.testing.assert_close(fl[0].cpu(), g["final_logits"][0], atol=1e-3, rtol=0)
    big.close()


def test_tpt_batch_equals_per_sample_bitwise(L, dev):
    """rlcf_tta_batch under the flag runs its samples one by one through the one-image call: the same bits"""
    g, meta = T.load_golden("tpt_tiny_s1")
    N, B = meta["n_views"], 3
    R = synth.GEOMETRIES[meta["student"]].image_resolution
    vs = torch.stack([synth.make_views(meta["view_seed"] + i, N, R) for i in range(B)]).to(dev)
    cfg = _cfg(meta)
    eng, _, _ = _engine(L, dev, meta, 2, reward=False, max_views=N * B)
    ref = [eng.tta_sample(vs[i], cfg) for i in range(B)]
    top5, fl = eng.tta_batch(vs, cfg, want_logits=True)
    for i in range(B):
        assert torch.equal(fl[i], ref[i]["final_logits"][0]) and torch.equal(top5[i], ref[i]["top5"])
    eng.close()


def test_tpt_refusals(L, dev):
    g, meta = T.load_golden("tpt_tiny_vis_s1")
    eng, ssd, views = _engine(L, dev, meta, 2, reward=True)
    lib = L.lib()
    N = meta["n_views"]
    out = L.TTAOut()
    top5 = torch.empty(1, 5, dtype=torch.int32, device=dev)
    for extra in (L.F_KD, L.F_DKD, L.F_ATKD, L.F_MIN_ENTROPY, 16):
        a = _cfg(meta).c_args(N)
        a.flags |= extra
        for fn in (lib.rlcf_tta_sample, lib.rlcf_tta_sample_ln, lib.rlcf_tta_sample_visual):
            assert fn(eng.h, views.data_ptr(), N, C.byref(a), C.byref(out), st()) == -1, extra
            assert b"RLCF_F_TPT" in lib.rlcf_last_error()
        for fn in (lib.rlcf_tta_batch, lib.rlcf_tta_batch_ln):
            assert fn(eng.h, views.data_ptr(), 1, N, C.byref(a), None, top5.data_ptr(), st()) == -1, extra
            assert b"RLCF_F_TPT" in lib.rlcf_last_error()
    a = _cfg(meta).c_args(N)
    engines = (C.c_void_p * 1)(eng.h)
    assert lib.rlcf_tta_lanes(engines, 1, views.data_ptr(), 1, N, C.byref(a), None, top5.data_ptr(), 0, st()) == -1
    assert b"rlcf_tta_lanes" in lib.rlcf_last_error()
    lanes = lib.rlcf_lanes_create(engines, 1)
    assert lanes
    assert lib.rlcf_lanes_submit(lanes, views.data_ptr(), 1, N, C.byref(a), None, top5.data_ptr(), 0, st()) == -1
    assert b"rlcf_lanes_submit" in lib.rlcf_last_error()
    lib.rlcf_lanes_destroy(lanes)
    tok = torch.zeros(synth.GEOMETRIES[meta["student"]].context_length, dtype=torch.int32)
    assert lib.rlcf_tta_retrieval_image(eng.h, views.data_ptr(), N, C.byref(a), C.byref(out), st()) == -1
    assert b"rlcf_tta_retrieval_image" in lib.rlcf_last_error()
    assert lib.rlcf_tta_retrieval_image_kd(eng.h, views.data_ptr(), N, C.byref(a), None, C.byref(out), st()) == -1
    assert b"rlcf_tta_retrieval_image_kd" in lib.rlcf_last_error()
    assert lib.rlcf_tta_retrieval_text(eng.h, tok.data_ptr(), C.byref(a), C.byref(out), st()) == -1
    assert b"rlcf_tta_retrieval_text" in lib.rlcf_last_error()
    assert lib.rlcf_tta_retrieval_text_kd(eng.h, tok.data_ptr(), C.byref(a), None, C.byref(out), st()) == -1
    assert b"rlcf_tta_retrieval_text_kd" in lib.rlcf_last_error()
    # the refusals leave the engine working
    o = eng.tta_sample_visual(views, _cfg(meta))
    torch.cuda.synchronize()
    _check_e2e(eng, o, g, meta, ssd)
    eng.close()


@pytest.mark.parametrize("kind", ["prompt", "ln", "vis"])
def test_tpt_nan_pixel_skips_the_step(L, dev, kind):
    """a NaN pixel in a selected view (a NaN entropy sorts last, so every view is selected here): non-finite loss and gradient, step_skipped set, the tuned tensors stay at their reset state"""
    g, meta = T.load_golden({"prompt": "tpt_tiny_s1", "ln": "tpt_tiny_ln_s1", "vis": "tpt_tiny_vis_s1"}[kind])
    eng, ssd, views = _engine(L, dev, meta, 2, reward=False)
    reset_ln = eng.ln_params(pristine=True).clone()
    bad = views.clone()
    bad[3, 1, 5, 7] = float("nan")
    o = _call(eng, meta)(bad, _cfg(meta, selection_p=1.0))      # every view selected: the poisoned one is in the loss
    assert o["step_skipped"].tolist() == [1]
    assert not torch.isfinite(o["loss"]).any()
    if kind == "prompt":
        ctx0 = ssd["token_embedding.weight"][torch.tensor(synth.ctx_token_ids_default(synth.GEOMETRIES[meta["student"]], meta["n_ctx"]), device=dev)]
        assert torch.equal(o["ctx_after"], ctx0)
    else:
        assert torch.equal(o["ln_after"], reset_ln)
        if kind == "vis":
            assert torch.equal(o["vis_after"], eng.visual_params(1))
    ok = _call(eng, meta)(views, _cfg(meta))                 # and the next clean sample is the fixture's
    assert ok["step_skipped"].tolist() == [0]
    torch.testing.assert_close(ok["final_logits"].cpu(), g["final_logits"], atol=1e-3, rtol=0)
    eng.close()


# ------------------------------------------------------------------------------ the mirrors
def _mirror_args(meta, **kw):
    return types.SimpleNamespace(tta_steps=meta["tta_steps"], selection_p=meta["selection_p"], gpu=0, tpt=True, print_freq=1000, cocoop=False, **kw)


def _loader(g, meta):
    loader = []
    for i in range(meta["n_samples"]):
        views = synth.make_views(meta["view_seed0"] + i, meta["n_views"], 32)
        target = int(g["top5"][i, 0]) if i % 2 == 0 else int(g["top5"][i, 4])
        loader.append(([views[j: j + 1] for j in range(meta["n_views"])], torch.tensor([target])))
    return loader


def test_tpt_cls_eval_loop_matches_reference(L, dev, monkeypatch):
    """tpt_cls.test_time_adapt_eval (TPT/tpt_cls.py:242-314) through the mirror, no reward model anywhere: the tpt_eval_tiny top-5"""
    from rlcf_amd import clip_store, custom_clip, runtime, tpt_cls, tpt_cls_rl
    g, meta = T.load_golden("tpt_eval_tiny")
    runtime.reset_session()
    sg = synth.GEOMETRIES[meta["student"]]
    clip_store.register_checkpoint(meta["student"], sg, synth.make_state_dict(sg, meta["student_seed"]))
    bank = clip_store.SyntheticBank(sg, meta["n_cls"], meta["n_ctx"], meta["bank_seed"])
    clip_store.set_tokenizer(bank.tokenize)
    model = custom_clip.get_coop(meta["student"], "I", dev, meta["n_ctx"], "a_photo_of_a", classnames=bank.classnames)
    for name, p in model.named_parameters():
        if "prompt_learner" not in name:
            p.requires_grad_(False)
    optimizer = torch.optim.AdamW(model.prompt_learner.parameters(), meta["lr"], weight_decay=meta["weight_decay"])
    optim_state = copy.deepcopy(optimizer.state_dict())
    model.reset_classnames(bank.classnames, meta["student"])
    args = _mirror_args(meta)
    loader = _loader(g, meta)
    seen = []
    acc = tpt_cls_rl.accuracy

    def record(output, target, topk=(1,)):
        seen.append(output.detach().float().cpu())
        return acc(output, target, topk)

    monkeypatch.setattr(tpt_cls_rl, "accuracy", record)
    top1, top5 = tpt_cls.test_time_adapt_eval(loader, model, None, optimizer, optim_state, None, args)
    assert not runtime.SESSION.rewards and len(seen) == meta["n_samples"]
    for i, out in enumerate(seen):
        assert torch.topk(out, 5, dim=-1).indices[0].tolist() == g["top5"][i].tolist()
        torch.testing.assert_close(out[0], g["final_logits"][i], atol=1e-3, rtol=0)
    n = meta["n_samples"]
    assert abs(top1 - 100.0 * ((n + 1) // 2) / n) < 1e-2 and abs(top5 - 100.0) < 1e-2
    # images_per_pass > 1: the engine loops over the samples (rlcf_tta_batch under the flag); in_flight and cocoop raise
    a2 = _mirror_args(meta, images_per_pass=2)
    assert tpt_cls.test_time_adapt_eval(loader, model, None, optimizer, optim_state, None, a2) == [top1, top5]
    with pytest.raises(NotImplementedError):
        tpt_cls.test_time_adapt_eval(loader, model, None, optimizer, optim_state, None, _mirror_args(meta, in_flight=2))
    args.cocoop = True
    with pytest.raises(NotImplementedError):
        tpt_cls.test_time_adapt_eval(loader, model, None, optimizer, optim_state, None, args)
    with pytest.raises(NotImplementedError):
        tpt_cls.test_time_tuning(model, torch.cat(loader[0][0]).to(dev), optimizer, None, args)
    with pytest.raises(ValueError):                          # reward_model=None is legal only with tpt
        tpt_cls_rl.test_time_tuning(model, torch.cat(loader[0][0]).to(dev), optimizer, None, _mirror_args(meta))
    runtime.reset_session()


def test_tune_cls_tpt_eval_loop(L, dev, monkeypatch):
    """tune_cls_tpt.test_time_adapt_eval (TPT/tune_cls_tpt.py:184-240) with reward_model=None on CLIPCLS_TTA(only_norm=True): sample 0
    of the loop is the reference's tpt_tiny_ln_s1 run; images_per_pass = 2 (the fused LayerNorm pass) predicts the same; in_flight raises"""
    from rlcf_amd import clip_store, custom_clip, runtime, tpt_cls_rl, tune_cls_tpt
    g, meta = T.load_golden("tpt_tiny_ln_s1")
    runtime.reset_session()
    sg = synth.GEOMETRIES[meta["student"]]
    clip_store.register_checkpoint(meta["student"], sg, synth.make_state_dict(sg, meta["student_seed"]))
    bank = clip_store.SyntheticBank(sg, meta["n_cls"], meta["n_ctx"], meta["bank_seed"])
    clip_store.set_tokenizer(bank.tokenize)
    model = custom_clip.CLIPCLS_TTA(dev, bank.classnames, arch=meta["student"], prompt_prefix="a_photo_of_a", only_visual=True, only_norm=True)
    optimizer = torch.optim.AdamW(model.parameters(), meta["lr"], weight_decay=meta["weight_decay"])
    optim_state = copy.deepcopy(optimizer.state_dict())
    args = _mirror_args(meta)
    loader = []
    for i in range(2):
        views = synth.make_views(meta["view_seed"] + i, meta["n_views"], sg.image_resolution)
        loader.append(([views[j: j + 1] for j in range(meta["n_views"])], torch.tensor([int(g["top5"][0])])))
    seen = []
    acc = tpt_cls_rl.accuracy

    def record(output, target, topk=(1,)):
        seen.append(output.detach().float().cpu())
        return acc(output, target, topk)

    monkeypatch.setattr(tpt_cls_rl, "accuracy", record)
    res = tune_cls_tpt.test_time_adapt_eval(loader, model, optimizer, optim_state, None, args, reward_model=None)
    assert not runtime.SESSION.rewards and len(seen) == 2
    torch.testing.assert_close(seen[0], g["final_logits"], atol=1e-3, rtol=0)
    assert torch.topk(seen[0], 5, dim=-1).indices[0].tolist() == g["top5"].tolist()
    assert tune_cls_tpt.test_time_adapt_eval(loader, model, optimizer, optim_state, None, _mirror_args(meta, images_per_pass=2),
                                             reward_model=None) == res
    with pytest.raises(NotImplementedError):
        tune_cls_tpt.test_time_adapt_eval(loader, model, optimizer, optim_state, None, _mirror_args(meta, in_flight=2), reward_model=None)
    runtime.reset_session()
