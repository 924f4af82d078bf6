"""GPU: the distillation losses of the KD ablation (TPT/tune_cls_kd.py) on the HIP path — the rlcf_kd_loss kernel against the
reference's float64 gradients (tests/golden/kd_ops.npz), rlcf_amd.kd_losses, the engine's LayerNorm / every-parameter / ResNet
tuning calls with RLCF_F_KD / DKD / ATKD against the reference's own tune_cls_kd.test_time_tuning runs (tests/golden/kd_*.npz,
tests/golden/make_kd_golden.py), the tune_cls_kd.py loop through the mirror, and the entry points that refuse the losses."""
import copy
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

from oracle import rlcf_ref as RR
from rlcf_amd import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
LOSSES = ("KD", "DKD", "ATKD")
E2E = ["kd_tiny_ln_s1", "kd_tiny_ln_s3", "kd_tiny_vis_s1", "kd_tiny_vis_s3", "kd_tiny_rn_s1"]


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


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    arrays = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("meta_")}
    meta = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    return arrays, meta


# ------------------------------------------------------------------------------ op level
def _ops():
    z = np.load(os.path.join(GOLDEN, "kd_ops.npz"))
    meta = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    return z, meta


def _op_entries():
    z, meta = _ops()
    return [(c, k) for c in meta["cases"].split(",") for k in LOSSES if f"{c}_{k}_loss" in z.files]


def _params(L, meta, case, kind):
    hp = dict(T_stu=1.0, T_tea=1.0, alpha=1.0, beta=0.5, temperature=1.0, multiplier=2.0, eps=1e-5)
    for k in hp:
        hp[k] = float(meta.get(f"{case}_{kind}_{k}", hp[k]))
    return L.KdParams(*[hp[k] for k in ("T_stu", "T_tea", "alpha", "beta", "temperature", "multiplier", "eps")]), hp


def _bar(case, kind, s):
    """relative bar of the kernel against float64.  The kernel evaluates every row in double and rounds once to float32, so the
    well-conditioned rows meet 1e-5.  The edge rows amplify nothing the kernel adds: DKD at p_target -> 1 forms p_other / p_other
    ratios as the NCKD softmax (no cancellation: exact to double rounding), and ATKD scales by multiplier / (mean + eps), an error
    amplification of |multiplier * max|z| / (mean + eps)| on the float64 side too — the bar widens by that factor over 100 (the
    row scale of CLIP logits), so a row mean near 0 would get a looser bar rather than a false failure."""
    if kind != "ATKD":
        return 1e-5
    m = s.double().mean(1).abs().min().item()
    amp = 2.0 * s.double().abs().max().item() / max(m, 1e-6)
    return 1e-5 * max(1.0, amp / 100.0)


@pytest.mark.parametrize("case,kind", _op_entries())
def test_kd_loss_op_matches_reference_float64(L, dev, case, kind):
    from rlcf_amd.engine import KD_MODES, kd_loss_op
    z, meta = _ops()
    p, _ = _params(L, meta, case, kind)
    s, t = torch.from_numpy(z[case + "_s"]).to(dev), torch.from_numpy(z[case + "_t"]).to(dev)
    loss, dlog, rows = kd_loss_op(s, t, KD_MODES[kind], None, p, row_loss=True)
    torch.cuda.synchronize()
    l64, d64 = torch.from_numpy(z[f"{case}_{kind}_loss64"]), torch.from_numpy(z[f"{case}_{kind}_dlog64"])
    bar = _bar(case, kind, s.cpu())
    torch.testing.assert_close(loss.cpu().double()[0], l64, rtol=bar, atol=1e-6)
    torch.testing.assert_close(rows.cpu().double().mean(), l64, rtol=bar, atol=1e-6)
    if d64.norm() == 0:                          # (one class: softmax = 1 on both sides, no gradient)
        assert dlog.abs().max().item() < 1e-12
    else:
        assert ((dlog.cpu().double() - d64).norm() / d64.norm()).item() < bar
    # bit-reproducible (fixed-order reductions, no atomics)
    loss2, dlog2, rows2 = kd_loss_op(s, t, KD_MODES[kind], None, p, row_loss=True)
    assert torch.equal(loss, loss2) and torch.equal(dlog, dlog2) and torch.equal(rows, rows2)
    if kind == "DKD":                            # the teacher argmax passed explicitly = the default target
        loss3, dlog3, _ = kd_loss_op(s, t, KD_MODES[kind], t.argmax(-1), p)
        assert torch.equal(loss, loss3) and torch.equal(dlog, dlog3)


def test_kd_loss_op_strided_rows_and_defaults(L, dev):
    """a row stride larger than C (rows of a wider matrix) and params = NULL (the reference's defaults)"""
    from rlcf_amd.engine import kd_loss_op
    z, meta = _ops()
    s, t = torch.from_numpy(z["c200_s"]).to(dev), torch.from_numpy(z["c200_t"]).to(dev)
    wide_s = torch.zeros(s.shape[0], 256, device=dev); wide_s[:, :200] = s
    wide_t = torch.full((s.shape[0], 256), 1e4, device=dev); wide_t[:, :200] = t
    for mode, kind in ((L.KD_KD, "KD"), (L.KD_DKD, "DKD"), (L.KD_ATKD, "ATKD")):
        loss, dlog, _ = kd_loss_op(wide_s[:, :200], wide_t[:, :200], mode)
        l0, d0, _ = kd_loss_op(s, t, mode)
        assert torch.equal(loss, l0) and torch.equal(dlog, d0)


def test_kd_loss_op_refuses_bad_arguments(L, dev):
    lib = L.lib()
    s = torch.zeros(2, 8, device=dev)
    out = torch.empty(1, device=dev)
    d = torch.empty(2, 8, device=dev)
    call = lambda mode, n, c: lib.rlcf_kd_loss(s.data_ptr(), 8, s.data_ptr(), 8, n, c, mode, None, None, out.data_ptr(), None,
                                               d.data_ptr(), st())
    assert call(L.KD_KD, 2, 8) == 0
    for mode, n, c in ((0, 2, 8), (4, 2, 8), (-1, 2, 8), (L.KD_KD, 0, 8), (L.KD_DKD, -3, 8), (L.KD_ATKD, 2, 0), (L.KD_KD, 1, L.KD_MAX_CLASSES + 1)):
        assert call(mode, n, c) == -1, (mode, n, c)
        assert lib.rlcf_last_error()
    torch.cuda.synchronize()


@pytest.mark.parametrize("case,kind", [e for e in _op_entries() if e[0] in ("c37", "c1000", "hp", "pgt1")])
def test_kd_losses_module_on_device(L, dev, case, kind):
    """rlcf_amd.kd_losses on device float32 tensors: one kernel launch, differentiable in the student (teacher constant)"""
    from rlcf_amd import kd_losses as K
    z, meta = _ops()
    _, hp = _params(L, meta, case, kind)
    s = torch.from_numpy(z[case + "_s"]).to(dev).requires_grad_(True)
    t = torch.from_numpy(z[case + "_t"]).to(dev)
    if kind == "KD":
        loss = K.kd_distill_loss_v2(s, t, hp["T_stu"], hp["T_tea"])
    elif kind == "DKD":
        loss = K.dkd_distill_loss(s, t, t.argmax(-1), hp["alpha"], hp["beta"], hp["temperature"])
    else:
        loss = K.atkd_distill_loss(s, t, multiplier=hp["multiplier"], eps=hp["eps"])
    (3.0 * loss).backward()
    l64, d64 = torch.from_numpy(z[f"{case}_{kind}_loss64"]), torch.from_numpy(z[f"{case}_{kind}_dlog64"])
    assert loss.shape == () and loss.is_cuda
    torch.testing.assert_close(loss.detach().cpu().double(), l64, rtol=1e-5, atol=1e-6)
    assert ((s.grad.cpu().double() - 3.0 * d64).norm() / (3.0 * d64).norm()).item() < 1e-5
    torch.testing.assert_close(loss.detach().cpu(), torch.from_numpy(z[f"{case}_{kind}_loss"]), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------ engine calls (tune_cls_kd.py:34-61)
def _engine(L, dev, meta, prec):
    from rlcf_amd.engine import Engine
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    ssd = synth.make_state_dict(sg, meta["student_seed"], device=dev)
    rsd = synth.make_state_dict(rg, meta["reward_seed"], device=dev)
    eng = Engine(sg, rg, meta["n_views"], meta["n_cls"], prec)
    eng.load_state_dict(L.STUDENT, ssd)
    eng.load_state_dict(L.REWARD, rsd)
    eng.finalize()
    tokens = synth.make_token_bank(sg, meta["n_cls"], seed=meta["bank_seed"], n_ctx=meta["n_ctx"])
    ctx0 = ssd["token_embedding.weight"][torch.tensor(synth.ctx_token_ids_default(sg, meta["n_ctx"]), device=dev)].clone()
    eng.set_class_bank(tokens, meta["n_ctx"], ctx0, L.TEXT_SHARED)
    views = synth.make_views(meta["view_seed"], meta["n_views"], sg.image_resolution, device=dev)
    return eng, ssd, views


def _cfg(meta, kd_loss=None):
    from rlcf_amd.engine import TTAConfig
    return TTAConfig(selection_p=meta["selection_p"], tta_steps=meta["tta_steps"], sample_k=meta["sample_k"], lr=meta["lr"],
                     weight_decay=meta["weight_decay"], kd_loss=kd_loss)


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


def _check_e2e(eng, o, g, meta, ssd, L):
    kind = meta["kd_loss"]
    rn = synth.GEOMETRIES[meta["student"]].is_resnet
    full_size = meta["n_cls"] > 64
    c = lambda k: o[k].cpu()
    assert c("selected_idx").tolist() == g["selected_idx"].tolist()
    assert c("top5").tolist()[: g["top5"].numel()] == g["top5"].tolist()
    assert not {"topk_idx", "clip_score", "rewards"} & set(o)          # the distillation losses sample no classes
    n_log = g["logits"].shape[1]
    torch.testing.assert_close(c("logits")[:, :n_log], g["logits"], atol=3e-4 if rn else 1e-3, rtol=0)
    rif = c("reward_image_features")
    torch.testing.assert_close(rif[:, ::7] if full_size else rif, g["reward_image_features"], atol=1e-4, rtol=0)
    # step 0: the loss and dlogits.  ATKD divides by the student's row mean (kd.hip): a student-logit error e becomes ~e * 2 / mean in
    # the normalised row, so its bars widen by 0.5 / min|row mean| (the generator records that value; >= 0.12 for these cases)
    widen = max(1.0, 0.5 / meta["min_abs_row_mean"]) if kind == "ATKD" else 1.0
    torch.testing.assert_close(c("loss"), g["loss"], rtol=1e-4 * widen, atol=1e-4 * widen)
    dl = c("dlogits")
    if full_size:
        torch.testing.assert_close(dl.double().norm(dim=1).float(), g["dlogits_l2"], rtol=2e-3, atol=1e-9)
        dl = dl[:, ::7]
    gd = g["dlogits"]
    assert ((dl - gd).norm() / gd.norm()).item() < 2e-3 * widen
    multi = meta["tta_steps"] > 1
    torch.testing.assert_close(c("final_logits"), g["final_logits"], atol=2e-3 if full_size else 1e-3, rtol=0)
    if meta["only_norm"]:
        if not multi:
            gr, og = g["ln_grad"], c("ln_grad")
            assert gr.norm() > 0 and (og - gr).norm() / gr.norm() < 2e-3 * widen
        d = (c("ln_after") - g["ln_after"]).abs()
        assert (d > 0.1 * meta["lr"]).float().mean() < 0.01
        return
    keys = RR.visual_param_keys(ssd)
    grad, after = eng.merge_visual(o["ln_grad"], o["vis_grad"]), eng.merge_visual(o["ln_after"], o["vis_after"])
    gn, gref = _tensor_norms(ssd, keys, grad), g["vis_grad_l2"]
    keep = torch.ones(len(keys), dtype=torch.bool)
    if rn:                         # attnpool.k_proj.bias: zero gradient in exact arithmetic (softmax is blind to a shift of the keys)
        kb = keys.index("visual.attnpool.k_proj.bias")
        keep[kb] = False
        assert gn[kb] < 1e-6 * gref.max()
    torch.testing.assert_close(gn[keep], gref[keep], rtol=(1e-2 if full_size else 3e-3) * widen, atol=1e-8)
    # attn.in_proj_bias: its key third has zero gradient in exact arithmetic (softmax is blind to a common shift of the scores), so
    # AdamW moves those Wv elements by up to lr each on either side's rounding noise: their delta norm carries up to lr * sqrt(Wv)
    dn, dref = _tensor_norms(ssd, keys, after, ssd), g["vis_delta_l2"]
    kbias = torch.tensor([k.endswith("attn.in_proj_bias") for k in keys])
    torch.testing.assert_close(dn[keep & ~kbias], dref[keep & ~kbias], rtol=0.05 if full_size else 0.01, atol=1e-7)
    if kbias.any():
        wv = synth.GEOMETRIES[meta["student"]].vision_width
        assert ((dn[kbias] - dref[kbias]).abs() <= 0.01 * dref[kbias] + meta["lr"] * wv ** 0.5).all()
    if "vis_grad_sample" in g:
        gr, og = g["vis_grad_sample"], grad[::7].cpu()
        assert (og - gr).norm() / gr.norm() < 2e-3 * widen
        d = (after[::7].cpu() - g["vis_after_sample"]).abs()
        assert (d > 0.1 * meta["lr"]).float().mean() < 0.01


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("kind", LOSSES)
@pytest.mark.parametrize("case", E2E)
def test_kd_tuning_matches_reference_fixture(L, dev, case, kind, prec):
    """rlcf_tta_sample_ln / rlcf_tta_sample_visual with the distillation loss vs the reference's own tune_cls_kd.test_time_tuning on
    CLIPCLS_TTA (only_norm 1 for `ln`, 0 for `vis` / `rn`): selection, the teacher's input, step 0's loss and dlogits, the gradients,
    the adapted parameters and the final logits.  The RL paths give what they gave before the call (the engine ends pristine)."""
    g, meta = load_golden(f"{case}_{kind.lower()}")
    eng, ssd, views = _engine(L, dev, meta, prec)
    rn = synth.GEOMETRIES[meta["student"]].is_resnet
    rl = _cfg(meta)
    call = eng.tta_sample_ln if meta["only_norm"] else eng.tta_sample_visual
    base_ln = eng.tta_sample_ln(views, rl)["final_logits"].clone()
    base_vis = eng.tta_sample_visual(views, rl)["final_logits"].clone()
    base_p = None if rn else eng.tta_sample(views, rl)["final_logits"].clone()
    o = call(views, _cfg(meta, kind))
    torch.cuda.synchronize()
    _check_e2e(eng, o, g, meta, ssd, L)
    # the same call repeats, and the RL LayerNorm / visual / prompt paths return what they returned before (float atomics in the
    # LayerNorm-gradient reductions: last-bit run-to-run differences, the bars of test_visual_tuning_matches_reference_fixture)
    o2 = call(views, _cfg(meta, kind))
    torch.testing.assert_close(o2["final_logits"], o["final_logits"], atol=2e-4, rtol=0)
    torch.testing.assert_close(eng.tta_sample_ln(views, rl)["final_logits"], base_ln, atol=1e-4, rtol=0)
    torch.testing.assert_close(eng.tta_sample_visual(views, rl)["final_logits"], base_vis, atol=2e-4, rtol=0)
    if base_p is not None:
        torch.testing.assert_close(eng.tta_sample(views, rl)["final_logits"], base_p, atol=2e-4, rtol=0)
    eng.close()


@pytest.mark.parametrize("prec", [2])
def test_kd_tune_sh_configuration_full_size(L, dev, prec):
    """scripts/kd-tune.sh at full size: ViT-B/16 student, ViT-L/14 reward, N = 64 views (6 selected), 1000 classes, 3 steps, lr 1e-5,
    every visual parameter tuned, --kd_loss KD"""
    g, meta = load_golden("kd_b16_l14_vis_s3_n64_kd")
    eng, ssd, views = _engine(L, dev, meta, prec)
    o = eng.tta_sample_visual(views, _cfg(meta, meta["kd_loss"]))
    torch.cuda.synchronize()
    _check_e2e(eng, o, g, meta, ssd, L)
    eng.close()


# ------------------------------------------------------------------------------ the mirror (tune_cls_kd.py:191-236)
def _mirror(dev, meta, only_norm=False):
    from rlcf_amd import clip_reward, clip_store, custom_clip, runtime
    runtime.reset_session()
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    clip_store.register_checkpoint(meta["student"], sg, synth.make_state_dict(sg, meta["student_seed"]))
    clip_store.register_checkpoint(meta["reward"], rg, synth.make_state_dict(rg, meta["reward_seed"]))
    bank = clip_store.SyntheticBank(sg, meta["n_cls"], meta["n_ctx"], meta["bank_seed"])
    clip_store.set_tokenizer(bank.tokenize)
    args = types.SimpleNamespace(tta_steps=meta["tta_steps"], selection_p=meta["selection_p"], gpu=0, tpt=True, print_freq=1000,
                                 reward_arch=meta["reward"], multiple_reward_models=0, sample_k=meta["sample_k"], reward_amplify=False,
                                 reward_process=True, process_batch=False, kd_loss=meta["kd_loss"])
    model = custom_clip.CLIPCLS_TTA(dev, bank.classnames, arch=meta["student"], prompt_prefix="a_photo_of_a", only_visual=True,
                                    only_norm=only_norm)
    reward_model = clip_reward.get_reward_model(dev, args)
    reward_model.set_class_features(tokenized_classes=model.tokenized_prompts)
    optimizer = torch.optim.AdamW(model.parameters(), meta["lr"], weight_decay=meta["weight_decay"])
    return model, reward_model, optimizer, args


def test_tune_cls_kd_eval_loop_matches_reference(L, dev, monkeypatch):
    from rlcf_amd import runtime, tpt_cls_rl, tune_cls_kd
    g, meta = load_golden("kd_eval_tiny")
    model, reward_model, optimizer, args = _mirror(dev, meta)
    optim_state = copy.deepcopy(optimizer.state_dict())
    loader = []
    for i in range(meta["n_samples"]):
        views = synth.make_views(meta["view_seed0"] + i, meta["n_views"], 32)
        target = int(g["top5"][i, 0]) if i % 2 == 0 else int(g["top5"][i, 4])
        loader.append(([views[j: j + 1] for j in range(meta["n_views"])], torch.tensor([target])))
    seen = []
    acc = tpt_cls_rl.accuracy

    def record(output, target, topk=(1,)):
        seen.append(output.detach().float().cpu())
        return acc(output, target, topk)

    monkeypatch.setattr(tpt_cls_rl, "accuracy", record)
    top1, top5 = tune_cls_kd.test_time_adapt_eval(loader, model, optimizer, optim_state, None, args, reward_model=reward_model)
    assert len(seen) == meta["n_samples"]
    for i, out in enumerate(seen):
        assert torch.topk(out, 5, dim=-1).indices[0].tolist() == g["top5"][i].tolist()
        torch.testing.assert_close(out[0], g["final_logits"][i], atol=1e-3, rtol=0)
    n = meta["n_samples"]
    assert abs(top1 - 100.0 * ((n + 1) // 2) / n) < 1e-2 and abs(top5 - 100.0) < 1e-2
    # the one-step entry: what the loop ran for sample 0
    model.reset()
    optimizer.load_state_dict(optim_state)
    model.train()
    tune_cls_kd.test_time_tuning(model, torch.cat(loader[0][0]).to(dev), optimizer, None, args, reward_model=reward_model)
    model.eval()
    torch.testing.assert_close(model(loader[0][0][0].to(dev)).cpu()[0], g["final_logits"][0], atol=1e-3, rtol=0)
    for name in ("images_per_pass", "in_flight"):
        with pytest.raises(NotImplementedError):
            tune_cls_kd.test_time_adapt_eval(loader, model, optimizer, optim_state, None, types.SimpleNamespace(**vars(args), **{name: 2}),
                                             reward_model=reward_model)
    runtime.reset_session()


# ------------------------------------------------------------------------------ refusals
def test_entries_without_a_distillation_form_refuse_it(L, dev):
    g, meta = load_golden("kd_tiny_vis_s1_kd")
    eng, ssd, views = _engine(L, dev, meta, 2)
    lib = L.lib()
    cfg = _cfg(meta, "KD")
    N = meta["n_views"]
    with pytest.raises(L.RlcfError, match="rlcf_tta_sample"):
        eng.tta_sample(views, cfg)
    a = cfg.c_args(N)
    top5 = torch.empty(1, 5, dtype=torch.int32, device=dev)
    assert lib.rlcf_tta_batch(eng.h, views.data_ptr(), 1, N, C.byref(a), None, top5.data_ptr(), st()) == -1
    assert lib.rlcf_tta_batch_ln(eng.h, views.data_ptr(), 1, N, C.byref(a), None, top5.data_ptr(), st()) == -1
    engines = (C.c_void_p * 1)(eng.h)
    assert lib.rlcf_tta_lanes(engines, 1, views.data_ptr(), 1, N, C.byref(a), None, top5.data_ptr(), 0, st()) == -1
    out = L.TTAOut()
    assert lib.rlcf_tta_retrieval_image(eng.h, views.data_ptr(), N, C.byref(a), C.byref(out), st()) == -1
    assert b"distillation" in lib.rlcf_last_error()
    a.flags |= L.F_MIN_ENTROPY                                  # no regulariser with the distillation losses
    for fn in (lib.rlcf_tta_sample_ln, lib.rlcf_tta_sample_visual):
        assert fn(eng.h, views.data_ptr(), N, C.byref(a), C.byref(out), st()) == -1
    # the refusals leave the engine working: the distillation call itself still matches the fixture
    o = eng.tta_sample_visual(views, cfg)
    torch.cuda.synchronize()
    _check_e2e(eng, o, g, meta, ssd, L)
    eng.close()


def test_distillation_needs_one_reward_model(L, dev):
    from rlcf_amd.engine import Engine
    sg, rg = synth.GEOMETRIES["tiny"], synth.GEOMETRIES["tiny-r"]
    eng = Engine(sg, [rg, rg], 8, 16, 2)
    eng.load_state_dict(L.STUDENT, synth.make_state_dict(sg, 11, device=dev))
    for m in range(2):
        eng.load_state_dict(L.REWARD + m, synth.make_state_dict(rg, 23 + m, device=dev))
    eng.finalize()
    tokens = synth.make_token_bank(sg, 16, seed=7, n_ctx=4)
    ssd = synth.make_state_dict(sg, 11, device=dev)
    ctx0 = ssd["token_embedding.weight"][torch.tensor(synth.ctx_token_ids_default(sg, 4), device=dev)].clone()
    eng.set_class_bank(tokens, 4, ctx0, L.TEXT_SHARED)
    views = synth.make_views(1000, 8, sg.image_resolution, device=dev)
    from rlcf_amd.engine import TTAConfig
    with pytest.raises(L.RlcfError, match="one reward model"):
        eng.tta_sample_ln(views, TTAConfig(selection_p=0.5, kd_loss="DKD"))
    eng.close()
