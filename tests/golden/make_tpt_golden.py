"""Generate the fixtures of the TPT baseline (TPT/tpt_cls.py, TPT/tune_cls_tpt.py): the reference itself, imported read-only as
make_golden.py imports it, run on CPU in float32 on this repo's seeded synthetic weights, views and class banks.

  tpt_ops.npz             op level: avg_entropy (tpt_cls.py:40-46) and its autograd gradient in float32 and in float64 on CLIP-like
                          logit rows for (n, C) in {(1,1), (1,37), (2,2), (6,37), (6,1000), (7,1025), (64,200)}, a 3-group case of
                          (6, 200), a strided case (row stride C + 3) and rows where one class leads by 120 (the float32 softmax of
                          the others underflows)
  tpt_tiny_s1 / _s3       the prompt learner through tpt_cls.test_time_tuning
  tpt_tiny_{ln,vis,rn}_*  CLIPCLS_TTA through tune_cls_tpt.test_time_tuning (only_norm = 1 for `ln`, 0 for `vis` / `rn`)
  tpt_eval_tiny.npz       a few test images through the tpt_cls.py:242-314 loop body: per-sample top-5

tune_cls_tpt.py imports a module `policy` the reference does not contain: an empty stand-in is registered before the import.
Usage: python tests/golden/make_tpt_golden.py [--only ops,e2e,eval]
"""
from __future__ import annotations

import argparse
import copy
import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402
from make_golden import synth, RR  # noqa: E402
from make_kd_golden import clip_rows  # noqa: E402


def import_tpt(ref):
    pol = types.ModuleType("policy")
    pol.get_reward_model = lambda *a, **k: None
    sys.modules.setdefault("policy", pol)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        prompt = importlib.import_module("tpt_cls")
        tune = importlib.import_module("tune_cls_tpt")
    return types.SimpleNamespace(prompt=prompt, tune=tune)


# ------------------------------------------------------------------ op level
OP_SHAPES = ((1, 1), (1, 37), (2, 2), (6, 37), (6, 1000), (7, 1025), (64, 200))


def op_cases():
    """name -> (rows [groups * n, C], groups)"""
    cases = {}
    for n, C in OP_SHAPES:
        cases[f"n{n}_c{C}"] = (clip_rows(500 + 7 * n + C, n, C), 1)
    cases["g3_n6_c200"] = (clip_rows(601, 18, 200), 3)
    cases["strided_n6_c200"] = (clip_rows(602, 6, 200), 1)          # (the test lays the rows out with a row stride of C + 3)
    x = clip_rows(603, 6, 200)
    lead = torch.tensor([3, 3, 50, 50, 120, 199])
    x[torch.arange(6), lead] = x.max(dim=1).values + 120.0          # exp(-120) = 8e-53: zero in float32, a number in float64
    cases["lead120_n6_c200"] = (x, 1)
    return cases


def run_avg_entropy(T, x, groups, dtype):
    x = x.to(dtype).clone().requires_grad_(True)
    n = x.shape[0] // groups
    losses = torch.stack([T.prompt.avg_entropy(x[g * n: (g + 1) * n]) for g in range(groups)])
    losses.sum().backward()
    return losses.detach(), x.grad.detach()


def gen_ops(T):
    arrays, names = {}, []
    for name, (x, groups) in op_cases().items():
        l32, d32 = run_avg_entropy(T, x, groups, torch.float32)
        l64, d64 = run_avg_entropy(T, x, groups, torch.float64)
        arrays[name + "_x"], arrays[name + "_groups"] = x.numpy(), np.int64(groups)
        arrays[name + "_loss"], arrays[name + "_dlog"] = l32.numpy(), d32.numpy()
        arrays[name + "_loss64"], arrays[name + "_dlog64"] = l64.numpy(), d64.numpy()
        names.append(name)
        print(f"  {name:18s} loss {l32.tolist()} max|l32 - l64| {(l32.double() - l64).abs().max():.3g} "
              f"max|d32 - d64| {(d32.double() - d64).abs().max():.3g} max|d64| {d64.abs().max():.3g}")
    MG.save("tpt_ops", arrays, dict(cases=",".join(names), strided_pad=3))


# ------------------------------------------------------------------ end to end
E2E_CASES = {      # name -> (student, views, classes, overrides, kind); the tiny geometries and settings of the kd_tiny_* cases
    "tpt_tiny_s1": ("tiny", 8, 16, dict(lr=5e-3), "prompt"),
    "tpt_tiny_s3": ("tiny", 8, 16, dict(lr=5e-3, tta_steps=3), "prompt"),
    "tpt_tiny_ln_s1": ("tiny", 8, 16, dict(lr=1e-3), "ln"),
    "tpt_tiny_ln_s3": ("tiny", 8, 16, dict(lr=1e-3, tta_steps=3), "ln"),
    "tpt_tiny_vis_s1": ("tiny", 8, 16, dict(lr=1e-4), "vis"),
    "tpt_tiny_rn_s1": ("tiny-rn", 8, 16, dict(lr=1e-4), "vis"),
}
BASE_HP = dict(lr=1e-4, weight_decay=5e-4, tta_steps=1, selection_p=0.5)


def _taps(mod):
    """record the first call of select_confident_samples and avg_entropy of `mod` (logits, selection, loss, dlogits)"""
    taps = {}
    orig_select, orig_ent = mod.select_confident_samples, mod.avg_entropy

    def tap_select(logits, top):
        out, idx = orig_select(logits, top)
        if "logits" not in taps:
            taps["logits"], taps["selected_idx"] = logits.detach().clone(), idx.clone()
        return out, idx

    def tap_ent(out):
        loss = orig_ent(out)
        if "loss" not in taps:
            taps["loss"] = loss.detach().clone()

            def keep(g):                 # must return None: a returned tensor would replace the gradient
                taps.setdefault("dlogits", g.detach().clone())
            out.register_hook(keep)
        return loss

    mod.select_confident_samples, mod.avg_entropy = tap_select, tap_ent

    def undo():
        mod.select_confident_samples, mod.avg_entropy = orig_select, orig_ent
    return taps, undo


def _scaler():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return torch.cuda.amp.GradScaler(init_scale=1000)


def build_prompt_model(ref, student, n_cls, n_ctx, hp):
    s_geo = synth.GEOMETRIES[student]
    MG.install_models(ref, {student: (s_geo, synth.make_state_dict(s_geo, seed=11))})
    bank = MG.Bank(s_geo, n_cls, n_ctx)
    ref.custom.tokenize = bank.tokenize
    ref.custom._tokenizer = types.SimpleNamespace(
        encode=lambda name: [0] * (int(bank.tokens[int(name.split("c")[-1])].argmax()) - 1 - n_ctx - 1))
    model = ref.custom.ClipTestTimeTuning("cpu", bank.classnames, None, arch=student, n_ctx=n_ctx, ctx_init="a_photo_of_a", ctx_position="end")
    for name, p in model.named_parameters():
        if "prompt_learner" not in name:
            p.requires_grad_(False)
    optimizer = torch.optim.AdamW(model.prompt_learner.parameters(), hp["lr"], weight_decay=hp["weight_decay"])
    return model, optimizer, s_geo


def run_reference_prompt(ref, T, student, n_views, n_cls, hp, view_seed=1000, n_ctx=4):
    """the harness body TPT/tpt_cls.py:278-297 around the reference's own tpt_cls.test_time_tuning"""
    model, optimizer, s_geo = build_prompt_model(ref, student, n_cls, n_ctx, hp)
    args = types.SimpleNamespace(tta_steps=hp["tta_steps"], selection_p=hp["selection_p"], gpu=None, tpt=True, cocoop=False)
    views = synth.make_views(view_seed, n_views, s_geo.image_resolution)
    taps, undo = _taps(T.prompt)
    grads = []
    model.prompt_learner.ctx.register_hook(lambda g: grads.append(g.detach().clone()))
    model.eval()
    with torch.no_grad():
        model.reset()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        T.prompt.test_time_tuning(model, views, optimizer, _scaler(), args)
        with torch.no_grad():
            final = model(views[:1])
    undo()
    out = dict(logits=taps["logits"], selected_idx=taps["selected_idx"], loss=taps["loss"].reshape(1), dlogits=taps["dlogits"],
               ctx_grad=grads[0], ctx_after=model.prompt_learner.ctx.detach().clone(), final_logits=final,
               top5=torch.topk(final, min(5, n_cls), dim=-1).indices[0])
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def run_reference_tune(ref, T, student, n_views, n_cls, hp, only_norm, view_seed=1000, n_ctx=4, full_vectors=True):
    """the harness body TPT/tune_cls_tpt.py:207-222 around the reference's own CLIPCLS_TTA and tune_cls_tpt.test_time_tuning"""
    s_geo = synth.GEOMETRIES[student]
    s_sd = synth.make_state_dict(s_geo, seed=11)
    MG.install_models(ref, {student: (s_geo, s_sd)})
    bank = MG.Bank(s_geo, n_cls, n_ctx)
    ref.custom.tokenize = bank.tokenize
    model = ref.custom.CLIPCLS_TTA("cpu", bank.classnames, arch=student, prompt_prefix="a_photo_of_a", only_visual=True,
                                   momentum_update=False, only_norm=only_norm)
    names = [n for n, p in model.clip_model.visual.named_parameters() if not only_norm or "ln" in n or "bn" in n]
    if not only_norm:
        assert ["visual." + n for n in names] == RR.visual_param_keys(s_sd), "oracle key order != named_parameters order"
    pristine = {n: p.detach().clone() for n, p in model.clip_model.visual.named_parameters()}
    optimizer = torch.optim.AdamW(model.parameters(), hp["lr"], weight_decay=hp["weight_decay"])
    args = types.SimpleNamespace(tta_steps=hp["tta_steps"], selection_p=hp["selection_p"], gpu=None, tpt=True)
    views = synth.make_views(view_seed, n_views, s_geo.image_resolution)
    taps, undo = _taps(T.tune)
    pmap = dict(model.clip_model.visual.named_parameters())
    first_grads = {}

    def keep_first(n):
        def hook(g):
            first_grads.setdefault(n, g.detach().clone())
        return hook

    for n in names:
        pmap[n].register_hook(keep_first(n))
    model.reset()
    model.train()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        T.tune.test_time_tuning(model, views, optimizer, _scaler(), args, reward_model=None)
    model.eval()
    with torch.no_grad():
        final = model(views[:1])
    undo()
    out = dict(logits=taps["logits"], selected_idx=taps["selected_idx"], loss=taps["loss"].reshape(1), dlogits=taps["dlogits"],
               final_logits=final, top5=torch.topk(final, min(5, n_cls), dim=-1).indices[0])
    if only_norm:
        out.update(ln_grad=torch.cat([first_grads[n].reshape(-1) for n in names]),
                   ln_after=torch.cat([pmap[n].detach().reshape(-1) for n in names]))
    else:
        if full_vectors:
            out.update(vis_grad_sample=torch.cat([first_grads[n].reshape(-1) for n in names])[::7].clone(),
                       vis_after_sample=torch.cat([pmap[n].detach().reshape(-1) for n in names])[::7].clone())
        out.update(vis_grad_l2=torch.stack([first_grads[n].double().norm() for n in names]).float(),
                   vis_delta_l2=torch.stack([(pmap[n].detach() - pristine[n]).double().norm() for n in names]).float())
    return {k: v.detach().cpu().numpy() for k, v in out.items()}


def e2e_meta(student, n_views, n_cls, hp, kind):
    return dict(student=student, n_views=n_views, n_cls=n_cls, n_ctx=4, student_seed=11, bank_seed=7, view_seed=1000, kind=kind,
                only_norm=int(kind == "ln"), **hp)


def gen_e2e(ref, T):
    for name, (student, n_views, n_cls, over, kind) in E2E_CASES.items():
        hp = {**BASE_HP, **over}
        if kind == "prompt":
            out = run_reference_prompt(ref, T, student, n_views, n_cls, hp)
        else:
            full = hp["tta_steps"] == 1 and not synth.GEOMETRIES[student].is_resnet
            out = run_reference_tune(ref, T, student, n_views, n_cls, hp, kind == "ln", full_vectors=full)
        print(f"  {name}: loss {out['loss'][0]:.6g}  selected {out['selected_idx'].tolist()}  top5 {out['top5'].tolist()}")
        MG.save(name, out, e2e_meta(student, n_views, n_cls, hp, kind))


def gen_eval(ref, T, n_samples=3):
    """the per-sample body of tpt_cls.py:260-297 over n_samples synthetic test images (view seeds 2000 + i): reset, optimizer state
    reset, test_time_tuning, clean-view inference, top-5"""
    student, n_views, n_cls = "tiny", 8, 16
    hp = {**BASE_HP, "lr": 5e-3}
    model, optimizer, s_geo = build_prompt_model(ref, student, n_cls, 4, hp)
    optim_state = copy.deepcopy(optimizer.state_dict())
    args = types.SimpleNamespace(tta_steps=hp["tta_steps"], selection_p=hp["selection_p"], gpu=None, tpt=True, cocoop=False)
    scaler = _scaler()
    model.eval()
    with torch.no_grad():
        model.reset()
    top5, finals = [], []
    for i in range(n_samples):
        views = synth.make_views(2000 + i, n_views, s_geo.image_resolution)
        with torch.no_grad():
            model.reset()
        optimizer.load_state_dict(optim_state)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            T.prompt.test_time_tuning(model, views, optimizer, scaler, args)
        with torch.no_grad():
            out = model(views[:1])
        finals.append(out[0])
        top5.append(torch.topk(out, 5, dim=-1).indices[0])
    arrays = dict(top5=torch.stack(top5).numpy(), final_logits=torch.stack(finals).numpy())
    print(f"  tpt_eval_tiny: top5 {arrays['top5'].tolist()}")
    MG.save("tpt_eval_tiny", arrays, dict(student=student, n_views=n_views, n_cls=n_cls, n_ctx=4, student_seed=11, bank_seed=7,
                                          view_seed0=2000, n_samples=n_samples, kind="prompt", **hp))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ops,e2e,eval", help="comma list of ops / e2e / eval")
    a = ap.parse_args()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    ref = MG.import_reference()
    T = import_tpt(ref)
    parts = a.only.split(",")
    if "ops" in parts:
        gen_ops(T)
    if "e2e" in parts:
        gen_e2e(ref, T)
    if "eval" in parts:
        gen_eval(ref, T)


if __name__ == "__main__":
    main()
