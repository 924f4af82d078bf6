"""Generate the distillation fixtures (TPT/tune_cls_kd.py, utils/{KD,DKD,ATKD}.py): the reference itself, imported read-only as
make_golden.py imports it, run on CPU in float32 on this repo's seeded synthetic weights, views and class banks.

  kd_ops.npz              op level: CLIP-like logit rows (100 * cosine, row means ~10-30) for C in {1, 37, 200, 1000} and edge rows
                          (teacher tie at the argmax, student p_target -> 1, negative row means for ATKD, one non-default
                          hyper-parameter set per loss): the reference loss, its autograd dlogits in float32 and in float64
  kd_<case>_<loss>.npz    end to end: the reference's own tune_cls_kd.test_time_tuning on CLIPCLS_TTA (only_norm = 1 for the `ln`
                          cases, 0 for `vis` / `rn`), one file per loss
  kd_eval_tiny.npz        a few test images through the tune_cls_kd.py:191-236 loop body: per-sample top-5

Every end-to-end case prints min |row mean| of the student rows the loss sees: ATKD divides by it (see rlcf_amd/kd_losses.py).
Usage: python tests/golden/make_kd_golden.py [--only ops|e2e|full|eval]
"""
from __future__ import annotations

import argparse
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

LOSSES = ("KD", "DKD", "ATKD")


def import_kd(ref):
    import importlib
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kd = importlib.import_module("tune_cls_kd")
    from utils import KD, DKD, ATKD
    return types.SimpleNamespace(entry=kd, KD=KD, DKD=DKD, ATKD=ATKD)


# ------------------------------------------------------------------ op level
def clip_rows(seed, n, C, mean_lo=0.1, mean_hi=0.3, spread=0.04):
    """100 * cosine-like rows: per-row mean in [mean_lo, mean_hi] * 100, spread 100 * `spread`"""
    g = torch.Generator().manual_seed(seed)
    mu = mean_lo + (mean_hi - mean_lo) * torch.rand(n, 1, generator=g)
    return (100.0 * (mu + spread * torch.randn(n, C, generator=g))).float()


def op_cases():
    cases = {}
    for C in (1, 37, 200, 1000):
        s = clip_rows(100 + C, 4, C)
        t = (0.5 * s + 0.5 * clip_rows(200 + C, 4, C)).float()
        cases[f"c{C}"] = (s, t, None)
    s, t = clip_rows(301, 3, 37), clip_rows(302, 3, 37)
    t[:, 5] = t.max(dim=1).values + 1.0
    t[:, 20] = t[:, 5]                       # two equal maxima: the first is the DKD target
    cases["tie"] = (s, t, None)
    s, t = clip_rows(311, 3, 200), clip_rows(312, 3, 200)
    g = t.argmax(dim=1)
    s[torch.arange(3), g] = s.max(dim=1).values + 22.0      # student p_target ~ 1 - 200 * e^-22: p_other ~ 6e-8
    cases["pgt1"] = (s, t, None)
    s, t = clip_rows(321, 3, 200, -0.3, -0.1), clip_rows(322, 3, 200, -0.25, -0.05)   # ATKD: negative row means
    cases["negmean"] = (s, t, None)
    hp = {"KD": dict(T_stu=2.0, T_tea=4.0), "DKD": dict(alpha=0.5, beta=2.0, temperature=2.0), "ATKD": dict(multiplier=1.5, eps=1e-3)}
    s, t = clip_rows(331, 4, 200), clip_rows(332, 4, 200)
    cases["hp"] = (s, t, hp)
    return cases


def run_loss(K, kind, s, t, hp, dtype):
    x = s.to(dtype).clone().requires_grad_(True)
    y = t.to(dtype)
    hp = hp or {}
    if kind == "KD":
        loss = K.KD.kd_distill_loss_v2(x, y, **hp)
    elif kind == "DKD":
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            loss = K.DKD.dkd_distill_loss(x, y, y.argmax(-1), **hp)
    else:
        loss = K.ATKD.atkd_distill_loss(x, y, **hp)
    loss.backward()
    return loss.detach(), x.grad.detach()


def gen_ops(K):
    arrays, meta = {}, {}
    names = []
    for name, (s, t, hp) in op_cases().items():
        arrays[name + "_s"], arrays[name + "_t"] = s.numpy(), t.numpy()
        names.append(name)
        for kind in LOSSES:
            if hp is not None and kind not in hp:
                continue
            if kind == "DKD" and s.shape[1] == 1:
                continue                     # (one class: no non-target class, p_other = 0 and the reference's log gives -inf)
            h = hp[kind] if hp else None
            l32, d32 = run_loss(K, kind, s, t, h, torch.float32)
            l64, d64 = run_loss(K, kind, s, t, h, torch.float64)
            key = f"{name}_{kind}"
            arrays[key + "_loss"], arrays[key + "_dlog"] = l32.numpy(), d32.numpy()
            arrays[key + "_loss64"], arrays[key + "_dlog64"] = l64.numpy(), d64.numpy()
            if h:
                for k, v in h.items():
                    meta[f"{key}_{k}"] = v
            mean_abs = s.double().mean(dim=1).abs().min().item()
            print(f"  {key:16s} loss {l32.item():.6g} (f64 {l64.item():.6g})  min|row mean| {mean_abs:.3g}")
    meta["cases"] = ",".join(names)
    MG.save("kd_ops", arrays, meta)


# ------------------------------------------------------------------ end to end
E2E_CASES = {      # name -> (student, reward, views, classes, overrides, only_norm)
    "kd_tiny_ln_s1": ("tiny", "tiny-r", 8, 16, dict(lr=1e-3), True),
    "kd_tiny_ln_s3": ("tiny", "tiny-r", 8, 16, dict(lr=1e-3, tta_steps=3), True),
    "kd_tiny_vis_s1": ("tiny", "tiny-r", 8, 16, dict(lr=1e-4), False),
    "kd_tiny_vis_s3": ("tiny", "tiny-r", 8, 16, dict(lr=1e-4, tta_steps=3), False),
    "kd_tiny_rn_s1": ("tiny-rn", "tiny-r", 8, 16, dict(lr=1e-4), False),
}
FULL_CASES = {     # scripts/kd-tune.sh: ViT-B/16 student, ViT-L/14 reward, N = 64, selection_p 0.1, 3 steps, lr 1e-5, tune_norm 0
    "kd_b16_l14_vis_s3_n64": ("ViT-B/16", "ViT-L/14", 64, 1000, dict(lr=1e-5, tta_steps=3, selection_p=0.1), False, "KD"),
}
BASE_HP = dict(lr=1e-4, weight_decay=5e-4, sample_k=3, tta_steps=1, selection_p=0.5)


def run_reference_kd(ref, K, student, reward, n_views, n_cls, hp, only_norm, kind, view_seed=1000, n_ctx=4, full_vectors=True):
    """TPT/tune_cls_kd.py harness body (:215-230) around the reference's own CLIPCLS_TTA and tune_cls_kd.test_time_tuning."""
    s_geo, r_geo = synth.GEOMETRIES[student], synth.GEOMETRIES[reward]
    s_sd = synth.make_state_dict(s_geo, seed=11)
    r_sd = synth.make_state_dict(r_geo, seed=23)
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
    args = types.SimpleNamespace(tta_steps=hp["tta_steps"], selection_p=hp["selection_p"], kd_loss=kind, gpu=None, tpt=True)
    MG.install_models(ref, {reward: (r_geo, r_sd)})
    rm = ref.clip_reward.CLIPRewards("cpu", arch=reward, classification=True, amplify_rewards=False, sample_k=hp["sample_k"],
                                     reward_process=True, process_batch=False)
    rm.set_class_features(tokenized_classes=model.tokenized_prompts)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scaler = torch.cuda.amp.GradScaler(init_scale=1000)
    views = synth.make_views(view_seed, n_views, s_geo.image_resolution)
    taps = {}
    orig_select = K.entry.select_confident_samples

    def tap_select(logits, top):
        out, idx = orig_select(logits, top)
        if "logits" not in taps:
            taps["logits"], taps["selected_idx"] = logits.detach().clone(), idx.clone()
        return out, idx

    orig_sim = rm.calulate_similarity

    def tap_sim():
        r = orig_sim()
        taps.setdefault("teacher", r[0].detach().clone())
        taps.setdefault("reward_image_features", rm.image_features.detach().clone())
        return r

    loss_fns = {"KD": "kd_distill_loss_v2", "DKD": "dkd_distill_loss", "ATKD": "atkd_distill_loss"}
    orig_loss = getattr(K.entry, loss_fns[kind])

    def tap_loss(out, teacher, *a, **k):
        loss = orig_loss(out, teacher, *a, **k)
        if "loss" not in taps:
            taps["loss"] = loss.detach().clone()
            taps["sel_logits"] = out.detach().clone()
            def keep(g):                 # must return None: a returned tensor would replace the gradient
                taps.setdefault("dlogits", g.detach().clone())
            out.register_hook(keep)
        return loss

    K.entry.select_confident_samples = tap_select
    rm.calulate_similarity = tap_sim
    setattr(K.entry, loss_fns[kind], tap_loss)
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
        K.entry.test_time_tuning(model, views, optimizer, scaler, args, reward_model=rm)
    model.eval()
    with torch.no_grad():
        final = model(views[:1])
    K.entry.select_confident_samples = orig_select
    setattr(K.entry, loss_fns[kind], orig_loss)
    out = dict(logits=taps["logits"], selected_idx=taps["selected_idx"], teacher=taps["teacher"], loss=taps["loss"].reshape(1),
               dlogits=taps["dlogits"], reward_image_features=taps["reward_image_features"], final_logits=final,
               top5=torch.topk(final, min(5, n_cls), dim=-1).indices[0])
    if only_norm:
        out.update(ln_grad=torch.cat([first_grads[n].reshape(-1) for n in names]),
                   ln_after=torch.cat([pmap[n].detach().reshape(-1) for n in names]))
    else:
        if full_vectors:
            out.update(vis_grad_sample=torch.cat([first_grads[n].reshape(-1) for n in names])[::7].clone(),
                       vis_after_sample=torch.cat([pmap[n].detach().reshape(-1) for n in names])[::7].clone())
        out.update(vis_grad_l2=torch.stack([first_grads[n].double().norm() for n in names]).float(),
                   vis_delta_l2=torch.stack([(pmap[n].detach() - pristine[n]).double().norm() for n in names]).float())
    cond = taps["sel_logits"].double().mean(dim=1).abs().min().item()
    return {k: v.detach().cpu().numpy() for k, v in out.items()}, cond


def e2e_meta(student, reward, n_views, n_cls, hp, only_norm, kind, cond):
    return dict(student=student, reward=reward, n_views=n_views, n_cls=n_cls, n_ctx=4, student_seed=11, reward_seed=23, bank_seed=7,
                view_seed=1000, only_norm=int(only_norm), kd_loss=kind, min_abs_row_mean=cond, **hp)


def gen_e2e(ref, K, cases, kinds=LOSSES):
    for name, spec in cases.items():
        student, reward, n_views, n_cls, over, only_norm = spec[:6]
        for kind in (spec[6:] or kinds):
            hp = {**BASE_HP, **over}
            # every 7th element of the vectors for the one-step ViT cases (the others: per-tensor norms, as make_golden.py keeps them)
            full = n_cls <= 64 and hp["tta_steps"] == 1 and not synth.GEOMETRIES[student].is_resnet
            out, cond = run_reference_kd(ref, K, student, reward, n_views, n_cls, hp, only_norm, kind, full_vectors=full)
            print(f"  {name}_{kind.lower()}: loss {out['loss'][0]:.6g}  min|row mean| of the student rows {cond:.4g}  top5 {out['top5'].tolist()}")
            if n_cls > 64:
                out.pop("teacher")       # (the full-size case: the reward image features pin the teacher; keeps the file small)
                out["logits"] = out["logits"][:, :64]
                out["dlogits_l2"] = np.linalg.norm(out["dlogits"].astype(np.float64), axis=1).astype(np.float32)
                out["dlogits"] = out["dlogits"][:, ::7].copy()
                out["reward_image_features"] = out["reward_image_features"][:, ::7].copy()
            MG.save(f"{name}_{kind.lower()}", out, e2e_meta(student, reward, n_views, n_cls, hp, only_norm, kind, cond))


def gen_eval(ref, K, n_samples=3):
    """the per-sample body of tune_cls_kd.py:198-236 over n_samples synthetic test images (view seeds 2000 + i): reset, optimizer
    state reset, train -> test_time_tuning -> eval, clean-view inference, top-5"""
    import copy
    student, reward, n_views, n_cls = "tiny", "tiny-r", 8, 16
    hp = {**BASE_HP, "lr": 1e-4}
    s_geo, r_geo = synth.GEOMETRIES[student], synth.GEOMETRIES[reward]
    MG.install_models(ref, {student: (s_geo, synth.make_state_dict(s_geo, seed=11))})
    bank = MG.Bank(s_geo, n_cls, 4)
    ref.custom.tokenize = bank.tokenize
    model = ref.custom.CLIPCLS_TTA("cpu", bank.classnames, arch=student, prompt_prefix="a_photo_of_a", only_visual=True,
                                   momentum_update=False, only_norm=False)
    optimizer = torch.optim.AdamW(model.parameters(), hp["lr"], weight_decay=hp["weight_decay"])
    optim_state = copy.deepcopy(optimizer.state_dict())
    MG.install_models(ref, {reward: (r_geo, synth.make_state_dict(r_geo, seed=23))})
    rm = ref.clip_reward.CLIPRewards("cpu", arch=reward, classification=True, amplify_rewards=False, sample_k=hp["sample_k"],
                                     reward_process=True, process_batch=False)
    rm.set_class_features(tokenized_classes=model.tokenized_prompts)
    args = types.SimpleNamespace(tta_steps=hp["tta_steps"], selection_p=hp["selection_p"], kd_loss="DKD", gpu=None, tpt=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scaler = torch.cuda.amp.GradScaler(init_scale=1000)
    top5, finals = [], []
    for i in range(n_samples):
        views = synth.make_views(2000 + i, n_views, s_geo.image_resolution)
        model.reset()
        optimizer.load_state_dict(optim_state)
        model.train()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            K.entry.test_time_tuning(model, views, optimizer, scaler, args, reward_model=rm)
        model.eval()
        with torch.no_grad():
            out = model(views[:1])
        finals.append(out[0])
        top5.append(torch.topk(out, 5, dim=-1).indices[0])
    arrays = dict(top5=torch.stack(top5).numpy(), final_logits=torch.stack(finals).numpy())
    print(f"  kd_eval_tiny: top5 {arrays['top5'].tolist()}")
    MG.save("kd_eval_tiny", arrays, dict(student=student, reward=reward, n_views=n_views, n_cls=n_cls, n_ctx=4, student_seed=11,
                                         reward_seed=23, bank_seed=7, view_seed0=2000, n_samples=n_samples, kd_loss="DKD", **hp))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ops,e2e,eval", help="comma list of ops / e2e / eval / full")
    a = ap.parse_args()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    ref = MG.import_reference()
    K = import_kd(ref)
    parts = a.only.split(",")
    if "ops" in parts:
        gen_ops(K)
    if "e2e" in parts:
        gen_e2e(ref, K, E2E_CASES)
    if "eval" in parts:
        gen_eval(ref, K)
    if "full" in parts:
        gen_e2e(ref, K, FULL_CASES)


if __name__ == "__main__":
    main()
