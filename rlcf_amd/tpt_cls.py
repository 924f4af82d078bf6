"""Host-side mirror of the TPT baseline's prompt-tuning entry (TPT/tpt_cls.py, run by TPT/scripts/tpt-prompt.sh): `select_confident_samples`
(:34-37), `avg_entropy` (:40-46), `test_time_tuning` (:49-78) and `test_time_adapt_eval` (:242-314) with the reference's signatures.

The step is the prompt step of rlcf_amd.tpt_cls_rl with the reward loss replaced by avg_entropy of the selected views
(rlcf_tta_sample with RLCF_F_TPT, the loss and its gradient from rlcf_tpt_loss): no reward model is built, run or asked for.
`args.tta_steps = 0`, which tpt-prompt.sh as shipped sets, is plain CLIP inference with the hand-written prompt.

`args.cocoop` (TPT/clip/cocoop.py) takes a model from rlcf_amd.cocoop.get_cocoop: per test image a prompt is generated from the clean
view's features, tuned for at most ONE step and used for the final logits (rlcf_tta_sample_cocoop).  The reference has no second
step: there its test_time_tuning indexes the (features, ctx) tuple (TPT/tpt_cls.py:60) and stops with a TypeError.
"""
from __future__ import annotations

import time

import torch

from . import tpt_cls_rl
from .engine import TTAConfig
from .tpt_cls_rl import accuracy, avg_entropy, select_confident_samples  # noqa: F401  (the names tpt_cls.py defines / imports)

COCOOP_WEIGHT_DECAY = 0.01      # torch.optim.AdamW([pgen_ctx], args.lr) (TPT/tpt_cls.py:53): every other setting is torch's default


def _cocoop_model(model, args) -> bool:
    """True: the CoCoOp path.  `args.cocoop` with any other model (a ClipTestTimeTuning, None) has nothing to run on."""
    if not getattr(args, "cocoop", False):
        return False
    from .cocoop import CoCoOpCLIP
    if not isinstance(model, CoCoOpCLIP):
        raise NotImplementedError("args.cocoop (TPT/clip/cocoop.py) needs a model from rlcf_amd.cocoop.get_cocoop; "
                                  f"got {type(model).__name__}")
    if args.tta_steps > 1:
        raise NotImplementedError(f"args.cocoop with tta_steps = {args.tta_steps}: CoCoOp exists for 0 or 1 steps only (at a second step "
                                  "the reference indexes its (features, ctx) tuple, TPT/tpt_cls.py:60, and stops with a TypeError)")
    return True


def _cocoop_config(args) -> TTAConfig:
    return TTAConfig(selection_p=args.selection_p, tta_steps=args.tta_steps, lr=args.lr, weight_decay=COCOOP_WEIGHT_DECAY, tpt=True)


def test_time_tuning(model, inputs, optimizer, scaler, args):
    """TPT/tpt_cls.py:49-78: selection at step 0, tta_steps AdamW steps on avg_entropy of the selected views (the GradScaler step
    skip on a non-finite gradient kept).  With args.cocoop `inputs` is (image_feature, pgen_ctx) and the tuned pgen_ctx is returned
    (rlcf_tta_sample_feats, final logits skipped); `optimizer` is unused there, as in the reference (:53 makes its own)."""
    if _cocoop_model(model, args):
        image_feature, pgen_ctx = inputs
        if args.tta_steps <= 0:
            return pgen_ctx
        eng = model._engine(image_feature.shape[0])
        out = eng.tta_sample_feats(image_feature, pgen_ctx.reshape(eng.n_ctx, -1), _cocoop_config(args), want_intermediates=False,
                                   skip_final=True)
        return out["ctx_after"].reshape(pgen_ctx.shape)
    return tpt_cls_rl.test_time_tuning(model, inputs, optimizer, scaler, args, reward_model=None, tpt=True)


def _cocoop_eval(val_loader, model, args):
    """The loop body TPT/tpt_cls.py:280-297 with args.cocoop: gen_ctx on the views, the step, the final logits on view 0 — one fused
    engine call per test image (rlcf_tta_sample_cocoop), the hits counted on the device from its top-5."""
    images_per_pass = tpt_cls_rl._loop_option(None, args, "images_per_pass")
    in_flight = tpt_cls_rl._loop_option(None, args, "in_flight")
    if images_per_pass > 1 or in_flight > 1:
        raise NotImplementedError("args.cocoop runs one test image per engine call (images_per_pass = in_flight = 1)")
    if not args.tpt:
        raise NotImplementedError("args.cocoop with args.tpt = False (a batch of test images, gen_ctx(aug=False) on its mean feature) has no "
                                  "loop here; CoCoOpCLIP.gen_ctx(images, aug=False) itself works")
    cfg = _cocoop_config(args)
    model.eval()
    n, hits = 0, None
    end = time.time()
    for i, (images, target) in enumerate(val_loader):
        assert args.gpu is not None
        if isinstance(images, list):
            images = torch.cat([im.cuda(args.gpu, non_blocking=True) for im in images], dim=0)          # tpt_cls.py:258-261,271
        else:
            images = (images.squeeze(0) if images.dim() > 4 else images).cuda(args.gpu, non_blocking=True)
        eng = model._engine(images.shape[0])
        out = eng.tta_sample_cocoop(images, cfg, want_intermediates=False)
        if hits is None:
            hits = torch.zeros(2, device=out["top5"].device)
        tpt_cls_rl._hits(out["top5"].reshape(1, 5), [target], hits)
        n += 1
        if (i + 1) % getattr(args, "print_freq", 500) == 0:
            print(f"Test: [{i + 1}/{len(val_loader)}] Time {time.time() - end:6.3f} Acc@1 {float(hits[0]) * 100 / n:6.2f} Acc@5 {float(hits[1]) * 100 / n:6.2f}")
        elif (i + 1) % 32 == 0:
            torch.cuda.current_stream().synchronize()                # (bounds how far the host runs ahead of the device)
        end = time.time()
    s1, s5 = (float(hits[0]) * 100.0, float(hits[1]) * 100.0) if n else (0.0, 0.0)
    return [round(x, 3) for x in [s1 / max(n, 1), s5 / max(n, 1)]]


def test_time_adapt_eval(val_loader, model, model_state, optimizer, optim_state, scaler, args):
    """TPT/tpt_cls.py:242-314: per test image reset -> test_time_tuning -> clean-view inference -> top-1 / top-5.  `model_state` is
    accepted and unused, as in the reference.  Returns [top1, top5] in percent.  With args.cocoop nothing is reset ("it's fixed",
    :251,274): a prompt is generated per image instead."""
    if _cocoop_model(model, args):
        return _cocoop_eval(val_loader, model, args)
    return tpt_cls_rl.test_time_adapt_eval(val_loader, model, optimizer, optim_state, scaler, args, reward_model=None, tpt=True)
