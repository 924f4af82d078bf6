"""Host-side mirror of the distillation entry (TPT/tune_cls_kd.py, run by TPT/scripts/kd-tune.sh): `test_time_tuning` (:34-61) and
`test_time_adapt_eval` (:191-236) with the reference's signatures.

The step is the CLIPCLS_TTA step of rlcf_amd.tpt_cls_rl with the reward loss replaced by `args.kd_loss` (KD / DKD / ATKD):
per test image the engine selects the confident views, computes the reward model's logits of the selected views once
(reward_model.calulate_similarity(), tune_cls_kd.py:45-46), and distils them into the student for tta_steps AdamW steps
(rlcf_tta_sample_ln / rlcf_tta_sample_visual with RLCF_F_KD / DKD / ATKD).  One test image per engine call: the batched and
in-flight forms of the RL loop are not offered here, and neither are an ensemble of reward models (CLIPRewardsMultiple has no
calulate_similarity, clip_reward.py:180-307) nor a prompt learner (the reference tunes CLIPCLS_TTA only).
"""
from __future__ import annotations

from . import tpt_cls_rl
from .clip_reward import CLIPRewardsMultiple
from .engine import kd_flag
from .kd_losses import atkd_distill_loss, dkd_distill_loss, kd_distill_loss_v2  # noqa: F401  (the names tune_cls_kd.py imports)
from .tpt_cls_rl import accuracy, select_confident_samples  # noqa: F401


def _kd_loss(model, args, reward_model) -> str:
    kind = getattr(args, "kd_loss", None)
    kd_flag(kind)                                               # NotImplementedError on anything but KD / DKD / ATKD (tune_cls_kd.py:55)
    if kind is None:
        raise NotImplementedError("args.kd_loss is not set")
    if reward_model is None:
        raise ValueError("the distillation losses need the reward model (get_reward_model)")
    if isinstance(reward_model, CLIPRewardsMultiple):
        raise NotImplementedError("CLIPRewardsMultiple has no calulate_similarity (clip_reward.py:180-307): use --multiple_reward_models 0")
    if hasattr(model, "prompt_learner"):
        raise NotImplementedError("tune_cls_kd.py tunes the image encoder (CLIPCLS_TTA), not a prompt learner")
    return kind


def test_time_tuning(model, inputs, optimizer, scaler, args, reward_model=None):
    """TPT/tune_cls_kd.py:34-61: selection at step 0, the teacher computed once from the selected views, tta_steps distillation
    steps (the GradScaler step skip on a non-finite gradient as in the RL path).  model.train() is the caller's, as in the reference."""
    kind = _kd_loss(model, args, reward_model)
    return tpt_cls_rl.test_time_tuning(model, inputs, optimizer, scaler, args, reward_model=reward_model, kd_loss=kind)


def test_time_adapt_eval(val_loader, model, optimizer, optim_state, scaler, args, device=None, reward_model=None):
    """TPT/tune_cls_kd.py:191-236: per test image reset -> model.train() -> test_time_tuning -> model.eval() -> clean-view inference
    -> momentum_update_model -> top-1 / top-5.  Returns [top1, top5] in percent."""
    kind = _kd_loss(model, args, reward_model)
    for name in ("images_per_pass", "in_flight"):
        if int(getattr(args, name, None) or 1) > 1:
            raise NotImplementedError(f"{name} > 1: the distillation losses run one test image per engine call")
    return tpt_cls_rl.test_time_adapt_eval(val_loader, model, optimizer, optim_state, scaler, args, device=device, reward_model=reward_model,
                                           images_per_pass=1, in_flight=1, kd_loss=kind)
