"""Host-side mirror of the TPT baseline's image-encoder entry (TPT/tune_cls_tpt.py, run by TPT/scripts/tpt-tune.sh): `test_time_tuning`
(:34-54) and `test_time_adapt_eval` (:184-240) with the reference's signatures.

The step is the CLIPCLS_TTA step of rlcf_amd.tpt_cls_rl with the reward loss replaced by avg_entropy of the selected views
(rlcf_tta_sample_ln / rlcf_tta_sample_visual with RLCF_F_TPT).  The reference's main_worker sets `reward_model = None`; a reward
model that is passed all the same is not run (the reference would only store its image features, which nothing reads).
"""
from __future__ import annotations

from . import tpt_cls_rl
from .tpt_cls_rl import accuracy, avg_entropy, select_confident_samples  # noqa: F401  (the names tune_cls_tpt.py imports)


def test_time_tuning(model, inputs, optimizer, scaler, args, reward_model=None):
    """TPT/tune_cls_tpt.py:34-54.  model.train() is the caller's, as in the reference."""
    return tpt_cls_rl.test_time_tuning(model, inputs, optimizer, scaler, args, reward_model=reward_model, tpt=True)


def test_time_adapt_eval(val_loader, model, optimizer, optim_state, scaler, args, device=None, reward_model=None):
    """TPT/tune_cls_tpt.py:184-240: per test image reset -> model.train() -> test_time_tuning -> model.eval() -> clean-view inference
    -> momentum_update_model -> top-1 / top-5.  Returns [top1, top5] in percent."""
    return tpt_cls_rl.test_time_adapt_eval(val_loader, model, optimizer, optim_state, scaler, args, device=device, reward_model=reward_model,
                                           tpt=True)
