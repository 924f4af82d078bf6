"""Host-side mirror of the TPT baseline's prompt-tuning entry (TPT/tpt_cls.py, run by TPT/scripts/tpt-prompt.sh): `select_confident_samples`
(:34-37), `avg_entropy` (:40-46), `test_time_tuning` (:49-78) and `test_time_adapt_eval` (:242-314) with the reference's signatures.

The step is the prompt step of rlcf_amd.tpt_cls_rl with the reward loss replaced by avg_entropy of the selected views
(rlcf_tta_sample with RLCF_F_TPT, the loss and its gradient from rlcf_tpt_loss): no reward model is built, run or asked for.
`args.tta_steps = 0`, which tpt-prompt.sh as shipped sets, is plain CLIP inference with the hand-written prompt.
CoCoOp (`args.cocoop`, TPT/clip/cocoop.py) is not built: its meta-net has no engine form.
"""
from __future__ import annotations

from . import tpt_cls_rl
from .tpt_cls_rl import accuracy, avg_entropy, select_confident_samples  # noqa: F401  (the names tpt_cls.py defines / imports)


def _no_cocoop(args) -> None:
    if getattr(args, "cocoop", False):
        raise NotImplementedError("CoCoOp (args.cocoop, TPT/clip/cocoop.py) is not built: the meta-net has no engine form")


def test_time_tuning(model, inputs, optimizer, scaler, args):
    """TPT/tpt_cls.py:49-78: selection at step 0, tta_steps AdamW steps on avg_entropy of the selected views (the GradScaler step
    skip on a non-finite gradient kept)."""
    _no_cocoop(args)
    return tpt_cls_rl.test_time_tuning(model, inputs, optimizer, scaler, args, reward_model=None, tpt=True)


def test_time_adapt_eval(val_loader, model, model_state, optimizer, optim_state, scaler, args):
    """TPT/tpt_cls.py:242-314: per test image reset -> test_time_tuning -> clean-view inference -> top-1 / top-5.  `model_state` is
    accepted and unused, as in the reference.  Returns [top1, top5] in percent."""
    _no_cocoop(args)
    return tpt_cls_rl.test_time_adapt_eval(val_loader, model, optimizer, optim_state, scaler, args, reward_model=None, tpt=True)
