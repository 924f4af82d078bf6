"""Host-side mirror of the retrieval distillation entry (retrieval/clip_ret_kd.py, run by retrieval/scripts/tta_coco_ret_kd.sh and
tta_flickr_ret_kd.sh): `kd_distill_loss_v2`, `tune_image` (:50-67), `tune_text` (:70-92) and `test_time_tune` (:95-150) with the
reference's signatures.

The step is the retrieval policy step of rlcf_amd.clip_ret_policy with the reward loss replaced by
kd_distill_loss_v2(student logits, teacher logits) over ALL rows of the query's logits: the teacher rows are the reward model's
calulate_similarity() (exp(reward.logit_scale) * reward features @ reward bank^T), computed once before the steps; there is no
top-K, no CLIPScore and no reward post-processing.  One engine call per query (rlcf_tta_retrieval_image_kd /
rlcf_tta_retrieval_text_kd).  An ensemble of reward models is refused: CLIPRewardsMultiple has no calulate_similarity.
"""
from __future__ import annotations

import torch

from . import _lib as L
from . import clip_ret_policy as _P
from . import clip_store, runtime
from .clip_ret_policy import CLIPRet_TTA, CLIPRewards, report_metrics  # noqa: F401
from .engine import TTAConfig
from .kd_losses import kd_distill_loss_v2  # noqa: F401  (the reference defines it in this module: same function)


def _cfg(optimizer, args) -> TTAConfig:
    g = optimizer.param_groups[0]
    b1, b2 = g.get("betas", (0.9, 0.999))
    return TTAConfig(selection_p=1.0, tta_steps=args.tta_steps, sample_k=1, lr=g["lr"], weight_decay=g.get("weight_decay", 0.0), beta1=b1, beta2=b2,
                     eps=g.get("eps", 1e-8), reward_process=False, process_batch=False, reward_amplify=False)


def _one_reward_model(reward_model):
    if isinstance(reward_model, _P.CLIPRewardsMultiple) or isinstance(getattr(reward_model, "image_features", None), (list, tuple)):
        raise NotImplementedError("CLIPRewardsMultiple has no calulate_similarity (retrieval/clip_reward.py): use one reward model")


def tune_image(image, model, reward_model, optimizer, scaler, args=None):
    """retrieval/clip_ret_kd.py:50-67.  `optimizer` supplies the AdamW hyper-parameters; `scaler` is accepted and unused (its inf /
    NaN step skip is built into the engine)."""
    _one_reward_model(reward_model)
    if not (torch.equal(model.ln.data, model._ln_init) and torch.equal(model.vis.data, model._vis_init)):
        raise NotImplementedError("tune_image starts from the reset state (model.reset_initial(), clip_ret_kd.py:132)")
    out = runtime.SESSION.engine(image.shape[0]).tta_retrieval_image_kd(image, _cfg(optimizer, args), skip_final=True)
    reward_model.image_features = out["reward_image_features"]            # reward_model.set_image_features(images=image), :55
    with torch.no_grad():
        model.ln.data.copy_(out["ln_after"])
        model.vis.data.copy_(out["vis_after"])
    return out


def tune_text(text, model, reward_model, optimizer, scaler, args=None):
    """retrieval/clip_ret_kd.py:70-92: `text` = one caption (bs = 1).  The image bank is model.image_features (student) and
    reward_model.image_features, set by the loop before the queries (:113-115)."""
    _one_reward_model(reward_model)
    if model.only_visual:
        raise ValueError("tune_text needs CLIPRet_TTA(only_visual=False)")
    if model.image_features is None or reward_model.image_features is None:
        raise L.RlcfError("tune_text: set_image_features of the model and of the reward model first (clip_ret_kd.py:113-115)")
    if not (torch.equal(model.ln.data, model._ln_init) and torch.equal(model.vis.data, model._vis_init)):
        raise NotImplementedError("tune_text starts from the reset state (model.reset_initial(), clip_ret_kd.py:147)")
    tok = clip_store.tokenize(text).reshape(1, -1)
    # the engine's bank follows the two feature tensors the loop set: version counters bumped by the setters (clip_ret_policy.tune_text)
    src = (getattr(model, "_img_version", None), getattr(reward_model, "_img_version", None), model.image_features.data_ptr(),
           reward_model.image_features.data_ptr(), tuple(model.image_features.shape))
    if runtime.SESSION.image_bank is None or None in src or getattr(runtime.SESSION, "_image_bank_src", None) != src:
        runtime.SESSION.set_image_bank(model.image_features, reward_model.image_features)
        runtime.SESSION._image_bank_src = src
    out = runtime.SESSION.engine().tta_retrieval_text_kd(tok[0], _cfg(optimizer, args))
    reward_model.class_features = out["reward_text_features"]             # reward_model.set_text_features(captions=text), :79
    with torch.no_grad():
        model.ln.data.copy_(out["ln_after"])
        model.vis.data.copy_(out["text_after"])
    model._tuned_query = (tok.cpu(), out["final_logits"])
    return out


def test_time_tune(data_loader, device, model, reward_model=None, scaler=None, optimizer=None, optim_state=None, text_bs=128, args=None):
    """retrieval/clip_ret_kd.py:95-150: the loop of clip_ret_policy.test_time_tune around the two distillation calls."""
    return _P._test_time_tune(tune_image, tune_text, data_loader, model, reward_model, scaler, optimizer, optim_state, text_bs, args)


test_time_tune.__test__ = False          # (the reference's name; not a test)
