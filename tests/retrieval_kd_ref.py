"""CPU restatement of the retrieval distillation step (retrieval/clip_ret_kd.py:37-92) for the tests: oracle.clip_ref / oracle.rlcf_ref /
oracle.retrieval_ref pieces plus the four-line loss.  Pinned to the reference's own run by the retkd_* fixtures
(tests/test_retrieval_kd_golden.py); the GPU tests compare the engine against it where no fixture exists."""
from __future__ import annotations

import os
from typing import Dict, Optional

import numpy as np
import torch

from oracle import clip_ref as C
from oracle import retrieval_ref as QR
from oracle import rlcf_ref as RR


def kd_distill_loss_v2(logits_student, logits_teacher, T_stu=1.0, T_tea=1.0):
    log_q = torch.log_softmax(logits_student / T_stu, dim=1)
    p_t = torch.softmax(logits_teacher / T_tea, dim=1)
    return -(p_t * log_q).sum(dim=1).mean() * T_stu * T_stu


def _tune(keys, student_sd, logits_of, teacher, hp, first_row_only) -> Dict[str, torch.Tensor]:
    params = {k: student_sd[k].clone() for k in keys}
    m = {k: torch.zeros_like(v) for k, v in params.items()}
    v2 = {k: torch.zeros_like(v) for k, v in params.items()}
    out: Dict[str, torch.Tensor] = {"teacher": teacher}
    for j in range(hp.tta_steps):
        prm = {k: p.detach().requires_grad_(True) for k, p in params.items()}
        lg = logits_of(prm)
        loss = kd_distill_loss_v2(lg, teacher)
        grads = torch.autograd.grad(loss, [prm[k] for k in keys] + [lg])
        if j == 0:
            out.update(logits=lg.detach(), loss=loss.detach().clone(), dlogits=grads[-1].clone(), grad=torch.cat([g.reshape(-1) for g in grads[:-1]]))
        with torch.no_grad():
            for k, g in zip(keys, grads[:-1]):
                params[k], m[k], v2[k] = RR.adamw_step(prm[k].detach(), g, m[k], v2[k], j + 1, hp)
    with torch.no_grad():
        fl = logits_of(params)
        out["final_logits"] = fl[:1] if first_row_only else fl
    out["after"] = torch.cat([params[k].reshape(-1) for k in keys])
    return out


def tune_image(student_sd, reward_sd, images, caption_tokens, hp, cap_feat: Optional[torch.Tensor] = None,
               reward_text: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """clip_ret_kd.py:50-67 + the evaluation of its loop: teacher = exp(reward.logit_scale) * reward image features @ reward caption
    bank^T once, then tta_steps of KD over all rows of logits_per_image; every visual parameter tuned."""
    with torch.no_grad():
        if reward_text is None:
            reward_text = RR.reward_class_features(reward_sd, caption_tokens)
        if cap_feat is None:
            cap_feat = C.l2_normalize(C.encode_text(student_sd, caption_tokens))
        teacher = reward_sd["logit_scale"].exp() * RR.reward_image_features(reward_sd, images) @ reward_text.t()
    scale = student_sd["logit_scale"].exp()

    def logits_per_image(prm):
        sd = dict(student_sd)
        sd.update(prm)
        return scale * C.l2_normalize(C.encode_image(sd, images)) @ cap_feat.t()

    return _tune(RR.visual_param_keys(student_sd), student_sd, logits_per_image, teacher, hp, True)


def tune_text(student_sd, reward_sd, query_tokens, bank_images, hp, student_bank: Optional[torch.Tensor] = None,
              reward_bank: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """clip_ret_kd.py:70-92 + the evaluation of its loop: teacher = exp(reward.logit_scale) * reward text feature @ reward image
    bank^T once, then tta_steps of KD on logits_per_text [1, n_images]; every non-visual parameter tuned."""
    with torch.no_grad():
        if student_bank is None:
            student_bank = C.l2_normalize(C.encode_image(student_sd, bank_images))
        if reward_bank is None:
            reward_bank = RR.reward_image_features(reward_sd, bank_images)
        rtxt = RR.reward_class_features(reward_sd, query_tokens)
        teacher = reward_sd["logit_scale"].exp() * rtxt @ reward_bank.t()

    def logits_per_text(prm):
        sd = dict(student_sd)
        sd.update(prm)
        return sd["logit_scale"].exp() * C.l2_normalize(C.encode_text(sd, query_tokens)) @ student_bank.t()

    out = _tune(QR.text_param_keys(student_sd), student_sd, logits_per_text, teacher, hp, False)
    out["reward_text"] = rtxt
    return out


# ------------------------------------------------------------------ seeded inputs shared by the fixture generator and the tests
METRIC_KEYS = ("txt_r1", "txt_r5", "txt_r10", "txt_r_mean", "img_r1", "img_r5", "img_r10", "img_r_mean", "r_mean", "agg_metrics")
# retkd_ops cases: (n, C, T_stu, T_tea, seed).  1025, 5 000 and 25 010 are no multiples of the split kernel's chunk (1024 elements).
OPS_CASES = [(1, 1, 1.0, 1.0, 1), (1, 37, 1.0, 1.0, 2), (2, 37, 1.0, 1.0, 3), (1, 1025, 1.0, 1.0, 4), (1, 5000, 1.0, 1.0, 5), (2, 5000, 1.0, 1.0, 6),
             (1, 25010, 1.0, 1.0, 7), (2, 25010, 2.0, 4.0, 8), (1, 65536, 1.0, 1.0, 9), (1, 5000, 0.5, 3.0, 10)]


def ops_rows(n, C, seed):
    """seeded student / teacher rows at CLIP logit scale (100 x a cosine)"""
    g = torch.Generator().manual_seed(1000 + seed)
    s = 100.0 * (0.2 + 0.05 * torch.randn(n, C, generator=g))
    t = 100.0 * (0.2 + 0.05 * torch.randn(n, C, generator=g))
    return s.float(), t.float()


def ops_cases():
    """(case index, n, C, T_stu, T_tea, seed, fixture arrays) of tests/golden/retkd_ops.npz"""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "retkd_ops.npz"))
    g = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("meta_")}
    for i, (n, C, ts, tt, seed) in enumerate(z["meta_cases"].tolist()):
        yield i, int(n), int(C), float(ts), float(tt), int(seed), g


def random_scores(seed, n_img=40, per=5):
    """two score matrices, tie-free by construction: a permutation of distinct values per matrix, half of the ground-truth entries
    lifted above the range (k / 64 + 200: still distinct) so the recalls are not all ~0"""
    rng = np.random.RandomState(seed)
    n_txt = n_img * per
    a = rng.permutation(n_img * n_txt).reshape(n_img, n_txt).astype(np.float32) / 64.0
    b = rng.permutation(n_img * n_txt).reshape(n_txt, n_img).astype(np.float32) / 64.0
    txt2img = [k // per for k in range(n_txt)]
    img2txt = [list(range(k * per, (k + 1) * per)) for k in range(n_img)]
    for k in range(n_txt):
        if rng.rand() < 0.5:
            a[txt2img[k], k] += 200.0
        if rng.rand() < 0.5:
            b[k, txt2img[k]] += 200.0
    for m in (a, b):
        assert all(len(np.unique(r)) == len(r) for r in m)
    return a, b, txt2img, img2txt
