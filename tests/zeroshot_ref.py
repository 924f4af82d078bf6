"""Numpy restatement of the zero-shot mixing expression (TPT/clip/custom_clip.py:555-566: per model `logit_scale.exp() * img @ txt.t()`,
then the mean over the models) and of top-5 with ties to the lower index, plus the seeded inputs of the tests/golden/zeroshot_ops.npz
cases (tests/golden/make_zeroshot_golden.py::op_inputs).  Test infrastructure only."""
from __future__ import annotations

import numpy as np
import torch

from rlcf_amd import synth
from tpt_ref import load_golden  # noqa: F401

LOGIT_BAR = 1e-3                      # the logits bar of the GPU end-to-end tests (tests/test_gpu_tpt.py::_check_e2e)
SCALES = (100.0, 1.0 / 0.07, 50.0, 100.0, 25.0)      # exp(logit_scale) of model m: CLIP's trained value, its initial value, others


def _unit_rows(seed, name, rows, D):
    x = synth.normal(seed, name, (rows, D), 1.0)
    return x / x.norm(dim=1, keepdim=True)


def op_inputs(widths, n, C, seed, tie=False):
    """seeded inputs of one case: per model L2-normalised float32 image rows [n, D_m] and text rows [C, D_m], and float32 scales.
    tie: text row 5 repeats text row 2 in every model and every image leans towards that row, so both sit at the top of every row."""
    imgs, txts = [], []
    for m, D in enumerate(widths):
        img, txt = _unit_rows(seed, f"zs.img{m}", n, D), _unit_rows(seed, f"zs.txt{m}", C, D)
        if tie:
            txt[5] = txt[2]
            img = img + 2.0 * txt[2]
            img = img / img.norm(dim=1, keepdim=True)
        imgs.append(img)
        txts.append(txt)
    scales = [float(np.float32(SCALES[m])) for m in range(len(widths))]
    return imgs, txts, scales


def mix_f64(imgs, txts, scales):
    """(1 / M) sum_m s_m img_m txt_m^T in float64, the models added in order -> [n, C]"""
    total = 0.0
    for a, t, s in zip(imgs, txts, scales):
        # (einsum's own loop, not a BLAS product: every output is the same serial sum over D, so equal text rows give equal logits)
        total = total + float(s) * np.einsum("bd,cd->bc", np.asarray(a, dtype=np.float64), np.asarray(t, dtype=np.float64))
    return total / float(len(imgs))


def top5(logits):
    """indices of the five largest entries per row, ties to the LOWER index (top5_kernel); rows shorter than five: what there is"""
    x = np.asarray(logits)
    k = min(5, x.shape[1])
    return np.stack([np.lexsort((np.arange(x.shape[1]), -r))[:k] for r in x]).astype(np.int64)


def margins(logits, targets=None):
    """the smallest gap that decides a stored top-5 entry or a counted hit: between ranks 1 .. 6 of each row and, with targets, between
    the target's logit and ranks 5 / 6 (where the target is neither)"""
    x = np.asarray(logits, dtype=np.float64)
    worst = np.inf
    for b, r in enumerate(x):
        s = np.sort(r)[::-1][:6]
        if s.size > 1:
            worst = min(worst, float(np.min(s[:-1] - s[1:])))
        if targets is not None:
            t = r[int(targets[b])]
            worst = min([worst] + [abs(float(t - v)) for v in s[4:6] if v != t])
    return worst


def hit_counts(top5_idx, targets):
    t = np.asarray(targets).reshape(-1, 1)
    idx = np.asarray(top5_idx)
    return int((idx[:, :1] == t).sum()), int((idx == t).any(axis=1).sum())


def op_cases():
    """[(name, (widths, n, C), fixture arrays)] of zeroshot_ops.npz, and its meta"""
    z, meta = load_golden("zeroshot_ops")
    out = []
    for c in meta["cases"].split(","):
        shape = (tuple(int(w) for w in z[c + "_widths"].tolist()), int(z[c + "_n"]), int(z[c + "_C"]))
        out.append((c, shape, {k: z[f"{c}_{k}"] for k in ("seed", "keep", "logits64", "logits32")}))
    return out, meta
