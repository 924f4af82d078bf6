"""Plain-torch restatement of the TPT baseline for the tests (TPT/tpt_cls.py:34-78, TPT/tune_cls_tpt.py:34-54): avg_entropy with its
gradient in closed form, and the prompt step on the oracle towers.  Test infrastructure only."""
from __future__ import annotations

import os

import numpy as np
import torch

from oracle import clip_ref as C
from oracle import rlcf_ref as RR

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    arrays = {k: torch.from_numpy(np.asarray(z[k])) for k in z.files if not k.startswith("meta_")}
    meta = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    return arrays, meta


def op_cases():
    """[(name, rows [groups * n, C], groups, fixture arrays)] of tests/golden/tpt_ops.npz"""
    z, meta = load_golden("tpt_ops")
    return [(c, z[c + "_x"], int(z[c + "_groups"]), {k: z[f"{c}_{k}"] for k in ("loss", "dlog", "loss64", "dlog64")})
            for c in meta["cases"].split(",")], meta


def avg_entropy_grad(x: torch.Tensor, groups: int = 1):
    """(loss [groups], dlogits) in x's dtype: with p = softmax(x_i), a_c = log(mean_i p_ic) clamped at finfo.min,
    L = -sum_c a_c e^{a_c},  dL/dx_id = (p_id / n) * (sum_c p_ic a_c - a_d)"""
    n = x.shape[0] // groups
    losses, grads = [], []
    for g in range(groups):
        r = x[g * n: (g + 1) * n]
        lp = r - r.logsumexp(dim=-1, keepdim=True)
        a = torch.clamp(lp.logsumexp(dim=0) - torch.log(torch.tensor(float(n), dtype=x.dtype)), min=torch.finfo(torch.float32).min)
        p = lp.exp()
        losses.append(-(a * a.exp()).sum())
        grads.append(p / n * ((p * a).sum(dim=1, keepdim=True) - a))
    return torch.stack(losses), torch.cat(grads)


def allowance(ref32: torch.Tensor, ref64: torch.Tensor) -> float:
    """what a float32 result may differ from the float64 reference by: the reference's own float32 error plus one rounding"""
    return float((ref32.double() - ref64).abs().max()) + 2.0 ** -23 * float(ref64.abs().max())


def tpt_prompt_sample(student_sd, views, tokens, ctx_init, hp: RR.TTAHyper):
    """one iteration of the loop body TPT/tpt_cls.py:278-297 on the oracle towers: reset -> test_time_tuning (:49-72) -> clean view"""
    out = {}
    ctx, m, v = ctx_init.clone(), torch.zeros_like(ctx_init), torch.zeros_like(ctx_init)
    selected = None
    for j in range(hp.tta_steps):
        ctx = ctx.detach().requires_grad_(True)
        if selected is None:
            logits_all = C.student_logits(student_sd, views, tokens, ctx, False, hp.ctx_position, hp.split_idx)
            output, selected = RR.select_confident_samples(logits_all, hp.selection_p)
        else:
            output = C.student_logits(student_sd, views[selected], tokens, ctx, False, hp.ctx_position, hp.split_idx)
        loss = RR.avg_entropy(output)
        grad, dlogits = torch.autograd.grad(loss, [ctx, output])
        if j == 0:
            out.update(logits=logits_all.detach(), selected_idx=selected.clone(), loss=loss.detach().reshape(1), dlogits=dlogits.clone(),
                       ctx_grad=grad.clone())
        with torch.no_grad():
            ctx, m, v = RR.adamw_step(ctx.detach(), grad, m, v, j + 1, hp)
    with torch.no_grad():
        final = C.student_logits(student_sd, views[:1], tokens, ctx.detach(), False, hp.ctx_position, hp.split_idx)
    out.update(ctx_after=ctx.detach().clone(), final_logits=final, top5=torch.topk(final, min(5, final.shape[1]), dim=-1).indices[0])
    return out
