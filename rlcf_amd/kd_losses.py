"""The distillation losses of the KD ablation (TPT/utils/KD.py, DKD.py, ATKD.py) with the reference's signatures.

On float32 device tensors each call is one launch of the rlcf_kd_loss kernel (kd.hip): the loss, and its gradient in the student
logits, which the backward of the returned tensor scales by the incoming gradient.  The teacher is a constant, as the reference
hands it over (the reward model's logits under torch.no_grad).  Tensors off the GPU, and teachers that require grad, take the torch
expression of each loss below.
"""
import torch
import torch.nn.functional as F

from . import _lib as L
from .engine import kd_loss_op


class _KdLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, student, teacher, mode, target, params):
        loss, dlogits, _ = kd_loss_op(student, teacher, mode, target, params)
        ctx.save_for_backward(dlogits)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, grad):
        (dlogits,) = ctx.saved_tensors
        return dlogits * grad, None, None, None, None


def _on_device(student, teacher):
    return (student.is_cuda and teacher.is_cuda and student.dim() == 2 and student.shape == teacher.shape
            and not teacher.requires_grad and student.shape[1] <= L.KD_MAX_CLASSES)


def _launch(student, teacher, mode, target, params):
    s = student.float()
    if s.stride(1) != 1:
        s = s.contiguous()
    t = teacher.detach().float().contiguous()
    tg = None if target is None else target.detach().reshape(-1)
    return _KdLoss.apply(s, t, mode, tg, params)


def kd_distill_loss_v2(logits_student, logits_teacher, T_stu=1.0, T_tea=1.0):
    """TPT/utils/KD.py:19-29: -mean_i sum_c softmax(t_i / T_tea)_c * log_softmax(s_i / T_stu)_c, times T_stu^2."""
    if _on_device(logits_student, logits_teacher):
        p = L.KdParams(float(T_stu), float(T_tea), 1.0, 0.5, 1.0, 2.0, 1e-5)
        return _launch(logits_student, logits_teacher, L.KD_KD, None, p)
    log_q = F.log_softmax(logits_student / T_stu, dim=1)
    p_t = F.softmax(logits_teacher / T_tea, dim=1)
    return -(p_t * log_q).sum(dim=1).mean() * T_stu * T_stu


def dkd_distill_loss(logits_student, logits_teacher, target, alpha=1.0, beta=0.5, temperature=1.0):
    """TPT/utils/DKD.py:13-37: alpha * TCKD + beta * NCKD, both summed over rows and divided by n, times temperature^2.  TCKD is the
    KL of the merged pair [p_target, p_other] (p_other summed over the other classes); NCKD the KL of the softmaxes with the target
    logit pushed down by 1000."""
    if _on_device(logits_student, logits_teacher) and target.numel() == logits_student.shape[0]:
        p = L.KdParams(1.0, 1.0, float(alpha), float(beta), float(temperature), 2.0, 1e-5)
        return _launch(logits_student, logits_teacher, L.KD_DKD, target.to(torch.int32), p)
    n = target.shape[0]
    gt = torch.zeros_like(logits_student).scatter_(1, target.reshape(-1, 1), 1).bool()
    ps = F.softmax(logits_student / temperature, dim=1)
    pt = F.softmax(logits_teacher / temperature, dim=1)
    pair_s = torch.stack([(ps * gt).sum(1), (ps * ~gt).sum(1)], dim=1)
    pair_t = torch.stack([(pt * gt).sum(1), (pt * ~gt).sum(1)], dim=1)
    tckd = F.kl_div(torch.log(pair_s), pair_t, reduction="sum") * temperature ** 2 / n
    shifted_t = F.softmax(logits_teacher / temperature - 1000.0 * gt, dim=1)
    shifted_s = F.log_softmax(logits_student / temperature - 1000.0 * gt, dim=1)
    nckd = F.kl_div(shifted_s, shifted_t, reduction="sum") * temperature ** 2 / n
    return alpha * tckd + beta * nckd


def atkd_distill_loss(logits_student, logits_teacher, temperature=4.0, multiplier=2.0, eps=1e-5, version=1):
    """TPT/utils/ATKD.py:12-42, version 1 (the one tune_cls_kd.py reaches; `temperature` is unused there).  ATKD.py:21-22 unpack
    torch.std_mean, which returns (std, mean), into names read as (mean, std): each row is normalised as
    (z - std(z)) / (mean(z) + eps) * multiplier and the per-row KL is scaled by mean(student)^2.  Reproduced as written."""
    if version != 1:
        raise NotImplementedError("atkd_distill_loss version 2 is not on the path of tune_cls_kd.py")
    if _on_device(logits_student, logits_teacher):
        p = L.KdParams(1.0, 1.0, 1.0, 0.5, 1.0, float(multiplier), float(eps))
        return _launch(logits_student, logits_teacher, L.KD_ATKD, None, p)
    with torch.no_grad():
        s_std, s_mean = torch.std_mean(logits_student, dim=-1, unbiased=False, keepdim=True)
        t_std, t_mean = torch.std_mean(logits_teacher, dim=-1, unbiased=False, keepdim=True)
    zs = (logits_student - s_std) / (s_mean + eps) * multiplier        # (the swapped statistics, see the docstring)
    zt = (logits_teacher - t_std) / (t_mean + eps) * multiplier
    kl = F.kl_div(F.log_softmax(zs, dim=-1), F.softmax(zt, dim=-1), reduction="none") * s_mean * s_mean
    return kl.sum(-1).mean()
