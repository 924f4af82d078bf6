"""CPU checks of the distillation losses (TPT/utils/{KD,DKD,ATKD}.py) against tests/golden/kd_ops.npz, made by the reference itself
(tests/golden/make_kd_golden.py): the analytic gradients the HIP kernel implements (rlcf_amd/csrc/kd.hip), restated here in float64,
reproduce the reference's autograd gradients; rlcf_amd.kd_losses on CPU tensors reproduces the reference's losses and gradients; the
entry points parse and refuse what the reference cannot run."""
import os
import types

import numpy as np
import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
LOSSES = ("KD", "DKD", "ATKD")
HP_DEFAULT = dict(T_stu=1.0, T_tea=1.0, alpha=1.0, beta=0.5, temperature=1.0, multiplier=2.0, eps=1e-5)


def ops():
    z = np.load(os.path.join(GOLDEN, "kd_ops.npz"))
    meta = {k[5:]: z[k].item() for k in z.files if k.startswith("meta_")}
    return z, meta


def op_entries():
    z, meta = ops()
    out = []
    for case in meta["cases"].split(","):
        for kind in LOSSES:
            if f"{case}_{kind}_loss" in z.files:
                out.append((case, kind))
    return out


def hyper(meta, case, kind):
    hp = dict(HP_DEFAULT)
    for k in hp:
        if f"{case}_{kind}_{k}" in meta:
            hp[k] = float(meta[f"{case}_{kind}_{k}"])
    return hp


def analytic(kind, s, t, hp):
    """float64 loss and d loss / d s of the three losses: the derivation of kd.hip's header comment, written out independently"""
    s, t = s.double(), t.double()
    n, C = s.shape
    if kind == "KD":
        zs, zt = s / hp["T_stu"], t / hp["T_tea"]
        ps, pt = torch.softmax(zs, 1), torch.softmax(zt, 1)
        loss = -(pt * torch.log_softmax(zs, 1)).sum(1).mean() * hp["T_stu"] ** 2
        grad = hp["T_stu"] * (ps * pt.sum(1, keepdim=True) - pt) / n
        return loss, grad
    if kind == "ATKD":
        std_s, mean_s = s.std(1, unbiased=False, keepdim=True), s.mean(1, keepdim=True)
        std_t, mean_t = t.std(1, unbiased=False, keepdim=True), t.mean(1, keepdim=True)
        ks, kt = hp["multiplier"] / (mean_s + hp["eps"]), hp["multiplier"] / (mean_t + hp["eps"])
        zs, zt = (s - std_s) * ks, (t - std_t) * kt           # (the swapped statistics of ATKD.py:21-22)
        lps, pt = torch.log_softmax(zs, 1), torch.softmax(zt, 1)
        row = (torch.xlogy(pt, pt) - pt * lps).sum(1, keepdim=True) * mean_s ** 2
        grad = mean_s ** 2 * ks * (lps.exp() * pt.sum(1, keepdim=True) - pt) / n
        return row.mean(), grad
    T, a, b = hp["temperature"], hp["alpha"], hp["beta"]
    g = t.argmax(1)
    zs, zt = s / T, t / T
    ps, pt = torch.softmax(zs, 1), torch.softmax(zt, 1)
    gm = torch.zeros_like(s, dtype=torch.bool).scatter_(1, g[:, None], True)
    ps_g, pt_g = ps[gm][:, None], pt[gm][:, None]
    ps_o, pt_o = (ps * ~gm).sum(1, keepdim=True), (pt * ~gm).sum(1, keepdim=True)
    tckd = (torch.xlogy(pt_g, pt_g) - pt_g * torch.log(ps_g) + torch.xlogy(pt_o, pt_o) - pt_o * torch.log(ps_o)).sum()
    neg = torch.full_like(zs, -float("inf"))
    qs = torch.softmax(torch.where(gm, neg, zs), 1)
    qt = torch.softmax(torch.where(gm, neg, zt), 1)
    lqs = torch.where(gm, torch.zeros_like(zs), torch.log_softmax(torch.where(gm, neg, zs), 1))
    nckd = (torch.xlogy(qt, qt) - qt * lqs).sum()
    loss = T * T * (a * tckd + b * nckd) / n
    d_t = torch.where(gm, ps * (pt_g + pt_o) - pt_g, ps * (pt_g + pt_o) - pt_o * qs)
    d_n = torch.where(gm, torch.zeros_like(zs), qs * qt.sum(1, keepdim=True) - qt)
    return loss, T * (a * d_t + b * d_n) / n


@pytest.mark.parametrize("case,kind", op_entries())
def test_analytic_gradients_match_reference_autograd(case, kind):
    z, meta = ops()
    s, t = torch.from_numpy(z[case + "_s"]), torch.from_numpy(z[case + "_t"])
    loss, grad = analytic(kind, s, t, hyper(meta, case, kind))
    l64, d64 = torch.from_numpy(z[f"{case}_{kind}_loss64"]), torch.from_numpy(z[f"{case}_{kind}_dlog64"])
    d32 = torch.from_numpy(z[f"{case}_{kind}_dlog"]).double()
    torch.testing.assert_close(loss, l64, rtol=1e-10, atol=1e-12)
    scale = max(d64.norm().item(), 1e-300)
    # float64 against float64: the same function, two summation orders.  The reference's float32 autograd: within float32 rounding,
    # amplified by ATKD's 1 / mean (min |row mean| >= 5 here)
    assert (grad - d64).norm().item() <= 1e-9 * scale + 1e-15
    assert (grad - d32).norm().item() <= 1e-4 * scale + 1e-12


@pytest.mark.parametrize("case,kind", op_entries())
def test_kd_losses_on_cpu_match_the_reference(case, kind):
    from rlcf_amd import kd_losses as K
    z, meta = ops()
    hp = hyper(meta, case, kind)
    s = torch.from_numpy(z[case + "_s"]).clone().requires_grad_(True)
    t = torch.from_numpy(z[case + "_t"])
    if kind == "KD":
        loss = K.kd_distill_loss_v2(s, t, hp["T_stu"], hp["T_tea"])
    elif kind == "DKD":
        loss = K.dkd_distill_loss(s, t, t.argmax(-1), hp["alpha"], hp["beta"], hp["temperature"])
    else:
        loss = K.atkd_distill_loss(s, t, multiplier=hp["multiplier"], eps=hp["eps"])
    loss.backward()
    torch.testing.assert_close(loss.detach(), torch.from_numpy(z[f"{case}_{kind}_loss"]), rtol=1e-6, atol=1e-7)
    torch.testing.assert_close(s.grad, torch.from_numpy(z[f"{case}_{kind}_dlog"]), rtol=1e-5, atol=1e-9)


def test_atkd_version_2_is_refused():
    from rlcf_amd import kd_losses as K
    with pytest.raises(NotImplementedError):
        K.atkd_distill_loss(torch.ones(2, 3), torch.ones(2, 3), version=2)


def test_kd_loss_flag_round_trips():
    from rlcf_amd import _lib as L
    from rlcf_amd.engine import TTAConfig
    from rlcf_amd.params import get_args
    for kind, flag in (("KD", L.F_KD), ("DKD", L.F_DKD), ("ATKD", L.F_ATKD)):
        assert get_args(["--kd_loss", kind]).kd_loss == kind
        assert TTAConfig(kd_loss=kind).flags() & L.F_KD_MASK == flag
        assert (flag & L.F_KD_MASK) >> 5 == {"KD": L.KD_KD, "DKD": L.KD_DKD, "ATKD": L.KD_ATKD}[kind]
    assert get_args([]).kd_loss == "KD"                     # the reference's default (TPT/params.py:84) ...
    assert TTAConfig().flags() & L.F_KD_MASK == 0           # ... which the RL entry points never read
    with pytest.raises(NotImplementedError):
        TTAConfig(kd_loss="MSE").flags()


def test_tune_cls_kd_refuses_what_the_reference_cannot_run():
    from rlcf_amd import tune_cls_kd
    from rlcf_amd.clip_reward import CLIPRewardsMultiple
    args = types.SimpleNamespace(kd_loss="KD", tta_steps=1, selection_p=0.1)
    ensemble = CLIPRewardsMultiple.__new__(CLIPRewardsMultiple)           # (no calulate_similarity in the reference)
    with pytest.raises(NotImplementedError, match="CLIPRewardsMultiple"):
        tune_cls_kd.test_time_tuning(types.SimpleNamespace(only_norm=False), None, None, None, args, reward_model=ensemble)
    with pytest.raises(NotImplementedError, match="prompt learner"):
        tune_cls_kd.test_time_tuning(types.SimpleNamespace(prompt_learner=None), None, None, None, args, reward_model=object())
    for name in ("images_per_pass", "in_flight"):
        a = types.SimpleNamespace(kd_loss="DKD", tta_steps=1, selection_p=0.1, **{name: 2})
        with pytest.raises(NotImplementedError, match=name):
            tune_cls_kd.test_time_adapt_eval([], types.SimpleNamespace(only_norm=False), None, None, None, a, reward_model=object())
    with pytest.raises(NotImplementedError):
        tune_cls_kd.test_time_tuning(types.SimpleNamespace(only_norm=False), None, None, None,
                                     types.SimpleNamespace(kd_loss="L2"), reward_model=object())
