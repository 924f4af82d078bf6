"""CPU: the TPT baseline's fixtures (tests/golden/tpt_*.npz, generated from the reference by tests/golden/make_tpt_golden.py) against
the plain-torch restatement in tests/tpt_ref.py: avg_entropy and its closed-form gradient on every op case, the selection, loss and
dlogits of every end-to-end fixture from its recorded logits, and the prompt step on the oracle towers."""
import types

import pytest
import torch

from oracle import rlcf_ref as RR
from rlcf_amd import synth

import tpt_ref as T

E2E = ["tpt_tiny_s1", "tpt_tiny_s3", "tpt_tiny_ln_s1", "tpt_tiny_ln_s3", "tpt_tiny_vis_s1", "tpt_tiny_rn_s1"]
OPS, OPS_META = T.op_cases()


@pytest.mark.parametrize("name,x,groups,g", OPS, ids=[c[0] for c in OPS])
def test_closed_form_matches_reference_autograd(name, x, groups, g):
    n = x.shape[0] // groups
    for dt, lk, dk, rtol in ((torch.float64, "loss64", "dlog64", 1e-12), (torch.float32, "loss", "dlog", 2e-5)):
        loss, grad = T.avg_entropy_grad(x.to(dt), groups)
        oracle = torch.stack([RR.avg_entropy(x[i * n: (i + 1) * n].to(dt)) for i in range(groups)])
        torch.testing.assert_close(oracle, g[lk].reshape(groups), rtol=rtol, atol=rtol)
        torch.testing.assert_close(loss, g[lk].reshape(groups), rtol=rtol, atol=rtol)
        torch.testing.assert_close(grad, g[dk], rtol=rtol, atol=rtol * max(float(g[dk].abs().max()), 1e-30))
    # the float64 closed form rounded once to float32 — what rlcf_tpt_loss computes — meets the bar of tests/test_gpu_tpt.py
    loss, grad = T.avg_entropy_grad(x.double(), groups)
    assert (loss.float().double() - g["loss64"].reshape(groups)).abs().max() <= T.allowance(g["loss"], g["loss64"])
    assert (grad.float().double() - g["dlog64"]).abs().max() <= T.allowance(g["dlog"], g["dlog64"])
    assert grad.float().double().sum(dim=1).abs().max() <= T.allowance(g["dlog"], g["dlog64"])
    if x.shape[1] == 1:
        assert float(loss.abs().max()) == 0.0 and float(grad.abs().max()) == 0.0


def test_op_cases_cover_the_shapes():
    names = [c[0] for c in OPS]
    for n, c in ((1, 1), (1, 37), (2, 2), (6, 37), (6, 1000), (7, 1025), (64, 200)):
        assert f"n{n}_c{c}" in names
    assert {"g3_n6_c200", "strided_n6_c200", "lead120_n6_c200"} <= set(names)
    x = dict((c[0], c[1]) for c in OPS)["lead120_n6_c200"]
    p = x.softmax(dim=1)
    assert (p == 0).sum() == 6 * 199                 # float32: every class but the leader underflows


@pytest.mark.parametrize("case", E2E)
def test_fixture_selection_loss_and_dlogits(case):
    g, meta = T.load_golden(case)
    out, idx = RR.select_confident_samples(g["logits"], meta["selection_p"])
    assert idx.tolist() == g["selected_idx"].tolist()
    loss, grad = T.avg_entropy_grad(out)
    torch.testing.assert_close(loss, g["loss"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(RR.avg_entropy(out).reshape(1), g["loss"], rtol=1e-5, atol=1e-6)
    assert ((grad - g["dlogits"]).norm() / g["dlogits"].norm()).item() < 1e-5
    assert g["top5"].tolist() == torch.topk(g["final_logits"], 5, dim=-1).indices[0].tolist()


@pytest.mark.parametrize("case", ["tpt_tiny_s1", "tpt_tiny_s3"])
def test_prompt_step_on_the_oracle_towers(case):
    g, meta = T.load_golden(case)
    geo = synth.GEOMETRIES[meta["student"]]
    sd = synth.make_state_dict(geo, meta["student_seed"])
    tokens = synth.make_token_bank(geo, meta["n_cls"], seed=meta["bank_seed"], n_ctx=meta["n_ctx"])
    ctx0 = sd["token_embedding.weight"][torch.tensor(synth.ctx_token_ids_default(geo, meta["n_ctx"]))].clone()
    views = synth.make_views(meta["view_seed"], meta["n_views"], geo.image_resolution)
    hp = RR.TTAHyper(selection_p=meta["selection_p"], tta_steps=meta["tta_steps"], lr=meta["lr"], weight_decay=meta["weight_decay"])
    o = T.tpt_prompt_sample(sd, views, tokens, ctx0, hp)
    assert o["selected_idx"].tolist() == g["selected_idx"].tolist() and o["top5"].tolist() == g["top5"].tolist()
    torch.testing.assert_close(o["logits"], g["logits"], atol=1e-4, rtol=0)
    torch.testing.assert_close(o["loss"], g["loss"], rtol=1e-5, atol=1e-6)
    assert ((o["dlogits"] - g["dlogits"]).norm() / g["dlogits"].norm()).item() < 1e-4
    assert ((o["ctx_grad"] - g["ctx_grad"]).norm() / g["ctx_grad"].norm()).item() < 1e-3
    torch.testing.assert_close(o["final_logits"], g["final_logits"], atol=1e-3, rtol=0)


def test_flag_and_mirror_refusals():
    from rlcf_amd import _lib as L
    from rlcf_amd import tpt_cls
    from rlcf_amd.engine import TTAConfig
    assert TTAConfig(tpt=True).flags() & L.F_TPT and not TTAConfig().flags() & L.F_TPT
    assert L.F_TPT == 128 and not L.F_TPT & (L.F_KD_MASK | L.F_MIN_ENTROPY | 16)
    with pytest.raises(NotImplementedError):
        tpt_cls.test_time_tuning(None, None, None, None, types.SimpleNamespace(cocoop=True, tta_steps=1))
    with pytest.raises(NotImplementedError):
        tpt_cls.test_time_adapt_eval([], None, None, None, None, None, types.SimpleNamespace(cocoop=True, tta_steps=1))
