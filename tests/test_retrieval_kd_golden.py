"""CPU checks of the retrieval distillation surface (retrieval/clip_ret_kd.py): the test-side restatement (tests/retrieval_kd_ref.py)
against the reference's own run (tests/golden/retkd_*.npz, tests/golden/make_retrieval_kd_golden.py), the mirror module's names and
parameter lists, and kd_distill_loss_v2 on CPU tensors.  Bars of the tuning fixtures: those tests/test_oracle_golden.py applies to the
policy retrieval fixtures for the same quantities."""
import inspect
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))
from rlcf_amd import synth  # noqa: E402
from oracle import rlcf_ref as R  # noqa: E402
import retrieval_kd_ref as KR  # noqa: E402
from retrieval_kd_ref import ops_cases, ops_rows  # noqa: E402

GOLDEN = os.path.join(HERE, "golden")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    g = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("meta_")}
    meta = {k[5:]: z[k] for k in z.files if k.startswith("meta_")}
    return g, meta


def _hp(meta):
    return R.TTAHyper(selection_p=1.0, tta_steps=int(meta["tta_steps"]), sample_k=1, lr=float(meta["lr"]), weight_decay=float(meta["weight_decay"]),
                      eps=float(meta["eps"]))


@pytest.mark.parametrize("name", ["retkd_i2t_tiny", "retkd_i2t_tiny_b2"])
def test_restatement_matches_reference_image_to_text(name):
    g, meta = load(name)
    sg, rg = synth.GEOMETRIES[str(meta["student"])], synth.GEOMETRIES[str(meta["reward"])]
    ssd, rsd = synth.make_state_dict(sg, int(meta["student_seed"])), synth.make_state_dict(rg, int(meta["reward_seed"]))
    tokens = synth.make_token_bank(sg, int(meta["n_bank"]), seed=int(meta["bank_seed"]), n_ctx=4)
    images = synth.make_views(int(meta["view_seed"]), int(meta["n_img"]), sg.image_resolution)
    o = KR.tune_image(ssd, rsd, images, tokens, _hp(meta))
    torch.testing.assert_close(o["logits"], g["logits"], atol=1e-4, rtol=0)
    torch.testing.assert_close(o["teacher"], g["teacher"], atol=1e-4, rtol=0)
    torch.testing.assert_close(o["loss"], g["loss"], atol=1e-7, rtol=1e-4)
    torch.testing.assert_close(o["dlogits"], g["dlogits"], atol=1e-7, rtol=1e-4)
    assert (o["grad"][::7] - g["grad_sample"]).norm() / g["grad_sample"].norm() < 1e-4
    torch.testing.assert_close(o["final_logits"], g["final_logits"], atol=2e-4, rtol=0)


def test_restatement_matches_reference_text_to_image():
    g, meta = load("retkd_t2i_tiny")
    sg, rg = synth.GEOMETRIES[str(meta["student"])], synth.GEOMETRIES[str(meta["reward"])]
    ssd, rsd = synth.make_state_dict(sg, int(meta["student_seed"])), synth.make_state_dict(rg, int(meta["reward_seed"]))
    bank = synth.make_token_bank(sg, int(meta["bank_size"]), seed=int(meta["bank_seed"]), n_ctx=4)
    images = synth.make_views(int(meta["image_seed"]), int(meta["n_images"]), sg.image_resolution)
    o = KR.tune_text(ssd, rsd, bank[int(meta["query_row"])][None], images, _hp(meta))
    torch.testing.assert_close(o["logits"], g["logits"], atol=1e-4, rtol=0)
    torch.testing.assert_close(o["teacher"], g["teacher"], atol=1e-4, rtol=0)
    torch.testing.assert_close(o["loss"], g["loss"], atol=1e-7, rtol=1e-4)
    torch.testing.assert_close(o["dlogits"], g["dlogits"], atol=1e-7, rtol=1e-4)
    torch.testing.assert_close(o["reward_text"], g["reward_text"], atol=1e-6, rtol=0)
    assert (o["grad"][::7] - g["grad_sample"]).norm() / g["grad_sample"].norm() < 1e-4
    d = (o["after"][::7] - g["after_sample"]).abs()
    assert (d > 0.1 * float(meta["lr"])).float().mean() < 0.01          # Adam's sign on ~zero gradients
    torch.testing.assert_close(o["final_logits"], g["final_logits"], atol=2e-3, rtol=0)


def test_mirror_module_has_the_reference_names_and_parameter_lists():
    from rlcf_amd import clip_ret_kd as K, clip_ret_policy as P, kd_losses
    want = {"kd_distill_loss_v2": ["logits_student", "logits_teacher", "T_stu", "T_tea"],
            "tune_image": ["image", "model", "reward_model", "optimizer", "scaler", "args"],
            "tune_text": ["text", "model", "reward_model", "optimizer", "scaler", "args"],
            "test_time_tune": ["data_loader", "device", "model", "reward_model", "scaler", "optimizer", "optim_state", "text_bs", "args"]}
    for name, params in want.items():
        assert list(inspect.signature(getattr(K, name)).parameters) == params, name
    assert K.kd_distill_loss_v2 is kd_losses.kd_distill_loss_v2
    assert list(inspect.signature(P.test_time_tune).parameters) == want["test_time_tune"]
    assert inspect.signature(K.test_time_tune).parameters["text_bs"].default == 128
    assert list(inspect.signature(P.report_metrics).parameters) == ["scores_i2t", "scores_t2i", "txt2img", "img2txt"]
    assert callable(getattr(P.CLIPRewards, "calulate_similarity"))


def test_kd_distill_loss_v2_on_cpu_tensors_matches_the_float64_reference():
    """float32 CPU tensors against the reference's float64 numbers: float32 log-softmax over C classes, relative 1e-4 on the loss
    (|loss| ~ 10, float32 eps 6e-8 x a few hundred accumulated roundings), 2e-4 on the gradient sample's relative norm error."""
    from rlcf_amd.clip_ret_kd import kd_distill_loss_v2
    for i, n, C, ts, tt, seed, g in ops_cases():
        s, t = ops_rows(n, C, seed)
        s = s.requires_grad_(True)
        loss = kd_distill_loss_v2(s, t, T_stu=ts, T_tea=tt)
        loss.backward()
        want = g[f"loss_{i}"].double()
        assert abs(float(loss) - float(want)) <= 1e-4 * max(abs(float(want)), 1e-3), (i, float(loss), float(want))
        gs = s.grad.reshape(-1)[::7].double()
        ref = g[f"grad_sample_{i}"].double()
        assert float((gs - ref).norm()) <= 2e-4 * float(ref.norm()) + 1e-12, i
