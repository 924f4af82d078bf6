"""GPU: distillation tuning for retrieval (retrieval/clip_ret_kd.py) on the HIP path — the split-row KD kernels (rlcf_kd_loss_split)
against the reference's float64 numbers (tests/golden/retkd_ops.npz), rlcf_tta_retrieval_image_kd / rlcf_tta_retrieval_text_kd
against the reference's own tune_image / tune_text runs (retkd_i2t_tiny*, retkd_t2i_tiny), the mirror module rlcf_amd.clip_ret_kd,
the test_time_tune loop of both entries (retkd_loop_tiny), the recall report (rlcf_retrieval_ranks) and the refusals.  Every call goes
on torch.cuda.current_stream()."""
import copy
import ctypes as C
import os
import sys
import types

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from oracle import retrieval_ref as QR
from oracle import rlcf_ref as RR
from rlcf_amd import synth
import retrieval_kd_ref as KR
from retrieval_kd_ref import METRIC_KEYS, ops_cases, ops_rows, random_scores

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden")
BAR = 1e-5       # test_gpu_kd.py::_bar for KD rows: the row arithmetic runs in double, one rounding to float32


@pytest.fixture(scope="module")
def L():
    from rlcf_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


def load_golden(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    arrays = {k: torch.from_numpy(z[k]) for k in z.files if not k.startswith("meta_")}
    meta = {k[5:]: (z[k].item() if z[k].ndim == 0 else z[k]) for k in z.files if k.startswith("meta_")}
    return arrays, meta


# ------------------------------------------------------------------------------ op level
@pytest.mark.parametrize("case", list(range(10)))
def test_kd_loss_split_matches_float64(L, dev, case):
    from rlcf_amd.engine import kd_loss_op, kd_loss_split_op
    i, n, Cn, ts, tt, seed, g = [c for c in ops_cases() if c[0] == case][0]
    s, t = (x.to(dev) for x in ops_rows(n, Cn, seed))
    p = L.KdParams(ts, tt, 1.0, 0.5, 1.0, 2.0, 1e-5)
    loss, d, rows = kd_loss_split_op(s, t, p, row_loss=True)
    torch.cuda.synchronize()
    want, ref, nrm = float(g[f"loss_{i}"]), g[f"grad_sample_{i}"].double(), float(g[f"grad_norm_{i}"])
    gs = d.reshape(-1)[::7].double().cpu()
    e_loss = abs(float(loss) - want) / abs(want) if want else abs(float(loss))
    e_grad = float((gs - ref).norm()) / float(ref.norm()) if float(ref.norm()) > 0 else float(gs.norm())
    print(f"[kd split] n={n} C={Cn} T=({ts},{tt}): loss {float(loss):.7f} vs {want:.7f} rel {e_loss:.2e}; |d dlogits|/|dlogits| {e_grad:.2e}")
    assert e_loss <= BAR and e_grad <= BAR
    assert abs(float(d.double().norm()) - nrm) <= BAR * nrm + 1e-12
    assert abs(float(rows.double().mean()) - want) <= BAR * abs(want) + 1e-12
    # two calls: the same bits
    loss2, d2, _ = kd_loss_split_op(s, t, p)
    assert torch.equal(loss, loss2) and torch.equal(d, d2)
    # strided rows: the same bits as packed rows
    wide_s, wide_t = torch.full((n, Cn + 13), 7.0, device=dev), torch.full((n, Cn + 5), -3.0, device=dev)
    wide_s[:, :Cn], wide_t[:, :Cn] = s, t
    loss3, d3, _ = kd_loss_split_op(wide_s[:, :Cn], wide_t[:, :Cn], p)
    assert torch.equal(loss, loss3) and torch.equal(d, d3)
    # against the one-workgroup-per-row kernel: within the same bar (another reduction order, so no bit equality asked)
    loss1, d1, _ = kd_loss_op(s, t, L.KD_KD, None, p)
    torch.cuda.synchronize()
    assert abs(float(loss1) - float(loss)) <= BAR * abs(float(loss1)) + 1e-12
    assert float((d1 - d).double().norm()) <= BAR * float(d1.double().norm()) + 1e-12


def test_kd_loss_split_refuses_bad_shapes(L, dev):
    lib = L.lib()
    x = torch.zeros(1, 8, device=dev)
    out = torch.zeros(1, device=dev)
    assert lib.rlcf_kd_loss_split(x.data_ptr(), 8, x.data_ptr(), 8, 1, 0, None, out.data_ptr(), None, None, st()) == -1
    assert lib.rlcf_kd_loss_split(x.data_ptr(), 8, x.data_ptr(), 8, 1, L.KD_MAX_CLASSES + 1, None, out.data_ptr(), None, None, st()) == -1
    assert lib.rlcf_kd_loss_split(x.data_ptr(), 4, x.data_ptr(), 8, 1, 8, None, out.data_ptr(), None, None, st()) == -1


# ------------------------------------------------------------------------------ engine entries vs the reference's runs
def _i2t_engine(L, dev, meta, prec):
    from rlcf_amd.engine import Engine
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    ssd, rsd = synth.make_state_dict(sg, meta["student_seed"], device=dev), synth.make_state_dict(rg, meta["reward_seed"], device=dev)
    eng = Engine(sg, rg, max(meta["n_img"], 2), meta["n_bank"], prec)
    eng.load_state_dict(L.STUDENT, ssd)
    eng.load_state_dict(L.REWARD, rsd)
    eng.finalize()
    eng.set_class_bank(synth.make_token_bank(sg, meta["n_bank"], seed=meta["bank_seed"], n_ctx=4), 0, None, L.TEXT_SHARED)
    return eng, ssd, sg


def _cfg(meta, K=1):
    from rlcf_amd.engine import TTAConfig
    return TTAConfig(selection_p=1.0, tta_steps=meta["tta_steps"], sample_k=K, lr=meta["lr"], weight_decay=meta["weight_decay"], eps=meta["eps"])


@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("name", ["retkd_i2t_tiny", "retkd_i2t_tiny_b2"])
def test_retrieval_image_kd_matches_reference_fixture(L, dev, name, prec):
    """Bars: test_gpu_round2.py::test_retrieval_image_to_text_matches_reference_fixture for final logits, gradient norms / sample and
    deltas; first-step logits, teacher rows and dlogits at the logits' bar (1e-3 absolute; dlogits relative to their norm)."""
    from test_gpu_parity import _tensor_norms
    g, meta = load_golden(name)
    eng, ssd, sg = _i2t_engine(L, dev, meta, prec)
    images = synth.make_views(meta["view_seed"], meta["n_img"], sg.image_resolution, device=dev)
    o = eng.tta_retrieval_image_kd(images, _cfg(meta))
    torch.cuda.synchronize()
    c = lambda k: o[k].cpu()
    torch.testing.assert_close(c("logits"), g["logits"], atol=1e-3, rtol=0)
    torch.testing.assert_close(c("teacher"), g["teacher"], atol=1e-3, rtol=0)
    torch.testing.assert_close(c("loss")[0], g["loss"], atol=1e-3, rtol=0)
    assert (c("dlogits") - g["dlogits"]).norm() / g["dlogits"].norm() < 1e-3
    torch.testing.assert_close(c("final_logits"), g["final_logits"], atol=1e-3, rtol=0)
    keys = RR.visual_param_keys(ssd)
    grad, after = eng.merge_visual(o["ln_grad"], o["vis_grad"]), eng.merge_visual(o["ln_after"], o["vis_after"])
    torch.testing.assert_close(_tensor_norms(ssd, keys, grad), g["grad_l2"], rtol=3e-3, atol=1e-9)
    torch.testing.assert_close(_tensor_norms(ssd, keys, after, ssd), g["delta_l2"], rtol=0.01, atol=1e-7)
    assert (grad[::7].cpu() - g["grad_sample"]).norm() / g["grad_sample"].norm() < 2e-3
    assert int(o["step_skipped"].sum()) == 0
    # the engine is left pristine: a policy call afterwards still matches its own fixture
    pname = name.replace("retkd_", "retrieval_")
    pg, pmeta = load_golden(pname)
    po = eng.tta_retrieval_image(images, _cfg(pmeta, pmeta["sample_k"]))
    torch.cuda.synchronize()
    assert po["topk_idx"].cpu().reshape(-1).tolist() == pg["topk_idx"].reshape(-1).tolist()
    torch.testing.assert_close(po["final_logits"].cpu(), pg["final_logits"], atol=1e-3, rtol=0)
    eng.close()


def _t2i_engine(L, dev, meta, prec):
    from rlcf_amd.engine import Engine
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    ssd, rsd = synth.make_state_dict(sg, meta["student_seed"], device=dev), synth.make_state_dict(rg, meta["reward_seed"], device=dev)
    eng = Engine(sg, rg, 8, meta["n_images"], prec)
    eng.load_state_dict(L.STUDENT, ssd)
    eng.load_state_dict(L.REWARD, rsd)
    eng.finalize()
    images = synth.make_views(meta["image_seed"], meta["n_images"], sg.image_resolution, device=dev)
    sb = torch.cat([eng.encode_image(L.STUDENT, images[i: i + 8]) for i in range(0, meta["n_images"], 8)])
    rb = torch.cat([eng.encode_image(L.REWARD, images[i: i + 8]) for i in range(0, meta["n_images"], 8)])
    eng.set_image_bank(sb, rb)
    query = synth.make_token_bank(sg, meta["bank_size"], seed=meta["bank_seed"], n_ctx=4)[meta["query_row"]]
    return eng, ssd, query


@pytest.mark.parametrize("prec", [0, 2])
def test_retrieval_text_kd_matches_reference_fixture(L, dev, prec):
    """Bars: the text-tuning fixture test of tests/test_gpu_round2.py for the same quantities (logits 1e-3, reward text 1e-5, gradient
    sample 2e-3 relative, tuned elements off by > 0.1 lr under 1 %, final logits 5e-3); teacher row and dlogits at the logits' bar."""
    g, meta = load_golden("retkd_t2i_tiny")
    eng, ssd, query = _t2i_engine(L, dev, meta, prec)
    o = eng.tta_retrieval_text_kd(query, _cfg(meta))
    torch.cuda.synchronize()
    c = lambda k: o[k].cpu()
    torch.testing.assert_close(c("logits"), g["logits"], atol=1e-3, rtol=0)
    torch.testing.assert_close(c("teacher"), g["teacher"], atol=1e-3, rtol=0)
    torch.testing.assert_close(c("loss")[0], g["loss"], atol=1e-3, rtol=0)
    assert (c("dlogits") - g["dlogits"]).norm() / g["dlogits"].norm() < 1e-3
    torch.testing.assert_close(c("reward_text_features"), g["reward_text"], atol=1e-5, rtol=0)
    grad = eng.merge_text(o["ln_grad"], o["text_grad"]).cpu()
    assert (grad[::7] - g["grad_sample"]).norm() / g["grad_sample"].norm() < 2e-3
    d = (eng.merge_text(o["ln_after"], o["text_after"]).cpu()[::7] - g["after_sample"]).abs()
    assert (d > 0.1 * meta["lr"]).float().mean() < 0.01
    torch.testing.assert_close(c("final_logits"), g["final_logits"], atol=5e-3, rtol=0)
    # pristine afterwards: the policy call still matches its own fixture
    pg, pmeta = load_golden("retrieval_t2i_tiny")
    po = eng.tta_retrieval_text(query, _cfg(pmeta, pmeta["sample_k"]))
    torch.cuda.synchronize()
    assert po["topk_idx"].cpu().reshape(-1).tolist() == pg["topk_idx"].reshape(-1).tolist()
    torch.testing.assert_close(po["final_logits"].cpu(), pg["final_logits"], atol=5e-3, rtol=0)
    eng.close()


def test_retrieval_text_kd_split_path_matches_restatement(L, dev):
    """A bank above the split threshold (4096 seeded unit vectors, tiny towers): the text entry on the split-row kernels, d logit_scale
    from their partial dot products, against the CPU restatement (tests/retrieval_kd_ref.py).  Bars of the fixture test above."""
    from rlcf_amd.engine import Engine, TTAConfig
    sg, rg = synth.GEOMETRIES["tiny"], synth.GEOMETRIES["tiny-r"]
    ssd, rsd = synth.make_state_dict(sg, 11), synth.make_state_dict(rg, 23)
    n, steps, lr = 4096, 2, 1e-4
    gen = torch.Generator().manual_seed(5)
    sbank = torch.nn.functional.normalize(torch.randn(n, sg.embed_dim, generator=gen), dim=-1)
    rbank = torch.nn.functional.normalize(torch.randn(n, rg.embed_dim, generator=gen), dim=-1)
    query = synth.make_token_bank(sg, 8, seed=7, n_ctx=4)[3]
    hp = RR.TTAHyper(selection_p=1.0, tta_steps=steps, sample_k=1, lr=lr, weight_decay=5e-4, eps=1e-6)
    ref = KR.tune_text(ssd, rsd, query[None], None, hp, student_bank=sbank, reward_bank=rbank)
    eng = Engine(sg, rg, 8, n, L.PREC_F32)
    eng.load_state_dict(L.STUDENT, {k: v.to(dev) for k, v in ssd.items()})
    eng.load_state_dict(L.REWARD, {k: v.to(dev) for k, v in rsd.items()})
    eng.finalize()
    eng.set_image_bank(sbank.to(dev), rbank.to(dev))
    o = eng.tta_retrieval_text_kd(query, TTAConfig(selection_p=1.0, tta_steps=steps, sample_k=1, lr=lr, weight_decay=5e-4, eps=1e-6))
    torch.cuda.synchronize()
    c = lambda k: o[k].cpu()
    torch.testing.assert_close(c("logits"), ref["logits"], atol=1e-3, rtol=0)
    torch.testing.assert_close(c("teacher"), ref["teacher"], atol=1e-3, rtol=0)
    assert (c("dlogits") - ref["dlogits"]).norm() / ref["dlogits"].norm() < 1e-3
    grad = eng.merge_text(o["ln_grad"], o["text_grad"]).cpu()
    assert (grad - ref["grad"]).norm() / ref["grad"].norm() < 2e-3
    keys = QR.text_param_keys(ssd)
    off = sum(ssd[k].numel() for k in keys[:keys.index("logit_scale")])
    assert abs(float(grad[off]) - float(ref["grad"][off])) <= 2e-3 * abs(float(ref["grad"][off])) + 1e-6       # d logit_scale alone
    d = (eng.merge_text(o["ln_after"], o["text_after"]).cpu() - ref["after"]).abs()
    assert (d > 0.1 * lr).float().mean() < 0.01
    torch.testing.assert_close(c("final_logits"), ref["final_logits"], atol=5e-3, rtol=0)
    eng.close()


def test_retrieval_text_kd_full_size_matches_restatement(L, dev):
    """rlcf_tta_retrieval_text_kd at the size the retrieval scripts run (CLIP ViT-B/16 text tower: 12 x 512, vocabulary 49408; a
    5000-image seeded bank as the COCO 5k test split, 3 steps) against the CPU restatement (tests/retrieval_kd_ref.py, pinned to the
    reference's tune_text by retkd_t2i_tiny), as test_gpu_round2.py::test_retrieval_text_tuning_full_size_matches_oracle does for the
    policy, with its bars: logits 1e-3, gradient 2e-3 relative, tuned elements off by > 0.1 lr under 1 %, final logits 5e-3; the teacher
    row at the logits' bar, the dense dlogits at 1e-3 of their norm.  5000 = 4 whole chunks of the split kernels + a tail of 904."""
    from rlcf_amd.engine import Engine, TTAConfig
    sg = synth.GEOMETRIES["ViT-B/16"]
    ssd, rsd = ({k: v.cpu() for k, v in synth.make_state_dict(sg, sd_, device=dev).items()} for sd_ in (11, 23))
    n, steps, lr = 5000, 3, 1e-5
    gen = torch.Generator().manual_seed(5)
    sbank = torch.nn.functional.normalize(torch.randn(n, sg.embed_dim, generator=gen), dim=-1)
    rbank = torch.nn.functional.normalize(torch.randn(n, sg.embed_dim, generator=gen), dim=-1)
    query = synth.make_token_bank(sg, 8, seed=7, n_ctx=4)[3]
    hp = RR.TTAHyper(selection_p=1.0, tta_steps=steps, sample_k=1, lr=lr, weight_decay=5e-4, eps=1e-6)
    ref = KR.tune_text(ssd, rsd, query[None], None, hp, student_bank=sbank, reward_bank=rbank)
    eng = Engine(sg, sg, 8, n, L.PREC_F16X3)
    eng.load_state_dict(L.STUDENT, {k: v.to(dev) for k, v in ssd.items()})
    eng.load_state_dict(L.REWARD, {k: v.to(dev) for k, v in rsd.items()})
    eng.finalize()
    eng.set_image_bank(sbank.to(dev), rbank.to(dev))
    o = eng.tta_retrieval_text_kd(query, TTAConfig(selection_p=1.0, tta_steps=steps, sample_k=1, lr=lr, weight_decay=5e-4, eps=1e-6))
    torch.cuda.synchronize()
    c = lambda k: o[k].cpu()
    grad = eng.merge_text(o["ln_grad"], o["text_grad"]).cpu()
    d = (eng.merge_text(o["ln_after"], o["text_after"]).cpu() - ref["after"]).abs()
    print(f"[text KD, ViT-B/16, {n} images] max|dlogit| {float((c('logits') - ref['logits']).abs().max()):.3e}, teacher "
          f"{float((c('teacher') - ref['teacher']).abs().max()):.3e}, |d dlogits|/|dlogits| {float((c('dlogits') - ref['dlogits']).norm() / ref['dlogits'].norm()):.3e}, "
          f"|d grad|/|grad| {float((grad - ref['grad']).norm() / ref['grad'].norm()):.3e}, {int((d > 0.1 * lr).sum())} of {d.numel()} tuned elements "
          f"differ by > 0.1 lr, final {float((c('final_logits') - ref['final_logits']).abs().max()):.3e}, loss {float(c('loss')):.6f} vs {float(ref['loss']):.6f}")
    torch.testing.assert_close(c("logits"), ref["logits"], atol=1e-3, rtol=0)
    torch.testing.assert_close(c("teacher"), ref["teacher"], atol=1e-3, rtol=0)
    assert (c("dlogits") - ref["dlogits"]).norm() / ref["dlogits"].norm() < 1e-3
    assert (grad - ref["grad"]).norm() / ref["grad"].norm() < 2e-3
    assert (d > 0.1 * lr).float().mean() < 0.01                          # Adam's sign on ~zero gradients
    torch.testing.assert_close(c("final_logits"), ref["final_logits"], atol=5e-3, rtol=0)
    assert int(o["step_skipped"].sum()) == 0
    eng.close()


def test_retrieval_image_kd_full_bank_matches_restatement(L, dev):
    """rlcf_tta_retrieval_image_kd over a bank of 25 010 seeded captions (the COCO 5k test split's count: 24 whole chunks of the split
    kernels + a tail of 434) on the small visual tower, a loader batch of two query images, 3 steps, against the CPU restatement
    (pinned to the reference's tune_image by retkd_i2t_tiny*).  Bars of
    test_gpu_round2.py::test_retrieval_image_to_text_matches_reference_fixture: final logits 1e-3, per-tensor gradient norms 3e-3,
    deltas 1 %, gradient 2e-3 relative; first-step logits and teacher rows at 1e-3, the dense dlogits at 1e-3 of their norm."""
    from rlcf_amd.engine import Engine, TTAConfig
    from test_gpu_parity import _tensor_norms
    sg, rg = synth.GEOMETRIES["tiny"], synth.GEOMETRIES["tiny-r"]
    ssd, rsd = synth.make_state_dict(sg, 11), synth.make_state_dict(rg, 23)
    n_bank, n_img, steps, lr = 25010, 2, 3, 1e-4
    tokens = synth.make_token_bank(sg, n_bank, seed=7, n_ctx=4)
    images = synth.make_views(1000, n_img, sg.image_resolution)
    hp = RR.TTAHyper(selection_p=1.0, tta_steps=steps, sample_k=1, lr=lr, weight_decay=5e-4, eps=1e-6)
    ref = KR.tune_image(ssd, rsd, images, tokens, hp)
    eng = Engine(sg, rg, 2, n_bank, L.PREC_F16X3)
    eng.load_state_dict(L.STUDENT, {k: v.to(dev) for k, v in ssd.items()})
    eng.load_state_dict(L.REWARD, {k: v.to(dev) for k, v in rsd.items()})
    eng.finalize()
    eng.set_class_bank(tokens, 0, None, L.TEXT_SHARED)
    o = eng.tta_retrieval_image_kd(images.to(dev), TTAConfig(selection_p=1.0, tta_steps=steps, sample_k=1, lr=lr, weight_decay=5e-4, eps=1e-6))
    torch.cuda.synchronize()
    c = lambda k: o[k].cpu()
    keys = RR.visual_param_keys(ssd)
    grad, after = eng.merge_visual(o["ln_grad"], o["vis_grad"]).cpu(), eng.merge_visual(o["ln_after"], o["vis_after"]).cpu()
    print(f"[image KD, tiny tower, {n_bank} captions x {n_img} images] max|dlogit| {float((c('logits') - ref['logits']).abs().max()):.3e}, teacher "
          f"{float((c('teacher') - ref['teacher']).abs().max()):.3e}, |d dlogits|/|dlogits| {float((c('dlogits') - ref['dlogits']).norm() / ref['dlogits'].norm()):.3e}, "
          f"|d grad|/|grad| {float((grad - ref['grad']).norm() / ref['grad'].norm()):.3e}, final {float((c('final_logits') - ref['final_logits']).abs().max()):.3e}, "
          f"loss {float(c('loss')):.6f} vs {float(ref['loss']):.6f}")
    assert c("logits").shape == (n_img, n_bank) and c("dlogits").shape == (n_img, n_bank)
    torch.testing.assert_close(c("logits"), ref["logits"], atol=1e-3, rtol=0)
    torch.testing.assert_close(c("teacher"), ref["teacher"], atol=1e-3, rtol=0)
    torch.testing.assert_close(c("loss")[0], ref["loss"], atol=1e-3, rtol=0)
    assert (c("dlogits") - ref["dlogits"]).norm() / ref["dlogits"].norm() < 1e-3
    assert (grad - ref["grad"]).norm() / ref["grad"].norm() < 2e-3
    torch.testing.assert_close(_tensor_norms(ssd, keys, grad), _tensor_norms(ssd, keys, ref["grad"]), rtol=3e-3, atol=1e-9)
    torch.testing.assert_close(_tensor_norms(ssd, keys, after, ssd), _tensor_norms(ssd, keys, ref["after"], ssd), rtol=0.01, atol=1e-7)
    torch.testing.assert_close(c("final_logits"), ref["final_logits"], atol=1e-3, rtol=0)
    assert int(o["step_skipped"].sum()) == 0
    eng.close()


# ------------------------------------------------------------------------------ the mirror module and its loop
def _register(dev, meta, n_tokens):
    from rlcf_amd import clip_store, runtime
    runtime.reset_session()
    sg, rg = synth.GEOMETRIES[str(meta["student"])] if "student" in meta else synth.GEOMETRIES["tiny"], synth.GEOMETRIES["tiny-r"]
    clip_store.register_checkpoint("student", sg, synth.make_state_dict(sg, int(meta["student_seed"])))
    clip_store.register_checkpoint("reward", rg, synth.make_state_dict(rg, int(meta["reward_seed"])))
    tokens = synth.make_token_bank(sg, n_tokens, seed=int(meta["bank_seed"]), n_ctx=4)
    clip_store.set_tokenizer(lambda texts, context_length=77, truncate=False: tokens[[int(t.strip().rstrip(".").split("c")[-1]) for t in ([texts] if isinstance(texts, str) else texts)]])
    return sg, rg


def test_mirror_tune_image_reproduces_the_engine_call(L, dev):
    from rlcf_amd import clip_ret_kd as K, runtime
    g, meta = load_golden("retkd_i2t_tiny")
    sg, rg = _register(dev, meta, meta["n_bank"])
    texts = [f"c{i}." for i in range(meta["n_bank"])]
    model = K.CLIPRet_TTA(dev, arch="student", only_visual=True)
    reward_model = K.CLIPRewards(dev, arch="reward", sample_k=20, reward_process=True, process_batch=False)
    model.set_text_bank(texts)
    reward_model.set_many_text_features(texts)
    optimizer = torch.optim.AdamW(model.parameters(), lr=meta["lr"], eps=meta["eps"], weight_decay=meta["weight_decay"])
    image = synth.make_views(meta["view_seed"], 1, sg.image_resolution, device=dev)
    out = K.tune_image(image, model, reward_model, optimizer, None, args=types.SimpleNamespace(tta_steps=meta["tta_steps"]))
    torch.testing.assert_close(out["teacher"].cpu(), g["teacher"], atol=1e-3, rtol=0)
    li, lt = reward_model.calulate_similarity()                           # what the reference's tune_image distils from
    torch.testing.assert_close(li.cpu(), g["teacher"], atol=1e-3, rtol=0)
    assert lt.shape == (meta["n_bank"], 1)
    logits_per_image, _ = model(image)
    torch.testing.assert_close(logits_per_image[:1].cpu(), g["final_logits"], atol=1e-3, rtol=0)
    direct = runtime.SESSION.engine(1).tta_retrieval_image_kd(image, _cfg(meta))
    assert torch.equal(direct["vis_after"], model.vis.data) and torch.equal(direct["ln_after"], model.ln.data)
    with pytest.raises(NotImplementedError, match="reset state"):
        K.tune_image(image, model, reward_model, optimizer, None, args=types.SimpleNamespace(tta_steps=1))
    model.reset_initial()
    runtime.reset_session()


def test_mirror_tune_text_reproduces_the_engine_call(L, dev):
    from rlcf_amd import clip_ret_kd as K, runtime
    g, meta = load_golden("retkd_t2i_tiny")
    sg, rg = _register(dev, meta, meta["bank_size"])
    model = K.CLIPRet_TTA(dev, arch="student", only_visual=False)
    reward_model = K.CLIPRewards(dev, arch="reward", sample_k=12, reward_process=True, process_batch=False)
    images = synth.make_views(meta["image_seed"], meta["n_images"], sg.image_resolution, device=dev)
    model.set_image_features(images=images)
    reward_model.set_image_features(images=images)
    optimizer = torch.optim.AdamW(model.parameters(), lr=meta["lr"], eps=meta["eps"], weight_decay=meta["weight_decay"])
    optim_state = copy.deepcopy(optimizer.state_dict())
    text = f"c{meta['query_row']}."
    for rep in range(2):
        out = K.tune_text(text, model, reward_model, optimizer, None, args=types.SimpleNamespace(tta_steps=meta["tta_steps"]))
        torch.testing.assert_close(out["teacher"].cpu(), g["teacher"], atol=1e-3, rtol=0)
        torch.testing.assert_close(reward_model.text_features.cpu(), g["reward_text"], atol=1e-5, rtol=0)
        _, per_text = reward_model.calulate_similarity()
        torch.testing.assert_close(per_text.cpu(), g["teacher"], atol=1e-3, rtol=0)
        _, logits_per_text = model(images=None, text=text)
        torch.testing.assert_close(logits_per_text.cpu(), g["final_logits"], atol=5e-3, rtol=0)
        model.reset_initial()
        optimizer.load_state_dict(optim_state)
    runtime.reset_session()


class _Loader:
    def __init__(self, images, texts):
        self.dataset = types.SimpleNamespace(image=[f"i{k}.jpg" for k in range(images.shape[0])], text=texts, vis_root="/nowhere")
        self.images = images

    def __iter__(self):
        for k in range(self.images.shape[0]):
            yield {"image": self.images[k: k + 1]}

    def __len__(self):
        return self.images.shape[0]


@pytest.mark.parametrize("direction", ["image2text", "text2image"])
def test_test_time_tune_reproduces_the_reference_loop(L, dev, direction):
    """clip_ret_kd.test_time_tune on the tiny duck-typed loader of retkd_loop_tiny: the tuned rows at the final-logits bar of the
    per-query fixture tests (1e-3 image -> text, 5e-3 text -> image), the untouched matrix at -100."""
    from rlcf_amd import clip_ret_kd as K, runtime
    g, meta = load_golden("retkd_loop_tiny")
    n_img, per = int(meta["n_img"]), int(meta["per"])
    sg, rg = _register(dev, meta, n_img * per)
    texts = [f"c{i}." for i in range(n_img * per)]
    i2t = direction == "image2text"
    model = K.CLIPRet_TTA(dev, arch="student", only_visual=i2t)
    reward_model = K.CLIPRewards(dev, arch="reward", sample_k=1, reward_process=True, process_batch=False)
    loader = _Loader(synth.make_views(int(meta["view_seed"]), n_img, sg.image_resolution, device=dev), texts)
    optimizer = torch.optim.AdamW(model.parameters(), lr=float(meta["lr"]), eps=float(meta["eps"]), weight_decay=float(meta["weight_decay"]))
    a, b = K.test_time_tune(loader, dev, model, reward_model=reward_model, scaler=None, optimizer=optimizer,
                            optim_state=copy.deepcopy(optimizer.state_dict()), text_bs=128, args=types.SimpleNamespace(tta_steps=int(meta["tta_steps"])))
    assert isinstance(a, np.ndarray) and a.shape == (n_img, n_img * per) and b.shape == (n_img * per, n_img)
    if i2t:
        np.testing.assert_allclose(a, g["score_i2t"].numpy(), atol=1e-3, rtol=0)
        assert (b == -100.0).all()
    else:
        np.testing.assert_allclose(b, g["score_t2i"].numpy(), atol=5e-3, rtol=0)
        assert (a == -100.0).all()
    runtime.reset_session()


@pytest.mark.parametrize("direction", ["image2text", "text2image"])
def test_policy_test_time_tune_rows_equal_per_query_calls(L, dev, direction):
    from rlcf_amd import clip_ret_policy as P, runtime
    g, meta = load_golden("retkd_loop_tiny")
    n_img, per, K_ = int(meta["n_img"]), int(meta["per"]), 3
    sg, rg = _register(dev, meta, n_img * per)
    texts = [f"c{i}." for i in range(n_img * per)]
    i2t = direction == "image2text"
    images = synth.make_views(int(meta["view_seed"]), n_img, sg.image_resolution, device=dev)
    args = types.SimpleNamespace(tta_steps=1)

    def objects():
        model = P.CLIPRet_TTA(dev, arch="student", only_visual=i2t)
        rm = P.CLIPRewards(dev, arch="reward", sample_k=K_, reward_process=True, process_batch=False)
        opt = torch.optim.AdamW(model.parameters(), lr=1e-4, eps=1e-6, weight_decay=5e-4)
        return model, rm, opt

    model, rm, opt = objects()
    a, b = P.test_time_tune(_Loader(images, texts), dev, model, reward_model=rm, scaler=None, optimizer=opt,
                            optim_state=copy.deepcopy(opt.state_dict()), args=args)
    model, rm, opt = objects()
    if i2t:
        model.set_text_bank(texts)
        rm.set_many_text_features(texts)
        for k in range(n_img):
            P.tune_image(images[k: k + 1], model, rm, opt, None, args=args)
            row = model(images[k: k + 1])[0][0].cpu().numpy()
            assert np.array_equal(a[k], row), k
            model.reset_initial()
        assert (b == -100.0).all()
    else:
        loader = _Loader(images, texts)                                   # (the bank as the loop builds it: one loader item at a time)
        model.set_image_features(image_features=torch.cat([model.get_image_features(s["image"]) for s in loader]))
        rm.set_image_features_with_dataloder(loader)
        for k in (0, 7, n_img * per - 1):
            P.tune_text(texts[k], model, rm, opt, None, args=args)
            row = model(images=None, text=texts[k])[1][0].cpu().numpy()
            assert np.array_equal(b[k], row), k
            model.reset_initial()
        assert (a == -100.0).all()
    runtime.reset_session()


def test_report_metrics_equals_the_reference_numbers(L, dev):
    from rlcf_amd.clip_ret_policy import report_metrics
    g, meta = load_golden("retkd_loop_tiny")
    m = report_metrics(g["score_i2t"].numpy(), g["score_t2i"].numpy(), g["txt2img"].tolist(), g["img2txt"].tolist())
    assert list(m) == list(METRIC_KEYS)
    assert [m[k] for k in METRIC_KEYS] == g["metrics_loop"].tolist()
    for j, seed in enumerate(meta["rand_seeds"].tolist()):
        a, b, t2, i2 = random_scores(int(seed), int(meta["rand_n_img"]), int(meta["rand_per"]))
        m = report_metrics(a, b, t2, i2)
        assert [m[k] for k in METRIC_KEYS] == g[f"metrics_rand{j}"].tolist(), j
    with pytest.raises(ValueError, match="ground"):
        report_metrics(np.zeros((2, 3), np.float32), np.zeros((3, 2), np.float32), [0, 1, 5], [[0], [1, 2]])


# ------------------------------------------------------------------------------ refusals (argument checks: nothing is launched)
def test_retrieval_kd_entries_refuse_what_the_reference_has_no_form_of(L, dev):
    from rlcf_amd.engine import Engine
    g, meta = load_golden("retkd_i2t_tiny")
    eng, ssd, sg = _i2t_engine(L, dev, meta, 0)
    lib = L.lib()
    images = synth.make_views(meta["view_seed"], 1, sg.image_resolution, device=dev)
    tok = synth.make_token_bank(sg, 8, seed=7, n_ctx=4)[3].to(torch.int32).contiguous()
    out = L.TTAOut()
    for flag, word in ((L.F_DKD, b"DKD"), (L.F_ATKD, b"DKD"), (L.F_MIN_ENTROPY, b"min-entropy")):
        a = _cfg(meta).c_args(1)
        a.flags |= flag
        assert lib.rlcf_tta_retrieval_image_kd(eng.h, images.data_ptr(), 1, C.byref(a), None, C.byref(out), st()) == -1
        assert word in lib.rlcf_last_error()
        assert lib.rlcf_tta_retrieval_text_kd(eng.h, tok.data_ptr(), C.byref(a), None, C.byref(out), st()) == -1
        assert word in lib.rlcf_last_error()
    a = _cfg(meta).c_args(1)
    # a caption bank is no image bank (and the other way round below)
    assert lib.rlcf_tta_retrieval_text_kd(eng.h, tok.data_ptr(), C.byref(a), None, C.byref(out), st()) != 0
    assert b"image bank" in lib.rlcf_last_error()
    # the policy entries still refuse the distillation flags
    a.flags |= L.F_KD
    assert lib.rlcf_tta_retrieval_image(eng.h, images.data_ptr(), 1, C.byref(a), C.byref(out), st()) == -1
    assert lib.rlcf_tta_retrieval_text(eng.h, tok.data_ptr(), C.byref(a), C.byref(out), st()) == -1
    assert b"distillation" in lib.rlcf_last_error()
    # refusals leave the engine working
    o = eng.tta_retrieval_image_kd(images, _cfg(meta))
    torch.cuda.synchronize()
    torch.testing.assert_close(o["final_logits"].cpu(), g["final_logits"], atol=1e-3, rtol=0)
    eng.close()
    # no bank at all; an ensemble engine
    rg = synth.GEOMETRIES["tiny-r"]
    e2 = Engine(sg, [rg, rg], 2, 16, 0)
    e2.load_state_dict(L.STUDENT, ssd)
    for m_ in range(2):
        e2.load_state_dict(L.REWARD + m_, synth.make_state_dict(rg, 23 + m_, device=dev))
    e2.finalize()
    a = _cfg(meta).c_args(1)
    assert lib.rlcf_tta_retrieval_image_kd(e2.h, images.data_ptr(), 1, C.byref(a), None, C.byref(out), st()) != 0
    assert b"exactly one reward model" in lib.rlcf_last_error()
    assert lib.rlcf_tta_retrieval_text_kd(e2.h, tok.data_ptr(), C.byref(a), None, C.byref(out), st()) != 0
    assert b"exactly one reward model" in lib.rlcf_last_error()
    e2.close()
    e3 = Engine(sg, rg, 2, 16, 0)
    e3.load_state_dict(L.STUDENT, ssd)
    e3.load_state_dict(L.REWARD, synth.make_state_dict(rg, 23, device=dev))
    e3.finalize()
    assert lib.rlcf_tta_retrieval_image_kd(e3.h, images.data_ptr(), 1, C.byref(a), None, C.byref(out), st()) != 0
    assert b"bank" in lib.rlcf_last_error()
    e3.close()
