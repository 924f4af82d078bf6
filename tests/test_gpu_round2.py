"""GPU parity, round-2 additions: the sample-batched call at the images-per-pass counts bench.py runs against a reference-generated
STREAM of ViT-B/16 samples; GradScaler's non-finite step skip; the shipped harness with the cross-sample EMA; engine-owned scratch
(two engines on two streams); the sharded eval driver on two ranks; host-side n_sel; the reward mirror's tensor contracts."""
import copy
import json
import os
import subprocess
import sys
import threading
import types

import pytest
import torch

from oracle import rlcf_ref as RR
from rlcf_amd import synth
from test_gpu_parity import _cfg_from_meta, load_golden, make_engine

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def L():
    from rlcf_amd import _lib
    _lib.lib()
    return _lib


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda:0")


# ------------------------------------------------------------------------------ the benchmarked path, at the benchmarked batch sizes
@pytest.mark.parametrize("B", [8, 20, 32])          # 20 = the pass size of the driver's `bench.py --steps 20`
def test_tta_batch_matches_reference_stream_b16_n64(L, dev, B):
    """BASELINE configs[1] as bench.py runs it (split-f16, shared-prefix text, sparse class backward, B test images per tower
    pass): eight consecutive ViT-B/16 N=64 C=1000 samples, each produced by the reference's own harness body one at a time
    (tests/golden/make_golden.py --only b16stream: TPT/tpt_cls_rl.py:251-262).  Every sample's top-5 and final logits must come
    out of rlcf_tta_batch, at 8, 20 and 32 per pass (the stream repeated until the pass is full: all copies must agree too)."""
    g, meta = load_golden("tta_b16_n64_stream")
    n = meta["n_samples"]
    eng, *_ = make_engine((meta["student"], meta["reward"]), meta["n_views"] * B, meta["n_cls"], L.TEXT_SHARED, meta["student_seed"],
                          meta["reward_seed"], meta["bank_seed"], meta["n_ctx"], prec=L.PREC_F16X3)
    R = synth.GEOMETRIES[meta["student"]].image_resolution
    stream = torch.stack([synth.make_views(meta["view_seed0"] + i, meta["n_views"], R, device=dev) for i in range(n)])
    views = stream[torch.arange(B) % n]                   # the stream, repeated until the pass is full
    top5, fl = eng.tta_batch(views, _cfg_from_meta(meta, sparse=True), want_logits=True)
    torch.cuda.synchronize()
    top5, fl = top5.cpu(), fl.cpu()
    worst = 0.0
    for j in range(views.shape[0]):
        i = j % n
        assert top5[j].tolist() == g[f"top5_{i}"].tolist(), f"sample {i} (slot {j})"
        err = (fl[j] - g[f"final_logits_{i}"][0]).abs().max().item()
        worst = max(worst, err)
        assert err < 1e-3, f"sample {i} (slot {j}): max|dlogit| {err:.2e}"
    print(f"[stream B={B}] {views.shape[0]} samples, worst max|dlogit| = {worst:.2e}")
    eng.close()


def test_tta_sample_matches_reference_stream_intermediates(L, dev):
    """The same stream one image at a time through rlcf_tta_sample: selection, sampled classes, scores, rewards and the adapted
    prompt of every sample against the reference (split-f16)."""
    g, meta = load_golden("tta_b16_n64_stream")
    eng, *_ = make_engine((meta["student"], meta["reward"]), meta["n_views"], meta["n_cls"], L.TEXT_SHARED, meta["student_seed"],
                          meta["reward_seed"], meta["bank_seed"], meta["n_ctx"], prec=L.PREC_F16X3)
    R = synth.GEOMETRIES[meta["student"]].image_resolution
    cfg = _cfg_from_meta(meta, sparse=True)
    flipped, worst = [], 0.0
    for i in range(meta["n_samples"]):
        o = eng.tta_sample(synth.make_views(meta["view_seed0"] + i, meta["n_views"], R, device=dev), cfg)
        assert o["selected_idx"].cpu().tolist() == g[f"selected_idx_{i}"].tolist()
        assert o["topk_idx"].cpu().reshape(-1).tolist() == g[f"topk_idx_{i}"].reshape(-1).tolist()
        assert o["top5"].cpu().tolist() == g[f"top5_{i}"].tolist()
        torch.testing.assert_close(o["clip_score"].cpu(), g[f"clip_score_{i}"].reshape(-1), atol=1e-5, rtol=1e-4)
        torch.testing.assert_close(o["rewards"].cpu(), g[f"rewards_{i}"].reshape(-1), atol=5e-5, rtol=1e-3)
        torch.testing.assert_close(o["final_logits"].cpu(), g[f"final_logits_{i}"], atol=1e-3, rtol=0)
        assert int(o["step_skipped"].sum()) == 0
        # the adapted prompt: AdamW's first step moves every element by ~lr in the direction of its gradient's SIGN (SURVEY section 0 fact
        # 6), so an element whose gradient is zero to the last bits of a float32 run may land 2 lr away from the reference's: counted,
        # reported, and bounded at 1 % of the 4 x 512 elements
        d = (o["ctx_after"].cpu() - g[f"ctx_after_{i}"]).abs()
        flipped.append(int((d > 0.1 * meta["lr"]).sum()))
        worst = max(worst, (o["final_logits"].cpu() - g[f"final_logits_{i}"]).abs().max().item())
        assert flipped[-1] <= 0.01 * d.numel(), f"sample {i}: {flipped[-1]} prompt elements off by more than 0.1 lr"
    print(f"[b16 stream, one image at a time] {meta['n_samples']} samples: worst max|dlogit| = {worst:.2e}; prompt elements whose step "
          f"differs in sign from the reference's (|d ctx| > 0.1 lr, of {d.numel()}) per sample: {flipped}")
    eng.close()


# ------------------------------------------------------------------------------ GradScaler semantics: a non-finite gradient skips the step
@pytest.mark.parametrize("prec", [0, 2])
def test_nonfinite_gradient_skips_the_optimizer_step(L, dev, prec):
    """scaler.step(optimizer) (TPT/tpt_cls_rl.py:76-79) does not step when the gradient holds an inf / NaN.  A NaN pixel in an
    augmented view that gets selected makes every gradient of the sample NaN: the prompt (and the LayerNorm set on the image-encoder
    path) must stay at the reset state, the flag must be raised, and the clean-view prediction must equal plain inference — while a
    clean sample in the SAME batched pass still takes its step."""
    from rlcf_amd.engine import TTAConfig
    N, n_cls = 8, 16
    eng, ssd, rsd, tokens, ctx0 = make_engine(("tiny", "tiny-r"), N * 2, n_cls, L.TEXT_SHARED, prec=prec)
    cfg = TTAConfig(selection_p=1.0, tta_steps=2)                      # every view selected: the poisoned one is in the loss
    clean = synth.make_views(1000, N, 32).to(dev)
    bad = clean.clone()
    bad[3, 1, 5, 7] = float("nan")
    plain = eng.tta_sample(clean, TTAConfig(selection_p=1.0, tta_steps=0), want_intermediates=False)      # inference only
    ok = eng.tta_sample(clean, cfg)
    assert ok["step_skipped"].tolist() == [0, 0] and not torch.equal(ok["ctx_after"].cpu(), ctx0)
    o = eng.tta_sample(bad, cfg)
    assert o["step_skipped"].tolist() == [1, 1]
    assert torch.equal(o["ctx_after"].cpu(), ctx0)                       # untouched: not even weight decay was applied
    assert o["top5"].tolist() == plain["top5"].tolist()
    torch.testing.assert_close(o["final_logits"], plain["final_logits"], atol=1e-6, rtol=0)
    # batched pass: sample 0 poisoned, sample 1 clean
    top5, fl = eng.tta_batch(torch.stack([bad, clean]), cfg, want_logits=True)
    assert top5[0].tolist() == plain["top5"].tolist() and top5[1].tolist() == ok["top5"].tolist()
    torch.testing.assert_close(fl[1], ok["final_logits"][0], atol=1e-3, rtol=0)
    # image-encoder (LayerNorm) tuning: same contract
    ln0 = eng.ln_params(pristine=True)
    o = eng.tta_sample_ln(bad, TTAConfig(selection_p=1.0, tta_steps=1, lr=1e-3))
    assert o["step_skipped"].tolist() == [1] and torch.equal(o["ln_after"], ln0)
    o = eng.tta_sample_ln(clean, TTAConfig(selection_p=1.0, tta_steps=1, lr=1e-3))
    assert o["step_skipped"].tolist() == [0] and not torch.equal(o["ln_after"], ln0)
    eng.close()


# ------------------------------------------------------------------------------ the shipped harness with CLIPCLS_TTA + momentum_update
def _cls_tta_objects(dev, meta, only_norm):
    from rlcf_amd import clip_reward, clip_store, custom_clip, runtime
    runtime.reset_session()
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    clip_store.register_checkpoint(meta["student"], sg, synth.make_state_dict(sg, meta["student_seed"]))
    clip_store.register_checkpoint("tiny-r", rg, synth.make_state_dict(rg, meta["reward_seed"]))
    bank = clip_store.SyntheticBank(sg, meta["n_cls"], meta["n_ctx"], meta["bank_seed"])
    clip_store.set_tokenizer(bank.tokenize)
    args = types.SimpleNamespace(tta_steps=meta["tta_steps"], selection_p=meta["selection_p"], gpu=0, tpt=True, print_freq=1000,
                                 min_entropy_reg=0, min_entropy_w=0.1, reward_arch="tiny-r", multiple_reward_models=0,
                                 sample_k=meta["sample_k"], reward_amplify=False, reward_process=True, process_batch=False)
    model = custom_clip.CLIPCLS_TTA(dev, bank.classnames, arch=meta["student"], prompt_prefix="a_photo_of_a", only_visual=True,
                                    only_norm=only_norm, momentum_update=True, update_freq=meta["update_freq"],
                                    update_w=meta["update_w"], momentum=meta["momentum"])
    reward_model = clip_reward.get_reward_model(dev, args)
    reward_model.set_class_features(tokenized_classes=model.tokenized_prompts)
    optimizer = torch.optim.AdamW(model.parameters(), meta["lr"], weight_decay=meta["weight_decay"])
    return model, optimizer, copy.deepcopy(optimizer.state_dict()), reward_model, args, bank


@pytest.mark.parametrize("fixture,only_norm", [("ln_tiny_momentum", True), ("vis_tiny_momentum", False), ("bn_tiny_momentum", True)])
def test_shipped_harness_applies_the_momentum_update(L, dev, fixture, only_norm):
    """rlcf_amd.tpt_cls_rl.test_time_adapt_eval with a CLIPCLS_TTA(momentum_update=True) model is TPT/tune_cls_rl.py:183-256: after every
    sample's clean-view inference it must call model.momentum_update_model() (:240).  Three consecutive samples THROUGH THE HARNESS:
    the moving reset state must follow the reference's run (update_freq=2: the second sample moves it), which it cannot if the EMA
    is dropped; then reset_classnames_and_state (custom_clip.py:449-454) must put reset state and EMA back to the checkpoint."""
    from rlcf_amd import runtime, tpt_cls_rl
    g, meta = load_golden(fixture)
    model, optimizer, optim_state, reward_model, args, bank = _cls_tta_objects(dev, meta, only_norm)
    R = synth.GEOMETRIES[meta["student"]].image_resolution
    n = meta["n_samples"]
    # targets = the reference's own clean-view top-1 of every sample: the harness must score 100 %
    loader = [([v.unsqueeze(0) for v in synth.make_views(1000 + i, meta["n_views"], R)],
               torch.tensor([int(g[f"final_logits_{i}"][0].argmax())])) for i in range(n)]
    calls = {"train": 0, "eval": 0}
    orig_train = model.train


    def counted_train(mode=True):                # (nn.Module.eval() is train(False): count the two directions separately)
        calls["train" if mode else "eval"] += 1
        return orig_train(mode)

    model.train = counted_train
    acc = tpt_cls_rl.test_time_adapt_eval(loader, model, optimizer, optim_state, None, args, reward_model=reward_model)
    assert acc == [100.0, 100.0]
    assert calls["train"] == n and calls["eval"] >= n                   # model.train() / model.eval() round every tuning step (:216-218)
    eng = runtime.SESSION.engine()
    last = n - 1
    if only_norm:
        reset_state = eng.ln_params(pristine=True).cpu()
        torch.testing.assert_close(reset_state, g[f"ln_reset_{last}"], atol=2.5 * meta["lr"] * (1 - meta["momentum"]) * meta["update_w"], rtol=1e-6)
        assert (reset_state - g["ln_reset_0"]).abs().max() > 0           # it moved: the EMA was applied at sample 2
    else:
        from test_gpu_parity import _tensor_norms
        ssd = synth.make_state_dict(synth.GEOMETRIES[meta["student"]], meta["student_seed"])
        keys = RR.visual_param_keys(ssd)
        reset_state = eng.merge_visual(eng.ln_params(pristine=True), eng.visual_params(1))
        torch.testing.assert_close(_tensor_norms(ssd, keys, reset_state, ssd), g[f"vis_reset_delta_l2_{last}"], rtol=0.01, atol=1e-7)
        assert float(g[f"vis_reset_delta_l2_{last}"].sum()) > 0
    # next dataset: class bank swapped, visual state back to the checkpoint (after sample 0 the reference's reset state still IS the checkpoint)
    model.reset_classnames_and_state(bank.classnames, meta["student"])
    eng = runtime.SESSION.engine()
    a, b = eng.ln_params(pristine=True), eng.ln_params(pristine=False)
    assert torch.equal(a, b) and torch.equal(model.ln.data, a)
    if only_norm:
        assert torch.equal(a.cpu(), g["ln_reset_0"])
    else:
        assert torch.equal(eng.visual_params(1), eng.visual_params(2)) and torch.equal(eng.visual_params(3), eng.visual_params(2))
        assert torch.equal(eng.visual_params(0), eng.visual_params(2)) and torch.equal(model.vis.data, eng.visual_params(2))
    runtime.reset_session()


# ------------------------------------------------------------------------------ engine-owned scratch
def test_two_engines_on_two_streams_do_not_share_scratch(L, dev):
    """Every scratch buffer of an engine call belongs to the engine (split-K workspace of the small-grid GEMM, reward / loss
    statistics, step-skip flags): two engines driven concurrently from two host threads on two streams give the results of the
    serial runs.  LayerNorm tuning of one image at a time exercises the split-K workspace (K >= 1536 products on < 128 tiles)."""
    from rlcf_amd.engine import TTAConfig
    cfgs = [TTAConfig(selection_p=0.5, tta_steps=2), TTAConfig(selection_p=0.25, tta_steps=1, lr=1e-3)]
    engines = [make_engine(("small", "small"), 16, 40, L.TEXT_SHARED, student_seed=11 + i, reward_seed=23 + i, prec=L.PREC_F16X3)[0] for i in range(2)]
    views = [synth.make_views(3000 + i, 16, 64).to(dev) for i in range(2)]

    def work(i, out, reps):
        with torch.cuda.stream(torch.cuda.Stream(device=dev)):
            res = []
            for r in range(reps):
                a = engines[i].tta_sample(views[i], cfgs[0], want_intermediates=False)
                b = engines[i].tta_sample_ln(views[i], cfgs[1])
                res.append((a["final_logits"].clone(), a["ctx_after"].clone(), b["final_logits"].clone(), b["ln_after"].clone()))
            torch.cuda.current_stream().synchronize()
            out[i] = res

    serial = {}
    for i in range(2):
        work(i, serial, 1)
    conc = {}
    th = [threading.Thread(target=work, args=(i, conc, 6)) for i in range(2)]
    [t.start() for t in th]
    [t.join() for t in th]
    for i in range(2):
        for rep in conc[i]:
            for x, y in zip(rep, serial[i][0]):
                torch.testing.assert_close(x, y, atol=2e-4, rtol=0)      # (float atomics on shared-prefix dK/dV: last bits)
    for e in engines:
        e.close()


# ------------------------------------------------------------------------------ host-side n_sel
def test_n_sel_is_the_hosts_double_product(L, dev):
    """int(N * selection_p) (tpt_cls_rl.py:34) in Python doubles; the float field of the C argument block rounds 10 * 0.7f down to 6.
    The engine must select what the host (and the reference) computes: 7 — and stay inside the caller's buffers."""
    from rlcf_amd.engine import TTAConfig
    N, p = 10, 0.7
    assert int(N * p) == 7
    eng, ssd, rsd, tokens, ctx0 = make_engine(("tiny", "tiny-r"), N, 16, L.TEXT_SHARED)
    views = synth.make_views(4250, N, 32)
    ref = RR.tta_sample(ssd, rsd, views, tokens, ctx0, RR.TTAHyper(selection_p=p))
    o = eng.tta_sample(views.to(dev), TTAConfig(selection_p=p))
    assert len(ref["selected_idx"]) == 7 and o["selected_idx"].cpu().tolist() == ref["selected_idx"].tolist()
    assert o["topk_idx"].cpu().tolist() == ref["topk_idx"].tolist()
    torch.testing.assert_close(o["final_logits"].cpu(), ref["final_logits"], atol=1e-3, rtol=0)
    eng.close()


# ------------------------------------------------------------------------------ reward mirror: tensor contracts of the reference
def test_reward_mirror_tensor_contracts(L, dev):
    """CLIPScore(pairwise=True) is [n*K, n*K] (text rows against the K-times repeated image rows, clip_reward.py:118-123);
    calulate_similarity returns the (logits_per_image, logits_per_text) pair scaled by exp(logit_scale) (:167-177)."""
    from rlcf_amd import runtime
    from test_gpu_parity import _harness_objects
    g, meta = load_golden("tta_tiny_s1")
    model, optimizer, optim_state, reward_model, args = _harness_objects(dev, meta)
    views = synth.make_views(meta["view_seed"], meta["n_views"], 32).to(dev)
    n, K = 4, reward_model.sample_k
    reward_model.set_image_features(views[:n])
    idx = torch.arange(n * K, device=dev) % meta["n_cls"]
    img, cls = reward_model.image_features, reward_model.class_features
    pw = reward_model.CLIPScore(class_index=idx, pairwise=True)
    ref_pw = (reward_model.clipscore_weight * cls[idx] @ img.repeat_interleave(K, dim=0).t()).clamp_min(0)
    assert pw.shape == (n * K, n * K)
    torch.testing.assert_close(pw, ref_pw, atol=1e-5, rtol=1e-5)
    rw = reward_model.CLIPScore(class_index=idx, pairwise=False)
    torch.testing.assert_close(rw, torch.diagonal(ref_pw), atol=1e-5, rtol=1e-5)
    per_image, per_text = reward_model.calulate_similarity()
    scale = float(synth.make_state_dict(synth.GEOMETRIES[meta["reward"]], meta["reward_seed"])["logit_scale"].exp())
    torch.testing.assert_close(per_image, scale * img @ cls.t(), atol=1e-3, rtol=1e-5)
    assert per_text.shape == (meta["n_cls"], n) and torch.equal(per_text, per_image.t())
    runtime.reset_session()


# ------------------------------------------------------------------------------ the sharded driver: two ranks == one rank
def test_sharded_eval_two_ranks_equal_one_rank(L, dev, tmp_path):
    """python -m rlcf_amd.eval: BASELINE configs[3] in miniature — a 7-image stream on one rank, then on two ranks (gloo, both on
    this one GPU, launched the way the driver launches bench.py).  No data-path collective: the gathered predictions of the two
    shards must be the one-rank predictions, and the reduced hit counts must agree."""
    common = ["--total-images", "7", "--arch", "tiny", "--reward-arch", "tiny-r", "--views", "8", "--classes", "16", "--selection-p", "0.5",
              "--images-per-pass", "2"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    one, two = os.path.join(tmp_path, "one.json"), os.path.join(tmp_path, "two.json")
    r = subprocess.run([sys.executable, "-m", "rlcf_amd.eval", "--gpus", "1", "--out", one] + common, cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29517", "-m", "rlcf_amd.eval", "--gpus", "2", "--dist-backend", "gloo", "--out", two] + common,
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    a, b = json.load(open(one)), json.load(open(two))
    assert a["images"] == b["images"] == 7 and b["n_gpus"] == 2
    assert a["top5"] == b["top5"] and a["predictions_sha256"] == b["predictions_sha256"]
    assert (a["acc1"], a["acc5"]) == (b["acc1"], b["acc5"])


def test_bench_strong_scaling_line_two_ranks(L, dev):
    """bench.py --total-images T on two ranks (gloo on one GPU): one JSON line, scaling 'strong', T images in total."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", "29519", "bench.py", "--gpus", "2", "--dist-backend", "gloo", "--total-images", "6", "--warmup", "2",
                        "--views", "16", "--classes", "64", "--batch", "2", "--no-cpu-baseline", "--full"], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    rec = json.loads(line)
    assert rec["scaling"] == "strong" and rec["n_gpus"] == 2 and rec["steps"] == 6 and rec["value"] > 0
    assert rec["config"]["timed_images_per_rank"] == 3 and rec["roofline"]["check_gemm_time_within_step"] in (True, False)


# ------------------------------------------------------------------------------ RLCF_PREC_F16: the reference's own GPU arithmetic (performance mode)
def test_f16_single_pass_mode_small(L, dev):
    """RLCF_PREC_F16 switches the forward tower pipeline to plain f16 operands, one MFMA per product (fp16 autocast of the reference,
    tpt_cls_rl.py:52).  Not parity-grade: image features deviate at the f16 level (and must deviate: the mode has to be active), the
    predictions of the fused step agree with the split-f16 engine."""
    from rlcf_amd.engine import TTAConfig
    N, n_cls = 64, 40                                                   # 64 views x 17 tokens = 1088 rows: the pipelined path
    ex, *_ = make_engine(("small", "small"), N, n_cls, L.TEXT_SHARED, prec=L.PREC_F16X3)
    eh, *_ = make_engine(("small", "small"), N, n_cls, L.TEXT_SHARED, prec=L.PREC_F16)
    views = synth.make_views(2000, N, 64).to(dev)
    fx, fh = ex.encode_image(L.STUDENT, views), eh.encode_image(L.STUDENT, views)
    d = (fx - fh).abs().max().item()
    assert 1e-6 < d < 5e-3, d
    cfg = TTAConfig(selection_p=0.25)
    ox, oh = ex.tta_sample(views, cfg), eh.tta_sample(views, cfg)
    dl = (ox["final_logits"] - oh["final_logits"]).abs().max().item()
    print(f"[f16 small] max|dfeat| = {d:.2e}, max|dlogit| = {dl:.2e}")
    assert dl < 0.25 and ox["top5"][0].item() == oh["top5"][0].item()
    ex.close(); eh.close()


def test_f16_folded_layernorms_follow_later_writes_of_the_parameters(L, dev):
    """The f16 mode folds the image tower's LayerNorm gamma / beta into its in_proj / c_fc weights at finalize.  Parameters written AFTER
    that (rlcf_engine_set_ln_params: a loaded CLIPCLS_TTA state, an applied EMA) must still be honoured: the engine falls back to the
    unfolded pipeline, which reads the live parameters."""
    N, n_cls = 64, 40
    ex, *_ = make_engine(("small", "small"), N, n_cls, L.TEXT_SHARED, prec=L.PREC_F16X3)
    eh, *_ = make_engine(("small", "small"), N, n_cls, L.TEXT_SHARED, prec=L.PREC_F16)
    views = synth.make_views(2001, N, 64).to(dev)
    f0 = eh.encode_image(L.STUDENT, views).clone()
    p = ex.ln_params()
    p2 = p * (1.0 + 0.2 * torch.sin(torch.arange(p.numel(), device=dev, dtype=torch.float32))) + 0.05
    ex.set_ln_params(p2); eh.set_ln_params(p2)
    fx, fh = ex.encode_image(L.STUDENT, views), eh.encode_image(L.STUDENT, views)
    assert (fh - f0).abs().max().item() > 1e-2                      # the new parameters matter ...
    d = (fx - fh).abs().max().item()
    assert d < 5e-3, d                                              # ... and the f16 engine used them
    ex.close(); eh.close()


def _stream_choices(sel, tk):
    """the discrete choices of one sample's step as order-free sets: which views were selected, which classes were sampled per view"""
    sel = [int(v) for v in sel]
    tk = [sorted(int(c) for c in row) for row in tk]
    return sorted(sel), {v: t for v, t in zip(sel, tk)}


@pytest.mark.parametrize("fold", [0, 1])
def test_f16_single_pass_mode_b16_stream(L, dev, fold):
    """RLCF_PREC_F16 on BASELINE configs[1] against the REFERENCE stream (32 samples), in both forms of the mode — fold = 0: f32 residual
    stream (the DEFAULT), fold = 1: f16 residual stream with the LayerNorms folded into the products (opt-in, rlcf_engine_set_f16_lnfold) —
    and against TWO runs of the reference: its float32 run (`tta_b16_n64_stream`, what parity is defined on) and its OWN fp16-autocast run
    (`tta_b16_n64_stream_fp16ref`: the reference's code under torch.autocast(float16) + GradScaler, TPT/tpt_cls_rl.py:52,127,261 — the
    arithmetic this mode is a performance mode OF; generated by tests/golden/make_golden.py --only b16stream_fp16).
    Every sample that leaves the logit bound is NAMED by the discrete choice of the step that f16 rounding flipped (which views were
    selected — the lowest-entropy 6 of 64 — or which classes were sampled — top-3 of 1000 per selected view): such a sample carries
    another, equally valid policy-gradient sample's logits, O(1) away.  Asserted: a sample outside the bound ALWAYS has a flipped
    choice; fold = 0 keeps the float32 reference's top-1 on EVERY sample and flips at most one sample in eight; fold = 1 (opt-in) at
    most one in four with top-1 on >= 7 of 8."""
    g, meta = load_golden("tta_b16_n64_stream")
    n = meta["n_samples"]
    p16 = os.path.join(GOLDEN, "tta_b16_n64_stream_fp16ref.npz")
    g16, n16 = None, 0
    if os.path.exists(p16):
        try:
            g16, m16 = load_golden("tta_b16_n64_stream_fp16ref")
            n16 = int(m16["n_samples"])
        except Exception as exc:                                  # (a fixture that is being regenerated: report, compare with the float32 run only)
            print(f"[f16 b16 stream] {p16} unreadable ({type(exc).__name__}): the fp16-autocast columns are skipped")
            g16, n16 = None, 0
    eng, *_ = make_engine((meta["student"], meta["reward"]), meta["n_views"] * n, meta["n_cls"], L.TEXT_SHARED, meta["student_seed"],
                          meta["reward_seed"], meta["bank_seed"], meta["n_ctx"], prec=L.PREC_F16)
    eng.set_f16_lnfold(bool(fold))
    R = synth.GEOMETRIES[meta["student"]].image_resolution
    views = torch.stack([synth.make_views(meta["view_seed0"] + i, meta["n_views"], R, device=dev) for i in range(n)])
    cfg = _cfg_from_meta(meta, sparse=True)
    top5, fl = eng.tta_batch(views, cfg, want_logits=True)
    top5, fl = top5.cpu(), fl.cpu()
    mine = []
    for i in range(n):                                     # the discrete choices of every sample, one image at a time
        o = eng.tta_sample(views[i], cfg)
        sel = o["selected_idx"].cpu().tolist()
        mine.append(_stream_choices(sel, o["topk_idx"].cpu().reshape(len(sel), -1).tolist()))

    def against(ref, n_ref, tag):
        err = [(fl[i] - ref[f"final_logits_{i}"].float().reshape(1, -1)[0]).abs().max().item() for i in range(n_ref)]
        agree = sum(int(top5[i, 0]) == int(ref[f"top5_{i}"][0]) for i in range(n_ref))
        flips = {}
        for i in range(n_ref):
            rs = ref[f"selected_idx_{i}"].tolist()
            r_sel, r_by = _stream_choices(rs, ref[f"topk_idx_{i}"].reshape(len(rs), -1).tolist())
            if mine[i][0] != r_sel:
                flips[i] = f"view selection {sorted(set(r_sel) - set(mine[i][0]))} -> {sorted(set(mine[i][0]) - set(r_sel))}"
            elif mine[i][1] != r_by:
                v = next(v for v in mine[i][0] if mine[i][1][v] != r_by[v])
                flips[i] = f"sampled classes of view {v}: {r_by[v]} -> {mine[i][1][v]}"
        inside = [e for i, e in enumerate(err) if i not in flips]
        print(f"[f16 b16 stream, fold={fold}] vs the reference's {tag} run ({n_ref} samples): top-1 agreement {agree}/{n_ref}; samples without a "
              f"flipped discrete choice {n_ref - len(flips)}/{n_ref}, their max|dlogit| = {max(inside or [0.0]):.3e}; over all samples {max(err):.3e}")
        for i, what in sorted(flips.items()):
            print(f"   sample {i}: {what}; max|dlogit| {err[i]:.3e}, top-1 {int(top5[i, 0])} ({tag} reference {int(ref[f'top5_{i}'][0])})")
        return err, agree, flips
    err, agree, flips = against(g, n, "float32")
    if g16 is not None:
        against(g16, min(n, n16), "fp16-autocast")
        # the reference against ITSELF: how far its own fp16-autocast run is from its float32 run (context for the numbers above)
        m = min(n, n16)
        d = [(g16[f"final_logits_{i}"].float().reshape(-1) - g[f"final_logits_{i}"].float().reshape(-1)).abs().max().item() for i in range(m)]
        same = [i for i in range(m) if _stream_choices(g16[f"selected_idx_{i}"].tolist(), g16[f"topk_idx_{i}"].reshape(len(g16[f"selected_idx_{i}"]), -1).tolist())
                == _stream_choices(g[f"selected_idx_{i}"].tolist(), g[f"topk_idx_{i}"].reshape(len(g[f"selected_idx_{i}"]), -1).tolist())]
        t1 = sum(int(g16[f"top5_{i}"][0]) == int(g[f"top5_{i}"][0]) for i in range(m))
        print(f"[reference fp16-autocast vs reference float32] {m} samples: top-1 agreement {t1}/{m}; same discrete choices {len(same)}/{m}, "
              f"their max|dlogit| = {max([d[i] for i in same] or [0.0]):.3e}; over all samples {max(d):.3e}")
    # measured (profiles/r6_notes.md): fold = 0: 2 of 32 samples flip a choice, top-1 32 / 32, samples without a flip within 0.045 of the
    # reference's float32 logits; fold = 1: 4-5 flips, top-1 31 / 32, within 0.18.
    for i in range(n):
        if i not in flips:
            assert err[i] < 0.3, f"sample {i}: max|dlogit| {err[i]:.3e} without a flipped discrete choice"
            assert int(top5[i, 0]) == int(g[f"top5_{i}"][0]), f"sample {i}: top-1 differs without a flipped discrete choice"
    if fold == 0:
        assert agree == n, f"default form of RLCF_PREC_F16: top-1 {agree}/{n} against the float32 reference"
        assert len(flips) <= max(1, n // 8), flips
    else:
        assert len(flips) <= max(1, n // 4), flips
        assert agree >= n - max(1, n // 8)
    eng.close()


# ------------------------------------------------------------------------------ retrieval policy
@pytest.mark.parametrize("prec", [0, 2])
@pytest.mark.parametrize("name", ["retrieval_i2t_tiny", "retrieval_i2t_tiny_b2"])
def test_retrieval_image_to_text_matches_reference_fixture(L, dev, name, prec):
    """rlcf_tta_retrieval_image vs the reference's tune_image (retrieval/clip_ret_policy.py:76-103) + the evaluation of its loop
    (:171-176) with CLIPRet_TTA / CLIPRewards, over a 300-caption bank without learnable rows (n_ctx = 0), K = 20 (the script's
    sample_k_i2t) / a loader batch of two query images."""
    from rlcf_amd.engine import Engine, TTAConfig
    from test_gpu_parity import _tensor_norms
    g, meta = load_golden(name)
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    ssd, rsd = synth.make_state_dict(sg, meta["student_seed"], device=dev), synth.make_state_dict(rg, meta["reward_seed"], device=dev)
    eng = Engine(sg, rg, max(meta["n_img"], 2), meta["n_bank"], prec)
    eng.load_state_dict(L.STUDENT, ssd)
    eng.load_state_dict(L.REWARD, rsd)
    eng.finalize()
    tokens = synth.make_token_bank(sg, meta["n_bank"], seed=meta["bank_seed"], n_ctx=4)
    eng.set_class_bank(tokens, 0, None, L.TEXT_SHARED)                   # captions: no learnable rows
    images = synth.make_views(meta["view_seed"], meta["n_img"], sg.image_resolution, device=dev)
    cfg = TTAConfig(selection_p=1.0, tta_steps=meta["tta_steps"], sample_k=meta["sample_k"], lr=meta["lr"], weight_decay=meta["weight_decay"],
                    eps=meta["eps"])
    o = eng.tta_retrieval_image(images, cfg)
    torch.cuda.synchronize()
    c = lambda k: o[k].cpu()
    assert c("selected_idx").tolist() == list(range(meta["n_img"]))      # every query image carries reward
    assert c("topk_idx").reshape(-1).tolist() == g["topk_idx"].reshape(-1).tolist()
    torch.testing.assert_close(c("clip_score"), g["clip_score"].reshape(-1), atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(c("rewards"), g["rewards"].reshape(-1), atol=5e-5, rtol=1e-3)
    torch.testing.assert_close(c("final_logits"), g["final_logits"], atol=1e-3, rtol=0)
    keys = RR.visual_param_keys(ssd)
    grad, after = eng.merge_visual(o["ln_grad"], o["vis_grad"]), eng.merge_visual(o["ln_after"], o["vis_after"])
    torch.testing.assert_close(_tensor_norms(ssd, keys, grad), g["grad_l2"], rtol=3e-3, atol=1e-9)
    torch.testing.assert_close(_tensor_norms(ssd, keys, after, ssd), g["delta_l2"], rtol=0.01, atol=1e-7)
    gs = grad[::7].cpu()
    assert (gs - g["grad_sample"]).norm() / g["grad_sample"].norm() < 2e-3
    # prompt tuning refuses a bank without learnable rows
    with pytest.raises(L.RlcfError, match="learnable context"):
        eng.tta_sample(images, cfg)
    eng.close()


def test_retrieval_mirror_tune_image(L, dev):
    """The reference-shaped objects (rlcf_amd.clip_ret_policy: CLIPRet_TTA, CLIPRewards, tune_image) reproduce the fixture through the
    loop body of test_time_tune (clip_ret_policy.py:166-181): tune, logits of the tuned model, reset."""
    import copy
    from rlcf_amd import clip_ret_policy as P, clip_store, runtime
    g, meta = load_golden("retrieval_i2t_tiny")
    runtime.reset_session()
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    clip_store.register_checkpoint("student", sg, synth.make_state_dict(sg, meta["student_seed"]))
    clip_store.register_checkpoint("reward", rg, synth.make_state_dict(rg, meta["reward_seed"]))
    tokens = synth.make_token_bank(sg, meta["n_bank"], seed=meta["bank_seed"], n_ctx=4)
    clip_store.set_tokenizer(lambda texts, context_length=77, truncate=False: tokens[[int(t.strip().rstrip(".").split("c")[-1]) for t in ([texts] if isinstance(texts, str) else texts)]])
    texts = [f"c{i}." for i in range(meta["n_bank"])]
    model = P.CLIPRet_TTA(dev, arch="student", only_visual=True)
    reward_model = P.CLIPRewards(dev, arch="reward", sample_k=meta["sample_k"], reward_process=True, process_batch=False)
    model.set_text_bank(texts)
    reward_model.set_many_text_features(texts)
    optimizer = torch.optim.AdamW(model.parameters(), lr=meta["lr"], eps=meta["eps"], weight_decay=meta["weight_decay"])
    optim_state = copy.deepcopy(optimizer.state_dict())
    image = synth.make_views(meta["view_seed"], 1, sg.image_resolution, device=dev)
    reward_model.set_image_features(image)
    P.tune_image(image, model, reward_model, optimizer, None, args=types.SimpleNamespace(tta_steps=meta["tta_steps"]))
    logits_per_image, logits_per_text = model(image)
    torch.testing.assert_close(logits_per_image[:1].cpu(), g["final_logits"], atol=1e-3, rtol=0)
    assert logits_per_text.shape == (meta["n_bank"], 1)
    sc = reward_model.CLIPScore(text_index=g["topk_idx"].reshape(-1).to(dev), pairwise=False)
    # (scores of the PRISTINE-step sample set: the reward model is frozen, so they are the fixture's)
    torch.testing.assert_close(sc.cpu(), g["clip_score"].reshape(-1), atol=1e-5, rtol=1e-4)
    model.reset_initial()
    optimizer.load_state_dict(optim_state)
    assert torch.equal(model.ln.data, model._ln_init)
    runtime.reset_session()


def test_retrieval_text_tuning_full_size_matches_oracle(L, dev):
    """rlcf_tta_retrieval_text at the size the retrieval scripts run (CLIP ViT-B/16 text tower: 12 x 512, vocabulary 49408; a 5000-image
    bank as the COCO 5k test split, K = 12, 2 steps) against the CPU oracle (oracle.retrieval_ref.tune_text, itself pinned to the
    reference's tune_text by retrieval_t2i_tiny).  The bank features are seeded unit vectors (no image tower needed on the CPU)."""
    from rlcf_amd.engine import Engine, TTAConfig
    from oracle import retrieval_ref as QR, rlcf_ref as RR2
    sg = synth.GEOMETRIES["ViT-B/16"]
    ssd, rsd = ({k: v.cpu() for k, v in synth.make_state_dict(sg, sd_, device=dev).items()} for sd_ in (11, 23))     # (device generator: same bits, seconds)
    n, K, steps, lr = 5000, 12, 2, 1e-5
    gen = torch.Generator().manual_seed(5)
    sbank = torch.nn.functional.normalize(torch.randn(n, sg.embed_dim, generator=gen), dim=-1)
    rbank = torch.nn.functional.normalize(torch.randn(n, sg.embed_dim, generator=gen), dim=-1)
    query = synth.make_token_bank(sg, 8, seed=7, n_ctx=4)[3]
    hp = RR2.TTAHyper(selection_p=1.0, tta_steps=steps, sample_k=K, lr=lr, weight_decay=5e-4, eps=1e-6)
    ref = QR.tune_text(ssd, rsd, query[None], None, hp, student_bank=sbank, reward_bank=rbank)
    eng = Engine(sg, sg, 8, n, L.PREC_F16X3)
    eng.load_state_dict(L.STUDENT, {k: v.to(dev) for k, v in ssd.items()})
    eng.load_state_dict(L.REWARD, {k: v.to(dev) for k, v in rsd.items()})
    eng.finalize()
    eng.set_image_bank(sbank.to(dev), rbank.to(dev))
    o = eng.tta_retrieval_text(query, TTAConfig(selection_p=1.0, tta_steps=steps, sample_k=K, lr=lr, weight_decay=5e-4, eps=1e-6))
    torch.cuda.synchronize()
    c = lambda k: o[k].cpu()
    assert c("topk_idx").reshape(-1).tolist() == ref["topk_idx"].reshape(-1).tolist()
    torch.testing.assert_close(c("logits"), ref["logits"], atol=1e-3, rtol=0)
    torch.testing.assert_close(c("clip_score"), ref["clip_score"].reshape(-1), atol=1e-5, rtol=1e-4)
    torch.testing.assert_close(c("rewards"), ref["rewards"].reshape(-1), atol=5e-5, rtol=1e-3)
    grad = eng.merge_text(o["ln_grad"], o["text_grad"]).cpu()
    assert (grad - ref["grad"]).norm() / ref["grad"].norm() < 2e-3
    after = eng.merge_text(o["ln_after"], o["text_after"]).cpu()
    d = (after - ref["after"]).abs()
    print(f"[text tuning, ViT-B/16] {int((d > 0.1 * lr).sum())} of {d.numel()} tuned elements differ by > 0.1 lr")
    assert (d > 0.1 * lr).float().mean() < 0.01                          # Adam's sign on ~zero gradients
    torch.testing.assert_close(c("final_logits"), ref["final_logits"], atol=5e-3, rtol=0)
    eng.close()


@pytest.mark.parametrize("geo,n_views,n_cls", [("tiny", 8, 16), ("ViT-B/16", 64, 1000)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_prompt_step_bit_reproducible(L, dev, geo, n_views, n_cls, mode):
    """The prompt-tuning step gives the same BITS on every run: the only order-dependent sums of the path were the float atomics of
    the shared prefix rows' dK / dV in the text attention backward, now parked per sequence and added in sequence order
    (attention_bwd_prefix_reduce_kernel).  One-image calls and the sample-batched call, all three text layouts."""
    from rlcf_amd.engine import TTAConfig
    from test_gpu_parity import make_engine
    eng, *_ = make_engine((geo, geo if geo != "tiny" else "tiny-r"), n_views * 2, n_cls, mode, prec=L.PREC_F16X3)
    cfg = TTAConfig(selection_p=0.5 if geo == "tiny" else 0.1, tta_steps=2)
    R = synth.GEOMETRIES[geo].image_resolution
    vs = torch.stack([synth.make_views(1113 + i, n_views, R, device=dev) for i in range(2)])
    runs = [eng.tta_sample(vs[0], cfg) for _ in range(3)]
    for o in runs[1:]:
        for k in ("ctx_grad", "ctx_after", "final_logits", "dlogits"):
            assert torch.equal(o[k], runs[0][k]), k
    b0 = eng.tta_batch(vs, cfg, want_logits=True)[1].clone()
    for _ in range(2):
        assert torch.equal(eng.tta_batch(vs, cfg, want_logits=True)[1], b0)
    eng.close()


def test_retrieval_text_tuning_momentum_matches_oracle(L, dev):
    """CLIPRet_TTA.momentum_update_model on the text side (retrieval/custom_models.py:128-143, scripts/tta_coco_ret.sh setting 03): an
    EMA of the tuned text parameters across captions, folded into the reset state every update_freq captions.  Three captions,
    update_freq = 2: rlcf_tta_retrieval_text + rlcf_engine_momentum_update_text against the oracle's tune_text run from the oracle's
    own evolving reset state (oracle.rlcf_ref.momentum_update)."""
    from rlcf_amd.engine import Engine, TTAConfig
    from oracle import retrieval_ref as QR, rlcf_ref as RR2
    sg, rg = synth.GEOMETRIES["tiny"], synth.GEOMETRIES["tiny-r"]
    ssd, rsd = synth.make_state_dict(sg, 11), synth.make_state_dict(rg, 23)
    n, K, lr, m, w = 120, 6, 1e-3, 0.9, 0.5
    gen = torch.Generator().manual_seed(9)
    sbank = torch.nn.functional.normalize(torch.randn(n, sg.embed_dim, generator=gen), dim=-1)
    rbank = torch.nn.functional.normalize(torch.randn(n, rg.embed_dim, generator=gen), dim=-1)
    bank = synth.make_token_bank(sg, 16, seed=7, n_ctx=4)
    hp = RR2.TTAHyper(selection_p=1.0, tta_steps=1, sample_k=K, lr=lr, weight_decay=5e-4, eps=1e-6)
    cfg = TTAConfig(selection_p=1.0, tta_steps=1, sample_k=K, lr=lr, weight_decay=5e-4, eps=1e-6)
    eng = Engine(sg, rg, 8, n, L.PREC_F32)
    eng.load_state_dict(L.STUDENT, {k: v.to(dev) for k, v in ssd.items()})
    eng.load_state_dict(L.REWARD, {k: v.to(dev) for k, v in rsd.items()})
    eng.finalize()
    eng.set_image_bank(sbank.to(dev), rbank.to(dev))
    keys = QR.text_param_keys(ssd)
    vec = lambda d: torch.cat([d[k].reshape(-1) for k in keys])
    def unvec(v):
        out, off = {}, 0
        for k in keys:
            out[k] = v[off: off + ssd[k].numel()].reshape(ssd[k].shape).clone(); off += ssd[k].numel()
        return out
    clip = vec(ssd)
    init, mom = clip.clone(), clip.clone()
    for i, row in enumerate([5, 9, 12]):
        sd_i = dict(ssd); sd_i.update(unvec(init))
        ref = QR.tune_text(sd_i, rsd, bank[row][None], None, hp, student_bank=sbank, reward_bank=rbank)
        o = eng.tta_retrieval_text(bank[row], cfg)
        torch.cuda.synchronize()
        assert o["topk_idx"].cpu().reshape(-1).tolist() == ref["topk_idx"].reshape(-1).tolist()
        torch.testing.assert_close(o["logits"].cpu(), ref["logits"], atol=1e-3, rtol=0)             # (the reset state of caption i)
        torch.testing.assert_close(o["final_logits"].cpu(), ref["final_logits"], atol=3e-3, rtol=0)
        apply = (i + 1) % 2 == 0
        mom, new_init = RR2.momentum_update(mom, ref["after"], clip, m, w, apply)
        if new_init is not None:
            init = new_init
        eng.momentum_update_text(o["text_after"], o["ln_after"], m, w, apply)
        flat1, ln1 = eng.text_params(1)
        d = (eng.merge_text(ln1, flat1).cpu() - init).abs()
        assert float(d.max()) < 2e-4, f"reset state after caption {i}: max |delta| {float(d.max()):.3e}"
    eng.close()


def test_retrieval_ensemble_text_to_image(L, dev):
    """scripts/tta_coco_ret.sh settings 02 / 03 (multiple_reward_models = 1) in the text -> image direction: the retrieval
    CLIPRewardsMultiple mirror hands one image bank per reward model to the engine; the scores of the sampled images are the weighted
    sum of the per-model clamped similarities (retrieval/clip_reward.py:286-310) — checked against the oracle's per-model features."""
    from rlcf_amd import clip_ret_policy as P, clip_store, runtime
    from oracle import rlcf_ref as RR2
    runtime.reset_session()
    sg, rg = synth.GEOMETRIES["tiny"], synth.GEOMETRIES["tiny-r"]
    rsds = [synth.make_state_dict(rg, 23), synth.make_state_dict(rg, 29)]
    clip_store.register_checkpoint("student", sg, synth.make_state_dict(sg, 11))
    clip_store.register_checkpoint("ViT-L/14", rg, rsds[0])               # (names the CONFIDECES table knows: weights 5 : 1)
    clip_store.register_checkpoint("ViT-B/16", rg, rsds[1])
    tokens = synth.make_token_bank(sg, 16, seed=7, n_ctx=4)
    clip_store.set_tokenizer(lambda texts, context_length=77, truncate=False: tokens[[int(t.strip().rstrip(".").split("c")[-1]) for t in ([texts] if isinstance(texts, str) else texts)]])
    K = 6
    model = P.CLIPRet_TTA(dev, arch="student", only_visual=False)
    reward_model = P.CLIPRewardsMultiple(dev, arch=["ViT-L/14", "ViT-B/16"], sample_k=K, reward_process=True, process_batch=False)
    images = synth.make_views(3000, 96, sg.image_resolution, device=dev)
    model.set_image_features(images=images)
    reward_model.set_image_features(images=images)
    assert len(reward_model.image_features) == 2 and reward_model.image_features[0].shape == (96, rg.embed_dim)
    optimizer = torch.optim.AdamW(model.parameters(), lr=1e-4, eps=1e-6, weight_decay=5e-4)
    out = P.tune_text("c5.", model, reward_model, optimizer, None, args=types.SimpleNamespace(tta_steps=1))
    idx = out["topk_idx"].cpu().reshape(-1).long()
    assert idx.tolist() == torch.topk(out["logits"].cpu()[0], K).indices.tolist()
    w = torch.tensor(reward_model.weights)
    per = []
    for m in range(2):
        t = RR2.reward_class_features(rsds[m], tokens[5][None])                                        # [1, Dr]
        per.append((2.5 * reward_model.image_features[m].cpu()[idx] @ t[0]).clamp_min(0))
    want = (w[:, None] * torch.stack(per)).sum(0)
    torch.testing.assert_close(out["clip_score"].cpu(), want, atol=2e-5, rtol=1e-4)
    r = out["rewards"].cpu()
    torch.testing.assert_close(r, want - want.mean(), atol=2e-5, rtol=1e-3)
    model.reset_initial()
    runtime.reset_session()


def test_retrieval_mirror_tune_text(L, dev):
    """The reference-shaped objects (rlcf_amd.clip_ret_policy: CLIPRet_TTA(only_visual=False), CLIPRewards, tune_text) reproduce the
    fixture through the loop body of test_time_tune's text -> image part (clip_ret_policy.py:183-196): image features of both models
    set once, then per caption: tune, logits_per_text of the tuned model, reset."""
    import copy
    from rlcf_amd import clip_ret_policy as P, clip_store, runtime
    g, meta = load_golden("retrieval_t2i_tiny")
    runtime.reset_session()
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    clip_store.register_checkpoint("student", sg, synth.make_state_dict(sg, meta["student_seed"]))
    clip_store.register_checkpoint("reward", rg, synth.make_state_dict(rg, meta["reward_seed"]))
    tokens = synth.make_token_bank(sg, meta["bank_size"], seed=meta["bank_seed"], n_ctx=4)
    clip_store.set_tokenizer(lambda texts, context_length=77, truncate=False: tokens[[int(t.strip().rstrip(".").split("c")[-1]) for t in ([texts] if isinstance(texts, str) else texts)]])
    model = P.CLIPRet_TTA(dev, arch="student", only_visual=False)
    reward_model = P.CLIPRewards(dev, arch="reward", sample_k=meta["sample_k"], reward_process=True, process_batch=False)
    images = synth.make_views(meta["image_seed"], meta["n_images"], sg.image_resolution, device=dev)
    model.set_image_features(images=images)
    reward_model.set_image_features(images=images)
    optimizer = torch.optim.AdamW(model.parameters(), lr=meta["lr"], eps=meta["eps"], weight_decay=meta["weight_decay"])
    optim_state = copy.deepcopy(optimizer.state_dict())
    text = f"c{meta['query_row']}."
    args = types.SimpleNamespace(tta_steps=meta["tta_steps"])
    for rep in range(2):
        out = P.tune_text(text, model, reward_model, optimizer, None, args=args)
        assert out["topk_idx"].cpu().reshape(-1).tolist() == g["topk_idx"].reshape(-1).tolist()
        torch.testing.assert_close(reward_model.text_features.cpu(), g["reward_text"], atol=1e-5, rtol=0)
        logits_per_image, logits_per_text = model(images=None, text=text)
        torch.testing.assert_close(logits_per_text.cpu(), g["final_logits"], atol=5e-3, rtol=0)
        assert logits_per_image.shape == (meta["n_images"], 1)
        sc = reward_model.CLIPScore(text_index=None, images_index=g["topk_idx"].reshape(-1).to(dev), pairwise=False)
        torch.testing.assert_close(sc.cpu(), g["clip_score"].reshape(-1), atol=1e-5, rtol=1e-4)
        with pytest.raises(NotImplementedError, match="tuned on"):
            model(images=None, text="c6.")
        model.reset_initial()
        optimizer.load_state_dict(optim_state)
        _, pristine = model(images=None, text=text)
        torch.testing.assert_close(pristine.cpu(), g["logits"], atol=1e-3, rtol=0)
    runtime.reset_session()


@pytest.mark.parametrize("name", ["retrieval_t2i_loss", "retrieval_t2i_loss_amp"])
def test_retrieval_text_to_image_loss_matches_reference_fixture(L, dev, name):
    """Loss section of the reference's tune_text (clip_ret_policy.py:123-133) on the HIP loss kernel with the banks exchanged:
    rows = logits_per_text over the image bank, class_feat = the reward model's image features, reward_img = its query text feature."""
    from rlcf_amd import clip_ret_policy as P
    g, meta = load_golden(name)
    rm = types.SimpleNamespace(sample_k=meta["sample_k"], reward_process=True, amplify_rewards=bool(meta["reward_amplify"]), process_batch=False,
                               clipscore_weight=meta["clipscore_weight"], image_features=g["reward_images"].to(dev),
                               class_features=g["reward_text"].to(dev))
    o = P.text2image_loss(g["logits_per_text"].to(dev), rm)
    assert o["topk_idx"].cpu().reshape(-1).tolist() == g["topk_idx"].reshape(-1).tolist()
    torch.testing.assert_close(o["clip_score"].cpu(), g["clip_score"].reshape(-1), atol=1e-6, rtol=1e-5)
    torch.testing.assert_close(o["rewards"].cpu(), g["rewards"].reshape(-1), atol=1e-5, rtol=1e-3)
    torch.testing.assert_close(o["loss"].cpu()[0], g["loss"], atol=1e-7, rtol=1e-3)
    torch.testing.assert_close(o["dlogits"].cpu(), g["dlogits"], atol=1e-7, rtol=1e-3)


@pytest.mark.parametrize("prec", [0, 2])
def test_retrieval_text_to_image_tuning_matches_reference_fixture(L, dev, prec):
    """rlcf_tta_retrieval_text vs the reference's tune_text (retrieval/clip_ret_policy.py:106-137) with CLIPRet_TTA(only_visual=False)
    + the evaluation of its loop (:193-196): one query caption against a 200-image bank, K = 12 (the script's sample_k_t2i), two AdamW
    steps over every non-visual parameter (embeddings, text transformer, ln_final, text_projection, logit_scale)."""
    from rlcf_amd.engine import Engine, TTAConfig
    from oracle import retrieval_ref as QR
    from test_gpu_parity import _tensor_norms
    g, meta = load_golden("retrieval_t2i_tiny")
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    ssd, rsd = synth.make_state_dict(sg, meta["student_seed"], device=dev), synth.make_state_dict(rg, meta["reward_seed"], device=dev)
    eng = Engine(sg, rg, 64, max(meta["n_images"], 64), prec)
    eng.load_state_dict(L.STUDENT, ssd)
    eng.load_state_dict(L.REWARD, rsd)
    eng.finalize()
    images = synth.make_views(meta["image_seed"], meta["n_images"], sg.image_resolution, device=dev)
    sfeat = torch.cat([eng.encode_image(L.STUDENT, images[i: i + 64]) for i in range(0, meta["n_images"], 64)])
    rfeat = torch.cat([eng.encode_image(L.REWARD, images[i: i + 64]) for i in range(0, meta["n_images"], 64)])
    eng.set_image_bank(sfeat, rfeat)
    bank = synth.make_token_bank(sg, meta["bank_size"], seed=meta["bank_seed"], n_ctx=4)
    query = bank[meta["query_row"]]
    cfg = TTAConfig(selection_p=1.0, tta_steps=meta["tta_steps"], sample_k=meta["sample_k"], lr=meta["lr"], weight_decay=meta["weight_decay"],
                    eps=meta["eps"])
    for rep in range(2):                                                  # the second call starts from the reset state: same results
        o = eng.tta_retrieval_text(query, cfg)
        torch.cuda.synchronize()
        c = lambda k: o[k].cpu()
        assert c("topk_idx").reshape(-1).tolist() == g["topk_idx"].reshape(-1).tolist()
        torch.testing.assert_close(c("logits"), g["logits"], atol=1e-3, rtol=0)
        torch.testing.assert_close(c("reward_text_features"), g["reward_text"], atol=1e-5, rtol=0)
        torch.testing.assert_close(c("clip_score"), g["clip_score"].reshape(-1), atol=1e-5, rtol=1e-4)
        torch.testing.assert_close(c("rewards"), g["rewards"].reshape(-1), atol=5e-5, rtol=1e-3)
        torch.testing.assert_close(c("dlogits"), g["dlogits"], atol=1e-6, rtol=2e-3)
        torch.testing.assert_close(c("final_logits"), g["final_logits"], atol=5e-3, rtol=0)
        assert c("step_skipped").tolist() == [0] * meta["tta_steps"]
        keys = QR.text_param_keys(ssd)
        grad, after = eng.merge_text(o["ln_grad"], o["text_grad"]), eng.merge_text(o["ln_after"], o["text_after"])
        torch.testing.assert_close(_tensor_norms(ssd, keys, grad), g["grad_l2"], rtol=3e-3, atol=1e-9)
        torch.testing.assert_close(_tensor_norms(ssd, keys, after, ssd), g["delta_l2"], rtol=0.01, atol=1e-7)
        gs = grad[::7].cpu()
        assert (gs - g["grad_sample"]).norm() / g["grad_sample"].norm() < 2e-3
        d = (after[::7].cpu() - g["after_sample"]).abs()
        assert (d > 0.1 * meta["lr"]).float().mean() < 0.01              # Adam's sign on ~zero gradients
    # the image bank replaced the class bank: calls that need texts refuse
    with pytest.raises(L.RlcfError, match="class bank"):
        eng.tta_sample(images[:8], cfg)
    eng.close()


@pytest.mark.parametrize("prec", [0, 2])
def test_config5_full_geometry_matches_reference_fixture(L, dev, prec):
    """BASELINE configs[4] at FULL geometry against the reference's own run (tta_rn50x64_l14_n32: RN50x64 student on 448^2 views,
    ViT-L/14 reward model behind the bicubic 448 -> 224 resample, N = 32 views, 200 classes, prompt tuning): selected views, sampled
    classes, scores, rewards, prompt gradient / update, final logits and top-5 — through rlcf_tta_sample and, two copies per pass,
    through rlcf_tta_batch."""
    from test_gpu_parity import make_engine, _check_against, _cfg_from_meta as cfgm
    g, meta = load_golden("tta_rn50x64_l14_n32")
    eng, ssd, rsd, tokens, ctx0 = make_engine((meta["student"], meta["reward"]), meta["n_views"] * 2, meta["n_cls"], L.TEXT_SHARED,
                                              meta["student_seed"], meta["reward_seed"], meta["bank_seed"], meta["n_ctx"], prec=prec)
    views = synth.make_views(meta["view_seed"], meta["n_views"], synth.GEOMETRIES[meta["student"]].image_resolution, device=dev)
    o = eng.tta_sample(views, cfgm(meta, True))
    torch.cuda.synchronize()
    _check_against(o, g, meta)
    top5, fl = eng.tta_batch(torch.stack([views, views]), cfgm(meta, True), want_logits=True)
    for b in range(2):
        assert top5[b].cpu().tolist() == g["top5"].tolist()
        torch.testing.assert_close(fl[b].cpu(), g["final_logits"][0], atol=1e-3, rtol=0)
    eng.close()


def test_reward_ensemble_full_size_matches_reference_fixture(L, dev):
    """The reward ensemble at FULL size against the reference's own run (tta_b16_ensfull_n64: ViT-B/16 student, N = 64 views, 1000 classes,
    CLIPRewardsMultiple over the arch list get_reward_model really uses — ViT-L/14@336px, RN50x64 @448^2, ViT-L/14, weights
    [0.56, 0.17, 0.28] — each scoring the selected 224^2 views through its own bicubic align_corners=True resample), product-default
    split-f16 precision, through rlcf_tta_sample and rlcf_tta_batch."""
    from test_gpu_parity import make_ensemble_engine, _check_against, _cfg_from_meta as cfgm
    g, meta = load_golden("tta_b16_ensfull_n64")
    eng, members, tokens = make_ensemble_engine(meta, L.TEXT_SHARED, prec=L.PREC_F16X3, device=dev)
    eng.set_reward_mix(g["reward_weights"].tolist(), mean=not meta.get("weighted_scores", 1))
    for m in range(len(members)):
        torch.testing.assert_close(eng.reward_class_features(m).cpu()[::25], g[f"reward_class_features_{m}"], atol=2e-5, rtol=1e-4)
    views = synth.make_views(meta["view_seed"], meta["n_views"], synth.GEOMETRIES[meta["student"]].image_resolution, device=dev)
    o = eng.tta_sample(views, cfgm(meta, True))
    torch.cuda.synchronize()
    for m in range(len(members)):
        torch.testing.assert_close(o["reward_image_features"][m].cpu(), g[f"reward_image_features_{m}"], atol=3e-5, rtol=1e-4)
    _check_against(o, g, meta)
    top5 = eng.tta_batch(views[None], cfgm(meta, True))
    assert top5[0].cpu().tolist() == g["top5"].tolist()
    eng.close()


def test_ln_batch_matches_reference_at_full_size_l14_n64(L, dev):
    """BASELINE configs[2] at FULL size (ViT-L/14 + ViT-L/14, N = 64 views, C = 1000, LayerNorm tuning) through the sample-batched call
    rlcf_tta_batch_ln, two copies of the reference's sample per pass: top-5 and final logits of the reference's own run (ln_l14_n64)."""
    from rlcf_amd.engine import Engine
    g, meta = load_golden("ln_l14_n64")
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    eng = Engine(sg, rg, meta["n_views"] * 2, meta["n_cls"], L.PREC_F16X3)
    ssd_d = synth.make_state_dict(sg, meta["student_seed"], device=dev)       # (generated on the device: bit-identical to the CPU generator,
    eng.load_state_dict(L.STUDENT, ssd_d)                                      #  and a ViT-L/14 takes the CPU generator ~100 s)
    eng.load_state_dict(L.REWARD, synth.make_state_dict(rg, meta["reward_seed"], device=dev))
    eng.finalize()
    ssd_tok = ssd_d["token_embedding.weight"].cpu()
    tokens = synth.make_token_bank(sg, meta["n_cls"], seed=meta["bank_seed"], n_ctx=meta["n_ctx"])
    ctx0 = ssd_tok[torch.tensor(synth.ctx_token_ids_default(sg, meta["n_ctx"]))].clone()
    eng.set_class_bank(tokens, meta["n_ctx"], ctx0, L.TEXT_SHARED)
    views = synth.make_views(meta["view_seed"], meta["n_views"], sg.image_resolution, device=dev)
    top5, fl = eng.tta_batch_ln(torch.stack([views, views]), _cfg_from_meta(meta), want_logits=True)
    for b in range(2):
        assert top5[b].cpu().tolist() == g["top5"].tolist()
        torch.testing.assert_close(fl[b].cpu(), g["final_logits"][0], atol=1e-3, rtol=0)
    eng.close()


def test_ln_batch_matches_reference_stream_at_full_size_l14_n64(L, dev):
    """BASELINE configs[2] at FULL size as a STREAM of four consecutive test images (view seeds 1000..1003; tests/golden/make_golden.py
    --only lnl14stream: the harness body of TPT/tune_cls_rl.py:206-227 one image at a time, the LayerNorms reset in between): (1) all four in
    ONE rlcf_tta_batch_ln pass — top-5 identical, final logits within 1e-3 of the reference's own run; (2) one at a time through
    rlcf_tta_sample_ln — selected views, sampled classes, rewards and the LayerNorm gradient of every sample.  Reports the worst
    max|dlogit| and, per sample, how many LayerNorm elements sit within 1e-5 of zero gradient relative to the largest (the elements whose
    AdamW step, +-lr by the gradient's SIGN at step 1, the last bits of a float32 run decide: SURVEY section 0 fact 6)."""
    from rlcf_amd.engine import Engine
    if not os.path.exists(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ln_l14_n64_stream.npz")):
        pytest.skip("fixture not generated")
    g, meta = load_golden("ln_l14_n64_stream")
    n = meta["n_samples"]
    sg, rg = synth.GEOMETRIES[meta["student"]], synth.GEOMETRIES[meta["reward"]]
    eng = Engine(sg, rg, meta["n_views"] * n, meta["n_cls"], L.PREC_F16X3)
    ssd_d = synth.make_state_dict(sg, meta["student_seed"], device=dev)
    eng.load_state_dict(L.STUDENT, ssd_d)
    eng.load_state_dict(L.REWARD, synth.make_state_dict(rg, meta["reward_seed"], device=dev))
    eng.finalize()
    ssd_tok = ssd_d["token_embedding.weight"].cpu()
    tokens = synth.make_token_bank(sg, meta["n_cls"], seed=meta["bank_seed"], n_ctx=meta["n_ctx"])
    ctx0 = ssd_tok[torch.tensor(synth.ctx_token_ids_default(sg, meta["n_ctx"]))].clone()
    eng.set_class_bank(tokens, meta["n_ctx"], ctx0, L.TEXT_SHARED)
    views = torch.stack([synth.make_views(meta["view_seed0"] + i, meta["n_views"], sg.image_resolution, device=dev) for i in range(n)])
    cfg = _cfg_from_meta(meta)
    top5, fl = eng.tta_batch_ln(views, cfg, want_logits=True)
    worst = 0.0
    for i in range(n):
        assert top5[i].cpu().tolist() == g[f"top5_{i}"].tolist(), f"stream sample {i}"
        err = (fl[i].cpu() - g[f"final_logits_{i}"][0]).abs().max().item()
        worst = max(worst, err)
        assert err < 1e-3, f"stream sample {i}: max|dlogit| {err:.2e}"
    fragile = []
    for i in range(n):
        o = eng.tta_sample_ln(views[i], cfg)
        assert o["selected_idx"].cpu().tolist() == g[f"selected_idx_{i}"].tolist()
        assert o["topk_idx"].cpu().reshape(-1).tolist() == g[f"topk_idx_{i}"].reshape(-1).tolist()
        torch.testing.assert_close(o["rewards"].cpu(), g[f"rewards_{i}"].reshape(-1), atol=5e-5, rtol=1e-3)
        torch.testing.assert_close(o["final_logits"].cpu(), g[f"final_logits_{i}"], atol=1e-3, rtol=0)
        gr, og = g[f"ln_grad_{i}"], o["ln_grad"].cpu()
        assert gr.norm() > 0 and (og - gr).norm() / gr.norm() < 2e-3
        fragile.append(int((gr.abs() < 1e-5 * gr.abs().max()).sum()))
    print(f"[configs[2] stream] {n} samples in one pass: worst max|dlogit| = {worst:.2e}; sign-fragile LayerNorm elements per sample "
          f"(|g| < 1e-5 max|g|, of {gr.numel()}): {fragile}")
    eng.close()
