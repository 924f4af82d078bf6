#!/usr/bin/env python3
"""RLCF hot-path benchmark: test-images/sec of the per-sample test-time-adaptation step.

A "step" = one test image: N augmented 224x224 views -> student ViT-B/16 image tower, prompt text tower
over a C-class bank, confidence selection, frozen reward CLIP on the selected views, top-K CLIP-reward
REINFORCE loss, backward to the prompt, AdamW, final clean-view inference, top-5 (reference:
TPT/tpt_cls_rl.py:219-279 with TPT/scripts/rlcf-prompt.sh hyper-parameters).  Defaults = BASELINE.json
configs[1] (N=64, C=1000, ViT-B/16 reward, 1 AdamW step).

Inputs (seeded synthetic views, weights, token bank) are resident in HBM before the timed region.  One process
per GPU; independent test images shard across ranks with no collective on the data path; only the barrier and
the max-over-ranks of the elapsed time use RCCL.  `--total-images T` switches from weak scaling (every rank times
`--steps` images of its own) to strong scaling (T images split over the ranks with rlcf_amd.shard.shard_range).

Legs, in order (all on the launch stream of the engine = torch's current stream):
  1. warm-up (`--warmup` images, untimed) and the TIMED region: exactly `--steps` images, barrier + synchronize on
     both sides, max over ranks -> `value`, `ms_per_step`; run `--timed-repeats` times (default 1; 2 with `--full`) and the SLOWEST
     region is the one reported (`timed_regions_seconds` lists them all).  `--dump-outputs DIR` then writes what the last timed region
     returned (`top5`, `final_logits`) as DIR/<name>.npy.  A plain run stops here; legs 2-5 run with `--full` only:
  2. sustained leg: full passes repeated for >= `--sustain-seconds` with a HIP event pair per pass -> mean / p50 / min / max ms
     per image (`sustained`; N=1 runs).  Multi-rank runs: every rank first settles its GPU's clock with untimed passes
     (`--settle-seconds`), the timed region reports each rank's own seconds and the slowest / fastest ratio, and the sustained leg
     runs on EVERY rank concurrently (`distributed.sustained`: per-rank and aggregate images/s);
  3. roofline leg: ONE pass of exactly the pass size the timed region ran, with a HIP event pair round every GEMM and
     attention launch (rlcf_profile_*): dominant-kernel rate, per-shape table of the ViT-B/16 layer kernels (K4-K7);
  4. secondary lines of configs[1]: the single-pass f16 mode, checkpoint-grid weights, the drop-in harness loop;
  5. cpu_baseline: the oracle (CPU restatement of the reference graph) on BASELINE configs[0] — N=8 views,
     selection_p=0.5, C=`--classes` — 1 warm-up + 3 timed samples on the host cores.

`--config {0,1,2,4}` selects the BASELINE.json configuration (default 1 = the one `metric` is quoted on; 3 is config 1 sharded
over 8 GPUs: `--gpus 8 --total-images 256`):
  0  ViT-B/16 + ViT-B/16, N = 8 views, selection_p = 0.5, prompt tuning      (the reference's CPU-runnable case)
  1  ViT-B/16 + ViT-B/16, N = 64, prompt tuning                               (rlcf_tta_batch)
  2  ViT-L/14 + ViT-L/14, N = 64, LayerNorm tuning of the image encoder        (rlcf_tta_batch_ln, TPT/tune_cls_rl.py:183-256)
  4  RN50x64 student @448 + ViT-L/14 reward, N = 32, prompt tuning             (one image per pass)
With `--full` every config prints the same JSON shape: whole-step TF/s, F_exec per image, the dominant kernel's roofline and a per-kernel table
built from ALL profiled launches of one pass (GEMMs by kernel kind and shape incl. the weight-gradient / dX GEMMs, attention forward
and backward, LayerNorm forward and backward).

Prints ONE JSON line on rank 0.  With `--full`, the numbers a review leans on are repeated as FLAT top-level keys next to `value`
(`value_sustained`, `roofline_frac`, `f16_images_per_s`, `f16_in_proj_frac`, `f16_c_fc_frac`, `f16_attention_frac`,
`f16_lnfold_*`, `grid_weights_images_per_s`, `harness_one_image_per_call`, `harness_three_in_flight`, ...).
"""
import os as _os
if int(_os.environ.get("WORLD_SIZE", "1")) == 1:         # one rank: the CPU-oracle leg pins one thread per core (read at OpenMP start-up)
    _os.environ.setdefault("OMP_PROC_BIND", "close")
    _os.environ.setdefault("OMP_PLACES", "cores")
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

from rlcf_amd import _lib, shard, synth  # noqa: E402
from rlcf_amd.engine import Engine, TTAConfig  # noqa: E402

PEAK_TFLOPS = {"f32": 157.3, "f16": 2500.0}      # /opt/skills/guides/MI355X_MICROARCH.md (dense MFMA peaks; f16 = bf16 rate)
HBM_PEAK_GBS = 8000.0                              # HBM3E, same guide
PRECISIONS = {"f32": _lib.PREC_F32, "f16x3": _lib.PREC_F16X3, "f16": _lib.PREC_F16}
MFMA_PASSES = {"f32": 1, "f16x3": 3, "f16": 1}
DTYPE = {"f32": "f32", "f16x3": "f32 via split-f16x3 MFMA", "f16": "f16 forward pipeline (one MFMA per product, f32 accumulate): NOT parity-grade"}


def cpu_model() -> str:
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


T_START = time.perf_counter()


def log(msg: str) -> None:
    """progress on stderr (stdout carries the one JSON line)"""
    print(f"[bench {time.perf_counter() - T_START:7.1f}s] {msg}", file=sys.stderr, flush=True)


def cpu_baseline(ssd, rsd, geo, n_cls, n_ctx=4, timed=3, budget_s=300.0):
    """the oracle (CPU torch fp32 restatement of the REFERENCE GRAPH: dense 77-token text tower with
    autograd tape, dense backward, AdamW, final inference) on BASELINE configs[0] — ViT-B/16 + ViT-B/16, one image -> N=8 views,
    selection_p=0.5, the full class bank — 1 warm-up + `timed` timed samples at the full class count; no extrapolation.
    Threads: the fastest of a 32 / 64 / 128 sweep (see below).
    `budget_s` bounds the leg: timed samples stop early (at least one is taken) once it is spent."""
    from oracle import clip_ref as CR, rlcf_ref as RR
    t_leg = time.perf_counter()
    ncpu = os.cpu_count() or 1
    ctx0 = CR.ctx_from_tokens(ssd, synth.ctx_token_ids_default(geo, n_ctx))
    hp = RR.TTAHyper(selection_p=0.5)

    def one(seed, tokens, rc):
        views = synth.make_views(seed, 8, geo.image_resolution)
        t0 = time.perf_counter()
        RR.tta_sample(ssd, rsd, views, tokens, ctx0, hp, reward_cls=rc)
        return time.perf_counter() - t0

    # Threads: BASELINE.md asks for os.cpu_count(); on the GPU boxes of this pool (hundreds of hardware threads) torch's intra-op pool
    # then thrashes so badly that a 1.5 s probe sample (32 classes) did not finish in ten minutes (round-2 measurement), so the pool
    # is capped at 32 threads — the count is reported as `cores`, the host's total as `hardware_threads`.
    # Round 3: the thread count is SWEPT — one probe sample at a 64-class bank per candidate (32 / 64 / 128 threads, never more than the
    # host has; OMP_PROC_BIND=close, OMP_PLACES=cores set at the top of this file) — and the fastest runs the timed samples.
    cands = sorted({t for t in (32, 64, 128) if t <= ncpu} or {ncpu})
    probe_tokens = synth.make_token_bank(geo, 64, seed=7, n_ctx=n_ctx)
    probe_rc = RR.reward_class_features(rsd, probe_tokens)
    sweep = {}
    for t_ in cands:
        torch.set_num_threads(t_)
        one(998, probe_tokens, probe_rc)                        # (first call at a thread count: pool start-up)
        sweep[t_] = one(997, probe_tokens, probe_rc)
        log(f"cpu_baseline thread sweep: {t_} threads -> {sweep[t_]:.2f} s per image at C=64")
        if time.perf_counter() - t_leg > 0.3 * budget_s:
            break
    threads = min(sweep, key=sweep.get)
    torch.set_num_threads(threads)
    tokens = synth.make_token_bank(geo, n_cls, seed=7, n_ctx=n_ctx)
    rc = RR.reward_class_features(rsd, tokens)              # once per dataset in the reference (tpt_cls_rl.py:182-183): not timed
    warm = one(999, tokens, rc)
    log(f"cpu_baseline warm-up at C={n_cls}, {threads} threads: {warm:.1f} s")
    times = []
    for i in range(timed):
        times.append(one(1000 + i, tokens, rc))
        log(f"cpu_baseline sample {i}: {times[-1]:.1f} s")
        if time.perf_counter() - t_leg > budget_s:
            break
    mean = sum(times) / len(times)
    return {"value": 1.0 / mean, "unit": "images/s", "cores": threads, "kind": "port",
            "sample": f"oracle (CPU torch fp32, dense-77 reference graph, no structural shortcuts) on BASELINE configs[0]: ViT-B/16 + ViT-B/16, "
                      f"1 image x N=8 views (selection_p=0.5 -> 4 selected), C={n_cls}, K=3, 1 AdamW step; 1 warm-up + {len(times)} timed "
                      f"samples, {threads} torch threads of {ncpu} hardware threads",
            "seconds_per_image": [round(t, 3) for t in times], "seconds_per_image_mean": mean, "warmup_seconds": round(warm, 3),
            "cpu_model": cpu_model(), "hardware_threads": ncpu,
            "thread_sweep_seconds_at_64_classes": {str(k): round(v, 3) for k, v in sweep.items()}}


def harness_leg(dev, student_arch, reward_arch, ssd, rsd, n_cls, n_views, selection_p, lr, n_one=48, n_batched=96, ipp=32, one_only=False):
    """The DROP-IN path: what a maintainer runs after INTEGRATION.md section A — the reference's harness loop
    (TPT/tpt_cls_rl.py:219-279) through this package's mirror: rlcf_amd.tpt_cls_rl.test_time_adapt_eval, model / reward objects from
    get_coop / get_reward_model, views from rlcf_amd.datautils.AugMixAugmenter (rlcf_make_views on the device from ONE decoded uint8
    image, the reference's random crop boxes drawn on the host) — one image at a time as the reference feeds it, and with
    `images_per_pass` test images per engine call.  Reported beside `value`; never the headline (the loader's host work is in it)."""
    import copy
    import types
    from rlcf_amd import clip_reward, clip_store, custom_clip, datautils, runtime, tpt_cls_rl
    runtime.reset_session()
    sg, rg = synth.GEOMETRIES[student_arch], synth.GEOMETRIES[reward_arch]
    clip_store.register_checkpoint(student_arch, sg, ssd)
    clip_store.register_checkpoint(reward_arch + "#r", rg, rsd)
    bank = clip_store.SyntheticBank(sg, n_cls, 4, 7)
    clip_store.set_tokenizer(bank.tokenize)
    args = types.SimpleNamespace(tta_steps=1, selection_p=selection_p, gpu=dev.index or 0, tpt=True, print_freq=10 ** 9, min_entropy_reg=0,
                                 min_entropy_w=0.2, reward_arch=reward_arch + "#r", multiple_reward_models=0, weighted_scores=1, sample_k=3,
                                 reward_amplify=False, reward_process=True, process_batch=False)
    model = custom_clip.get_coop(student_arch, "I", dev, 4, "a_photo_of_a", classnames=bank.classnames)
    for name, p_ in model.named_parameters():                   # tpt_cls_rl.py:103-105
        if "prompt_learner" not in name:
            p_.requires_grad_(False)
    optimizer = torch.optim.AdamW(model.prompt_learner.parameters(), lr, weight_decay=5e-4)
    optim_state = copy.deepcopy(optimizer.state_dict())
    reward_model = clip_reward.get_reward_model(dev, args)
    model.reset_classnames(bank.classnames, student_arch)
    reward_model.set_class_features(tokenized_classes=model.prompt_learner.tokenized_prompts)
    aug = datautils.AugMixAugmenter(None, None, n_views=n_views - 1, augmix=False, resolution=sg.image_resolution, device=dev)
    gen = torch.Generator().manual_seed(3)
    photos = [torch.randint(0, 256, (375, 500, 3), dtype=torch.uint8, generator=gen) for _ in range(8)]      # decoded test images (ImageNet-sized)

    class Loader:                                            # one (list of N views [1, 3, R, R], target) per test image, views made on the device
        def __init__(self, n, staged=None):
            self.n, self.staged = n, staged
            self.on_device = staged is None                  # (views made on the device inside next(): tpt_cls_rl._eval_in_flight advances it under the lane's stream)

        def __len__(self):
            return self.n

        def __iter__(self):
            if self.staged is None:
                # views made IN the loop: the decoded image and its 63 crop boxes come from a loader thread one or two images ahead
                # (datautils.ViewPrefetcher — what the reference's DataLoader workers do, TPT/tpt_cls_rl.py:187-188), the device half
                # (rlcf_make_views) is launched by the loop's own thread
                pf = datautils.ViewPrefetcher([(photos[i % len(photos)], i % n_cls) for i in range(self.n)], aug)
                yield from pf
                loader_stats.append({k: (round(v, 4) if isinstance(v, float) else v) for k, v in pf.stats.items()})
                return
            for i in range(self.n):
                v = self.staged[i % len(self.staged)]
                yield [x.unsqueeze(0) for x in v.unbind(0)], torch.tensor([i % n_cls])

    loader_stats = []                                           # one entry per views-in-loop run: the loop thread's seconds waiting for the loader / in `apply`

    def run(n, images_per_pass, staged, in_flight=1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tpt_cls_rl.test_time_adapt_eval(Loader(n, staged), model, optimizer, optim_state, None, args, reward_model=reward_model,
                                        images_per_pass=images_per_pass, in_flight=in_flight)
        torch.cuda.synchronize()
        return n / (time.perf_counter() - t0)

    def ViewPrefetcher_probe(phs):
        return datautils.ViewPrefetcher([(ph, 0) for ph in phs] * 4, aug)

    staged = [aug.views(ph) for ph in photos]
    out = {"what": "rlcf_amd.tpt_cls_rl.test_time_adapt_eval (mirror of TPT/tpt_cls_rl.py:219-279) on a synthetic stream of 375x500 uint8 images; "
                   "views by rlcf_amd.datautils.AugMixAugmenter -> rlcf_make_views, the crop boxes drawn one or two images ahead on a loader thread "
                   "(datautils.ViewPrefetcher; the reference: DataLoader workers); 'staged' rows re-use pre-made view tensors (the loop alone)",
           "views": n_views, "classes": n_cls}
    run(4, 1, staged)                                         # warm-up: engine build, class bank, workspaces
    out["images_per_s_one_image_per_pass_staged_views"] = run(n_one, 1, staged)
    out["images_per_s_one_image_per_pass_views_in_loop"] = run(n_one, 1, None)
    # still one image per engine call, two samples in flight on two engines / two streams (test_time_adapt_eval(in_flight=2)): one sample's
    # few-row tail runs under the next sample's 64-view tower pass; per-sample results are the one-at-a-time call's
    # round 6: ONE host thread enqueues every lane (rlcf_lanes_submit, events between the streams); round 5 ran a Python thread per lane and
    # its legs scattered 72-116 images/s for one setting.  Every in-flight row is still the median of three legs, all three kept next to it
    # (legs are kept in RUN ORDER, with the loop thread's own account of a views-in-loop leg next to them — seconds waiting for the loader
    #  thread / inside `apply`.  That account found round 6's bimodal legs, 70 - 82 against 91 - 97 images/s: the decoded image was copied from
    #  PAGEABLE memory, which blocks the host until the device has run the copy, behind whatever shared its hardware queue — a lane's whole step
    #  in the legs where the streams fell that way.  The image is pinned on the loader thread now: datautils._upload.)
    def run3(key, st, k):
        if st is None:
            run(12, 1, None, k)
        n0 = len(loader_stats)
        legs = [run(2 * n_one, 1, st, k) for _ in range(3)]
        out[key], out[key + "_legs"] = sorted(legs)[1], [round(x, 2) for x in legs]
        if st is None:
            out[key + "_legs_loop_thread"] = loader_stats[n0:]
        if key.endswith("three_in_flight_staged_views"):
            out["three_in_flight_staged_legs_max_over_min"] = max(legs) / min(legs)
        if key.endswith("three_in_flight_views_in_loop"):
            out["three_in_flight_views_in_loop_legs_max_over_min"] = max(legs) / min(legs)

    run(12, 1, None)                                          # (views made in the loop allocate per image: let the caching allocator reach its steady pool first)
    run(4, 1, staged, 2)                                      # (builds the second engine)
    run3("images_per_s_one_image_per_pass_two_in_flight_staged_views", staged, 2)
    run3("images_per_s_one_image_per_pass_two_in_flight_views_in_loop", None, 2)
    run(6, 1, staged, 3)
    run3("images_per_s_one_image_per_pass_three_in_flight_staged_views", staged, 3)
    run3("images_per_s_one_image_per_pass_three_in_flight_views_in_loop", None, 3)
    if not one_only:
        run(ipp, ipp, staged)                                     # (batched workspaces)
        out[f"images_per_s_{ipp}_images_per_pass_staged_views"] = run(n_batched, ipp, staged)
        out[f"images_per_s_{ipp}_images_per_pass_views_in_loop"] = run(n_batched, ipp, None)
    t0 = time.perf_counter()
    for ph in photos:
        aug.views(ph)
    torch.cuda.synchronize()
    out["view_generation_ms_per_image"] = (time.perf_counter() - t0) / len(photos) * 1e3          # draws + device half, one thread, nothing overlapped
    t0 = time.perf_counter()
    for _ in ViewPrefetcher_probe(photos):
        pass
    torch.cuda.synchronize()
    out["view_generation_ms_per_image_prefetched"] = (time.perf_counter() - t0) / (4 * len(photos)) * 1e3   # what the loop's thread pays with the draws on the loader thread
    runtime.reset_session()
    return out


def dump_outputs(dirname, arrays, limit_bytes=64 << 20):
    """`--dump-outputs`: each [rows, ...] array as DIR/<name>.npy in float32 (class indices are exact in float32).  Over `limit_bytes`
    in all, a fixed seeded sample of the rows, the same for every array, is written instead and its row indices go to rows.npy."""
    import numpy as np
    os.makedirs(dirname, exist_ok=True)
    arrays = {k: v.detach().float().cpu() for k, v in arrays.items()}
    n = next(iter(arrays.values())).shape[0]
    per_row = sum(v[0].numel() * 4 for v in arrays.values())
    if n * per_row > limit_bytes:
        keep = max(1, (limit_bytes - 8 * n) // per_row)
        rows = torch.randperm(n, generator=torch.Generator().manual_seed(0))[:keep].sort().values
        arrays = {k: v[rows] for k, v in arrays.items()}
        np.save(os.path.join(dirname, "rows.npy"), rows.numpy().astype(np.float64))
    for k, v in arrays.items():
        np.save(os.path.join(dirname, k + ".npy"), v.numpy())
    log(f"outputs of the last timed region -> {dirname}: " + ", ".join(f"{k} {tuple(v.shape)}" for k, v in arrays.items()))


def profile_entries(lib):
    """per-launch records of the roofline leg: (kind, ms, flops, (d0, d1, d2))"""
    out = []
    for i in range(lib.rlcf_profile_count()):
        kind, ms, fl, dims = C.c_int(0), C.c_double(0), C.c_double(0), (C.c_int * 3)()
        _lib.check(lib.rlcf_profile_entry(i, C.byref(kind), C.byref(ms), C.byref(fl), dims))
        out.append((kind.value, ms.value, fl.value, tuple(dims)))
    return out


KIND_NAMES = {0: "gemm_nt_f32 (f32 MFMA)", 1: "gemm_nt_f16x3 128x128 (DMA ring / split-K / register-staged)", 2: "gemm_nt_f16x3_v2 256x128",
              3: "gemm_nt_f16x3_v3i 256x256", 4: "gemm_skinny_x3 (M <= 256: A split in the kernel)", 5: "gemm_nt_f16x3_v3i 192x256", 10: "attention forward (QK^T, softmax, PV)", 11: "LayerNorm forward -> operand pairs (HBM-bound)",
              12: "attention backward (dQ, dK, dV)", 13: "LayerNorm backward (HBM-bound)"}
HBM_KINDS = (11, 13)
CONFIGS = {
    # (96 images of 8 views per tower pass: 388 images/s at 32, 410 at 64, 417 at 96-160)
    0: dict(student="ViT-B/16", reward="ViT-B/16", views=8, selection_p=0.5, mode="prompt", lr=7e-3, batch=96, steps=192, warmup=96,
            what="BASELINE configs[0]: ViT-B/16, 1 image x N=8 views, 1000-class bank, 1 AdamW step on the prompt"),
    1: dict(student="ViT-B/16", reward="ViT-B/16", views=64, selection_p=0.1, mode="prompt", lr=7e-3, batch=32,
            what="BASELINE configs[1]: ViT-B/16 student + ViT-B/16 reward, N=64, prompt-tuning RLCF"),
    # (images per tower pass is the engine's own batching: 20 fills the tile rounds of the tuned path's GEMMs — 6 selected views x 20 x 257
    # tokens = 121 row tiles — where 16 left 6.06 / 1.52 rounds: 40.6 -> 39.7 ms/image on one box)
    2: dict(student="ViT-L/14", reward="ViT-L/14", views=64, selection_p=0.1, mode="ln", lr=1e-5, batch=20, steps=60, warmup=20,
            what="BASELINE configs[2]: ViT-L/14 student + ViT-L/14 reward, N=64, LayerNorm tuning of the image encoder"),
    # (8 images per tower pass: the convolutions' GEMMs see 256 views — 72.6 ms/image one at a time, 69.9 at 4, 66.0 at 8, 65.9 at 16)
    # the setting the paper ships (TPT/scripts/rlcf-prompt.sh:13-41): ViT-B/16 student, ViT-L/14 reward model, 3 AdamW steps per test image
    5: dict(student="ViT-B/16", reward="ViT-L/14", views=64, selection_p=0.1, mode="prompt", lr=7e-3, batch=20, steps=40, warmup=20, tta_steps=3,
            what="rlcf-prompt.sh (TPT/scripts/rlcf-prompt.sh:13-41): ViT-B/16 student + ViT-L/14 reward, N=64, 3 prompt-tuning steps per image"),
    4: dict(student="RN50x64", reward="ViT-L/14", views=32, selection_p=0.1, mode="prompt", lr=7e-3, batch=8, steps=32, warmup=8,
            what="BASELINE configs[4]: RN50x64 image encoder student @448 + ViT-L/14 reward, N=32, prompt tuning"),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None, help="timed test images (default: 64; configs 2 / 4: a multiple of their images per pass)")
    ap.add_argument("--warmup", type=int, default=None, help="untimed warm-up images (default: 32; configs 2 / 4: one pass)")
    ap.add_argument("--config", type=int, default=1, choices=sorted(CONFIGS), help="BASELINE.json configs[i] (3 = config 1 with --gpus 8 --total-images 256); 5 = the shipped script rlcf-prompt.sh")
    ap.add_argument("--views", type=int, default=None)
    ap.add_argument("--classes", type=int, default=1000)
    ap.add_argument("--text-mode", default="shared", choices=["dense", "packed", "shared"])
    ap.add_argument("--precision", default="f16x3", choices=sorted(PRECISIONS))
    ap.add_argument("--reward-arch", default=None, help="reward CLIP (BASELINE configs[1]: ViT-B/16; rlcf-prompt.sh: ViT-L/14)")
    ap.add_argument("--tta-steps", type=int, default=None, help="AdamW steps per test image (BASELINE metric: 1; rlcf-prompt.sh = --config 5 runs 3)")
    ap.add_argument("--batch", type=int, default=None, help="independent test images per tower pass (engine-internal batching)")
    ap.add_argument("--total-images", type=int, default=0,
                    help="strong scaling: this many test images in total, split over the ranks (BASELINE configs[3]: 256); overrides --steps")
    ap.add_argument("--sustain-seconds", type=float, default=3.0, help="length of the sustained leg (0 = skip)")
    ap.add_argument("--timed-repeats", type=int, default=None,
                    help="how many times the timed region (exactly --steps images, barrier + synchronize on both sides) is run; the slowest is "
                         "`value` (default: 1; 2 with --full)")
    ap.add_argument("--settle-seconds", type=float, default=1.0,
                    help="multi-rank runs: untimed passes of the timed pass size for this long before the barrier (clock / power settle)")
    ap.add_argument("--weights", default="fp32", choices=["fp32", "fp16grid"],
                    help="fp32: arbitrary float32 random-init weights (the headline: three MFMA passes per product); fp16grid: the same weights rounded to "
                         "fp16 values where a released CLIP checkpoint stores fp16 (two exact passes; see secondary_checkpoint_grid_weights)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-baseline-budget", type=float, default=300.0, help="seconds after which no further timed CPU sample is started")
    ap.add_argument("--no-f16-line", action="store_true", help="skip the secondary single-pass f16 measurement (RLCF_PREC_F16, not parity-grade)")
    ap.add_argument("--no-harness-leg", action="store_true", help="skip the drop-in harness measurement (test_time_adapt_eval through the mirror)")
    ap.add_argument("--no-roofline", action="store_true", help="skip the per-launch profiling leg (rocprofv3 runs: fewer launches in the trace)")
    ap.add_argument("--dist-backend", default="nccl", choices=["nccl", "gloo"],
                    help="nccl (= RCCL) for real multi-GPU runs; gloo lets two ranks share one GPU in a smoke test")
    ap.add_argument("--full", action="store_true",
                    help="also run every leg beyond the headline: a second timed region, the roofline, sustained, secondary f16 / grid-weights, "
                         "harness and CPU-baseline legs (each --no-* / --sustain-seconds switch above still applies)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed region computed (rank 0: top5, final_logits) as DIR/<name>.npy, float32, at most 64 MB")
    a = ap.parse_args()
    # `python bench.py --gpus N` typed without a launcher: become N ranks under torch.distributed.run (rlcf_amd/shard.py)
    rc = shard.self_launch(a.gpus, sys.argv[1:])
    if rc is not None:
        sys.exit(rc)
    wl = CONFIGS[a.config]
    if a.steps is None: a.steps = wl.get("steps", 64)
    if a.warmup is None: a.warmup = wl.get("warmup", 32)
    a.views = a.views if a.views is not None else wl["views"]
    if a.tta_steps is None: a.tta_steps = wl.get("tta_steps", 1)
    if a.timed_repeats is None: a.timed_repeats = 2 if a.full else 1
    a.reward_arch = a.reward_arch or wl["reward"]
    student_arch, mode_ln = wl["student"], wl["mode"] == "ln"
    is_default_wl = (a.views, a.reward_arch, a.classes, a.tta_steps) == (wl["views"], wl["reward"], 1000, wl.get("tta_steps", 1))

    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    assert world == a.gpus, f"--gpus {a.gpus} but WORLD_SIZE={world}"
    local = shard.local_device(local, a.dist_backend)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    use_dist = world > 1 or bool(os.environ.get("RLCF_FORCE_DIST"))     # RLCF_FORCE_DIST: exercise the RCCL path with one rank
    dist_info = None
    if world > 1:
        # one process per GPU on one host: each rank keeps to its own slice of the host cores (view generation and launches are
        # host work: 8 ranks with the default intra-op pool of 256 threads each would thrash)
        ncpu = os.cpu_count() or 1
        per = max(1, ncpu // world)
        torch.set_num_threads(min(per, 16))
        try:
            os.sched_setaffinity(0, set(range(local * per, (local + 1) * per)))
        except (AttributeError, OSError):
            pass
    if use_dist:
        import torch.distributed as dist
        if a.dist_backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group("gloo")
        try:
            ver = torch.cuda.nccl.version() if a.dist_backend == "nccl" else None
        except Exception:           # (not every build exposes it)
            ver = None
        dist_info = {"backend": a.dist_backend + (" (RCCL)" if a.dist_backend == "nccl" else ""), "rccl_ranks": dist.get_world_size(),
                     "rccl_version": ".".join(str(v) for v in ver) if ver else None,
                     "collectives": "barriers + all_reduce(MAX) of the elapsed time + all_gather of per-rank seconds; none on the data path"}

    geo = synth.GEOMETRIES[student_arch]
    n_ctx = 4
    ssd = synth.make_state_dict(geo, 11, device=dev)
    rgeo = synth.GEOMETRIES[a.reward_arch]
    rsd = synth.make_state_dict(rgeo, 23, device=dev)
    if a.weights == "fp16grid":
        ssd, rsd = synth.to_fp16_grid(ssd), synth.to_fp16_grid(rsd)
    tokens = synth.make_token_bank(geo, a.classes, seed=7, n_ctx=n_ctx)
    ctx0 = ssd["token_embedding.weight"][torch.tensor(synth.ctx_token_ids_default(geo, n_ctx), device=dev)].clone()
    batch = max(a.batch if a.batch is not None else wl["batch"], 1)
    eng = Engine(geo, rgeo, a.views * batch, a.classes, PRECISIONS[a.precision])
    eng.load_state_dict(_lib.STUDENT, ssd)
    eng.load_state_dict(_lib.REWARD, rsd)
    eng.finalize()
    mode = {"dense": _lib.TEXT_DENSE, "packed": _lib.TEXT_PACKED, "shared": _lib.TEXT_SHARED}[a.text_mode]
    eng.set_class_bank(tokens, n_ctx, ctx0, mode)
    log("engine ready")
    cfg = TTAConfig(selection_p=wl["selection_p"], tta_steps=a.tta_steps, sample_k=3, lr=wl["lr"], weight_decay=5e-4)
    run_pass = (lambda v: eng.tta_batch_ln(v, cfg, want_logits=True)) if mode_ln else (lambda v: eng.tta_batch(v, cfg, want_logits=True))

    # which test images this rank times: weak scaling = `steps` images of its own; strong = its shard of a fixed stream
    if a.total_images > 0:
        lo, hi = shard.shard_range(a.total_images, rank, world)
        first, steps, scaling, total_steps = 1000 + lo, hi - lo, "strong", a.total_images
    else:
        first, steps, scaling, total_steps = 1000 + rank * (a.warmup + a.steps) + a.warmup, a.steps, "weak", a.steps * world
    assert steps > 0, "no test image for this rank"
    pass_images = min(batch, steps)                      # images per tower pass in the timed region (its last pass may be smaller)

    def make(seed0, n):
        return torch.stack([synth.make_views(seed0 + i, a.views, geo.image_resolution, device=dev) for i in range(n)])

    wviews = make(first - a.warmup, max(a.warmup, pass_images))     # seeds are per sample; warm-up images differ
    views = make(first, steps)
    torch.cuda.synchronize()

    run_pass(wviews[:pass_images])                       # engine setup: sizes the batch workspaces once (not a step)
    torch.cuda.synchronize()
    if a.warmup:
        run_pass(wviews[: a.warmup])
    torch.cuda.synchronize()
    settle = 0
    if use_dist and a.settle_seconds > 0:
        # multi-rank runs: the timed region is ONE short pass per rank, so every rank first brings its GPU to the clock / power state
        # of the steady loop (untimed passes of the timed pass size) — otherwise the first N-GPU number measures clock ramp and
        # launch skew, not the step
        t_end = time.perf_counter() + a.settle_seconds
        while time.perf_counter() < t_end:
            run_pass(wviews[:pass_images])
            torch.cuda.synchronize()
            settle += 1
    # The timed region — exactly `steps` images per rank between barrier + synchronize on both sides — is run `--timed-repeats` times
    # back to back (default 2) and the SLOWER one is reported: at the driver's command line (--steps 20) a region is ONE 0.17-s pass,
    # and one pass alone can sit on a clock ramp either way.  Every region's seconds are in the line (`timed_regions_seconds`).
    regions = []
    for _ in range(max(1, a.timed_repeats)):
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        top5, final_logits = run_pass(views)
        torch.cuda.synchronize()
        own_ = time.perf_counter() - t0                  # this rank's own K steps (before it waits for the others)
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        regions.append((time.perf_counter() - t0, own_))
    cdev = dev if a.dist_backend == "nccl" else "cpu"
    region_dt = [r[0] for r in regions]
    if use_dist:
        t = torch.tensor(region_dt, device=cdev, dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)         # per region: the max over ranks
        region_dt = [float(x) for x in t.tolist()]
    slow = max(range(len(region_dt)), key=lambda i: region_dt[i])
    dt, dt_own = region_dt[slow], regions[slow][1]
    rank_seconds = [dt_own]
    if use_dist:
        own = torch.tensor([dt_own], device=cdev, dtype=torch.float64)
        parts = [torch.empty_like(own) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, own)
        rank_seconds = [float(x.item()) for x in parts]
    flops_exec = eng.last_flops()
    log(f"timed region: {total_steps} images in {dt:.3f} s")
    ms_per_step = dt / (total_steps / world) * 1e3       # per rank: every rank runs total/world images concurrently

    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, {"top5": top5, "final_logits": final_logits})

    dist_sustained = None
    if use_dist and a.full and a.sustain_seconds > 0:
        # ---- sustained leg of a multi-rank run: EVERY rank repeats full passes for >= sustain_seconds at the same time (barrier in
        # front, none inside), one HIP event pair per pass; the per-rank rates are gathered (the aggregate is their sum: no rank waits
        # for another on the data path)
        pv = views[:pass_images]
        dist.barrier()
        evs, t_end = [], time.perf_counter() + a.sustain_seconds
        while time.perf_counter() < t_end or len(evs) < 5:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run_pass(pv)
            e1.record()
            evs.append((e0, e1))
            if len(evs) % 4 == 0:
                torch.cuda.synchronize()
        torch.cuda.synchronize()
        per_img = [e0.elapsed_time(e1) / pass_images for e0, e1 in evs]
        mine = torch.tensor([statistics.fmean(per_img), float(len(per_img))], device=cdev, dtype=torch.float64)
        parts = [torch.empty_like(mine) for _ in range(dist.get_world_size())]
        dist.all_gather(parts, mine)
        ms = [float(x[0].item()) for x in parts]
        dist_sustained = {"seconds_per_rank_at_least": a.sustain_seconds, "passes_per_rank": [int(x[1].item()) for x in parts],
                          "images_per_pass": pass_images, "mean_ms_per_image_per_rank": ms,
                          "images_per_s_per_rank": [1e3 / m for m in ms], "images_per_s_aggregate": sum(1e3 / m for m in ms),
                          "slowest_over_fastest_rank": max(ms) / min(ms),
                          "timer": "HIP events on each rank's launch stream, one pair per pass, all ranks running concurrently"}
    if rank == 0:
        lib = _lib.lib()
        if dist_info:
            dist_info["timed_region_seconds_per_rank"] = rank_seconds
            dist_info["timed_region_slowest_over_fastest_rank"] = max(rank_seconds) / max(min(rank_seconds), 1e-12)
            dist_info["settle_passes_before_timed_region"] = settle
            if dist_sustained:
                dist_info["sustained"] = dist_sustained
        peak = PEAK_TFLOPS["f32"] if a.precision == "f32" else PEAK_TFLOPS["f16"]
        passes = MFMA_PASSES[a.precision] if not (a.precision == "f16x3" and a.weights == "fp16grid") else 2
        tuned = "LayerNorm parameters of the image encoder" if mode_ln else "prompt"
        out = {
            "metric": "test_images_per_sec", "value": total_steps / dt, "unit": "images/s", "n_gpus": world,
            "steps": a.steps if scaling == "weak" else total_steps, "warmup": a.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": scaling, "vs_baseline": None, "dtype": DTYPE[a.precision], "data": "synthetic" if a.weights == "fp32" else "synthetic; GEMM weights on the fp16 grid as in the released CLIP checkpoints (two exact MFMA passes per product)",
            "config": {"workload": f"RLCF test-time-adaptation step ({tuned} tuned), CLIP {student_arch} student + {a.reward_arch} reward, "
                                   f"N={a.views} views, {a.classes}-class bank, selection_p={wl['selection_p']}, K=3, {a.tta_steps} AdamW step(s)"
                                   + (f" ({wl['what'].split(':')[0]})" if is_default_wl else ""),
                       "baseline_config": a.config if is_default_wl else None,
                       "views": a.views, "classes": a.classes, "text_mode": a.text_mode, "text_rows": eng.text_rows(),
                       "tta_steps": a.tta_steps, "images_per_pass": pass_images, "timed_images_per_rank": steps,
                       "parallelism": f"sample-sharded x{world}, no data-path collective"},
            "timed_regions_seconds": region_dt, "timed_region_reported": "the slowest of the regions above (each exactly `steps` images per rank)",
            "flops_exec_per_image": flops_exec,
            "whole_step_tflops": flops_exec * total_steps / dt / 1e12,
            "top1_first": int(top5[0, 0].item()),
        }
        if dist_info:
            out["distributed"] = dist_info
        if a.full and not a.no_roofline:
            # ---- roofline leg: one pass of exactly the timed pass size, HIP event pair per GEMM / attention / LayerNorm launch
            lib.rlcf_profile_gemm(1)
            run_pass(views[:pass_images])
            torch.cuda.synchronize()
            ent = profile_entries(lib)
            lib.rlcf_profile_gemm(0)
            log(f"roofline leg: {len(ent)} profiled launches")
            gemms = [e for e in ent if e[0] < 10]
            # dominant kernel = the GEMM kernel kind with the most time in the pass (configs[1]: the 256x256 split-f16 kernel)
            by_kind = {}
            for e in gemms:
                by_kind[e[0]] = by_kind.get(e[0], 0.0) + e[1]
            dom_kind = max(by_kind, key=by_kind.get) if by_kind else 3
            dom = [e for e in gemms if e[0] == dom_kind]
            d_ms, d_fl = sum(e[1] for e in dom), sum(e[2] for e in dom)
            g_ms, g_fl = sum(e[1] for e in gemms), sum(e[2] for e in gemms)
            achieved = d_fl / (d_ms * 1e-3) / 1e12 if d_ms > 0 else 0.0
            table = []
            if not geo.is_resnet:
                # named rows: the student image tower's layer kernels (K4 in_proj, K5 attention, K6 out_proj,
                # K7 c_fc / c_proj, K3 LayerNorm) at the token-matrix size of this pass
                Wv, tok = geo.vision_width, geo.vision_tokens
                M_student = pass_images * a.views * tok
                names = {(3 * Wv, Wv): "K4 in_proj (QKV)", (Wv, Wv): "K6 out_proj + residual", (4 * Wv, Wv): "K7 c_fc + QuickGELU",
                         (Wv, 4 * Wv): "K7 c_proj + residual"}
                for (n_, k_), nm in names.items():
                    sel = [e for e in gemms if e[3] == (M_student, n_, k_)]
                    if sel:
                        ms_, fl_ = sum(e[1] for e in sel), sum(e[2] for e in sel)
                        table.append({"kernel": nm, "M": M_student, "N": n_, "K": k_, "launches": len(sel), "avg_ms": ms_ / len(sel),
                                      "tflops": fl_ / ms_ / 1e9, "frac_of_peak": fl_ / ms_ / 1e9 / peak})
                ln = [e for e in ent if e[0] == 11 and e[3][0] == M_student]
                if ln:      # HBM GB/s for the bandwidth-bound kernels — K3 LayerNorm, algorithmic bytes = f32 row in + pair row out
                    ms_, by_ = sum(e[1] for e in ln), sum(e[2] for e in ln)
                    table.append({"kernel": "K3 LayerNorm forward -> operand pairs (HBM-bound)", "rows": M_student, "launches": len(ln),
                                  "avg_ms": ms_ / len(ln), "gb_per_s": by_ / ms_ / 1e6, "frac_of_hbm_peak": by_ / ms_ / 1e6 / HBM_PEAK_GBS})
                att = [e for e in ent if e[0] == 10 and e[3][0] == M_student]
                if att:
                    ms_, fl_ = sum(e[1] for e in att), sum(e[2] for e in att)
                    # HBM roofline of this kernel: Q, K, V operand pairs in + O pairs out = 16 B per token and column
                    hbm_ms = M_student * Wv * 16.0 / (HBM_PEAK_GBS * 1e6)
                    table.append({"kernel": "K5 attention forward (QK^T, softmax, PV)", "rows": M_student, "launches": len(att),
                                  "avg_ms": ms_ / len(att), "tflops": fl_ / ms_ / 1e9, "frac_of_peak": fl_ / ms_ / 1e9 / peak,
                                  "hbm_roofline_ms": hbm_ms, "frac_of_hbm_roofline": hbm_ms / (ms_ / len(att))})
            # every profiled launch of the pass, grouped by kernel kind and shape, longest first (forward AND backward kernels: the
            # dX / weight-gradient GEMMs, the attention backward and the LayerNorm backward of the encoder-tuning configs)
            groups = {}
            for e in ent:
                g = groups.setdefault((e[0], e[3]), [0, 0.0, 0.0])
                g[0] += 1; g[1] += e[1]; g[2] += e[2]
            all_ms = sum(g[1] for g in groups.values())
            by_shape = []
            for (kind, dims), (n_l, ms_, w_) in sorted(groups.items(), key=lambda kv: -kv[1][1])[:24]:
                row = {"kernel": KIND_NAMES.get(kind, f"kind {kind}"), "dims": list(dims), "launches": n_l, "total_ms_per_image": ms_ / pass_images,
                       "share_of_profiled_time": ms_ / all_ms if all_ms > 0 else 0.0}
                if kind in HBM_KINDS:
                    row.update(gb_per_s=w_ / ms_ / 1e6, frac_of_hbm_peak=w_ / ms_ / 1e6 / HBM_PEAK_GBS)
                else:
                    row.update(tflops=w_ / ms_ / 1e9, frac_of_peak=w_ / ms_ / 1e9 / peak)
                by_shape.append(row)
            # HBM/fabric bytes per launch of the dominant kernel come from a separate rocprofv3 --pmc pass (counters perturb timing
            # and cannot be read in-process); they are quoted only from a committed profile of this exact pass size
            traffic, tsrc = None, None
            tname = next((n for n in ("r6_gemm_hbm_traffic.json", "r5_gemm_hbm_traffic.json", "r4_gemm_hbm_traffic.json") if os.path.exists(os.path.join(ROOT, "profiles", n))), None)
            if a.precision == "f16x3" and tname and a.config == 1 and is_default_wl:
                rec = json.load(open(os.path.join(ROOT, "profiles", tname))).get("bytes_per_launch_by_images_per_pass", {}).get(str(pass_images))
                if rec:
                    traffic, tsrc = rec, (f"profiles/{tname} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this GEMM at {pass_images} images per "
                                          f"pass on the round-{tname[1]} build; Infinity-Cache hits are inside the counter)")
            # MFMA-pipe utilisation by COUNTER (SQ_VALU_MFMA_BUSY_CYCLES / (4 x SQ_BUSY_CU_CYCLES)) of the dominant kernel on this round's build:
            # like `traffic`, read from the committed rocprofv3 --pmc profile of the same GEMM shapes (counters cannot be read in-process)
            busy, bsrc = None, None
            cname = next((n for n in ("r6_sq_counters.json", "r5_sq_counters.json") if os.path.exists(os.path.join(ROOT, "profiles", n))), None)
            cpath = os.path.join(ROOT, "profiles", cname or "none")
            if a.precision == "f16x3" and cname and a.config == 1 and is_default_wl:
                busy = json.load(open(cpath)).get("summary", {}).get("dominant_gemm_parity_mode_mfma_busy")
                bsrc = (f"profiles/{cname[:-5]}.txt: rocprofv3 --pmc SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CU_CYCLES SQ_INSTS_MFMA over the four layer products "
                        "at 20 images per pass (tools/r5_sq_counters.sh), cycles summed over the launches; at the clock the part sustains under the counters")
            out["roofline"] = {
                "bound": "mfma", "achieved": achieved, "peak": peak, "unit": "TFLOP/s", "frac": achieved / peak,
                "traffic": traffic, "traffic_source": tsrc, "mfma_passes": passes,
                "mfma_busy_counter": busy, "mfma_busy_counter_source": bsrc,
                "frac_of_mfma_pipe": passes * achieved / peak,     # issued MFMA flops / peak (computed: passes x achieved, not a counter)
                "kernel": KIND_NAMES.get(dom_kind, str(dom_kind)) + (" (3x v_mfma_f32_32x32x16_f16 per f32-grade product)" if a.precision == "f16x3" else ""),
                "profiled_images_per_pass": pass_images, "launches": len(dom), "avg_launch_ms": d_ms / max(len(dom), 1),
                "launches_per_image": len(dom) / pass_images, "gemm_flops_per_image": d_fl / pass_images,
                "all_gemm_kernels": {"launches_per_image": len(gemms) / pass_images, "ms_per_image": g_ms / pass_images,
                                     "achieved": g_fl / (g_ms * 1e-3) / 1e12 if g_ms > 0 else 0.0},
                "per_kernel": table, "per_kernel_all_launches": by_shape,
                # the profiled pass is the timed pass: its GEMM time cannot exceed the step time (5 % for event overhead / clock drift)
                "check_gemm_time_within_step": bool(g_ms / pass_images <= 1.05 * ms_per_step),
            }
        if a.full and world == 1 and a.sustain_seconds > 0 and not use_dist:
            # ---- sustained leg: full passes for >= sustain_seconds, a HIP event pair per pass (p50 / mean)
            pv = views[:pass_images]
            # shader clock / socket power while the passes run (rocm-smi at ~3 Hz from a host thread): under this load the package sits
            # on its power limit and the clock settles well below the 2.4 GHz the dense peaks are quoted at (profiles/r3_gemm_experiments.txt)
            smp, smp_stop = [], threading.Event()

            def _poll():
                import re
                import subprocess
                while not smp_stop.is_set():
                    try:
                        o = subprocess.run(["rocm-smi", "--showclocks", "--showpower", "--json"], capture_output=True, text=True, timeout=5).stdout
                        card = next(iter(json.loads(o).values()))
                        sclk = next((float(re.sub(r"[^0-9.]", "", v)) for k, v in card.items() if "sclk clock speed" in k.lower()), None)
                        pw = next((float(v) for k, v in card.items() if "power (w)" in k.lower()), None)
                        if sclk:
                            smp.append((sclk, pw))
                    except Exception:
                        pass
                    smp_stop.wait(0.3)
            th = threading.Thread(target=_poll, daemon=True)
            th.start()
            evs, t_end = [], time.perf_counter() + a.sustain_seconds
            while time.perf_counter() < t_end or len(evs) < 8:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run_pass(pv)
                e1.record()
                evs.append((e0, e1))
                if len(evs) % 4 == 0:
                    torch.cuda.synchronize()             # keeps the host at most 4 passes ahead (the loop is time-bounded)
            torch.cuda.synchronize()
            smp_stop.set()
            th.join(timeout=6)
            per_img = sorted(e0.elapsed_time(e1) / pass_images for e0, e1 in evs)
            log(f"sustained leg: {len(per_img)} passes")
            out["sustained"] = {"passes": len(per_img), "images_per_pass": pass_images, "mean_ms_per_image": statistics.fmean(per_img),
                                "p50_ms_per_image": statistics.median(per_img), "min_ms_per_image": per_img[0],
                                "max_ms_per_image": per_img[-1], "images_per_s_mean": 1e3 / statistics.fmean(per_img),
                                "timer": "HIP events on the launch stream, one pair per pass"}
            body = smp[len(smp) // 3:] if len(smp) >= 3 else smp          # (skip the ramp at the start of the leg)
            if body:
                sclk = statistics.median(x[0] for x in body)
                pws = [x[1] for x in body if x[1] is not None]
                out["sustained"]["clocks"] = {"sclk_mhz_median": sclk, "socket_power_w_median": statistics.median(pws) if pws else None,
                                              "samples": len(body), "nominal_sclk_mhz": 2400.0,
                                              "source": "rocm-smi --showclocks --showpower, sampled by a host thread during this leg"}
                if "roofline" in out and out["roofline"].get("bound") == "mfma":
                    # the same achieved rate against the matrix-pipe peak AT THE CLOCK THE PART SUSTAINS under this load (dense peak x sclk / 2.4 GHz)
                    out["roofline"]["peak_at_sustained_clock"] = out["roofline"]["peak"] * sclk / 2400.0
                    out["roofline"]["frac_at_sustained_clock"] = out["roofline"]["achieved"] / out["roofline"]["peak_at_sustained_clock"]
                    out["roofline"]["frac_of_mfma_pipe_at_sustained_clock"] = out["roofline"]["frac_of_mfma_pipe"] * 2400.0 / sclk
        if a.full and world == 1 and a.precision == "f16x3" and a.config == 1 and not a.no_f16_line and not use_dist:
            # ---- secondary, clearly labelled: the reference's own GPU arithmetic (fp16 autocast, tpt_cls_rl.py:52) = RLCF_PREC_F16.
            # Not the headline and not parity-grade: reported with its measured deviation from the split-f16 engine on this very pass.
            # Two forms: the DEFAULT (f32 residual stream: keeps the reference's top-1 on 32 / 32 stream samples) and the opt-in with the
            # LayerNorms folded into the products on an f16 residual stream (rlcf_engine_set_f16_lnfold: 31 / 32).
            top5x, flx = eng.tta_batch(views[:pass_images], cfg, want_logits=True)
            eh = Engine(geo, rgeo, a.views * batch, a.classes, _lib.PREC_F16)
            eh.load_state_dict(_lib.STUDENT, ssd)
            eh.load_state_dict(_lib.REWARD, rsd)
            eh.finalize()
            eh.set_class_bank(tokens, n_ctx, ctx0, mode)
            Wv, tok = geo.vision_width, geo.vision_tokens
            M_st = pass_images * a.views * tok

            def f16_form(fold):
                eh.set_f16_lnfold(fold)
                top5h, flh = eh.tta_batch(views[:pass_images], cfg, want_logits=True)         # also sizes the workspaces
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                reps = 4
                e0.record()
                for _ in range(reps):
                    eh.tta_batch(views[:pass_images], cfg)
                e1.record()
                torch.cuda.synchronize()
                ms_h = e0.elapsed_time(e1) / (reps * pass_images)
                lib.rlcf_profile_gemm(1)
                eh.tta_batch(views[:pass_images], cfg)
                torch.cuda.synchronize()
                ent_h = profile_entries(lib)
                lib.rlcf_profile_gemm(0)

                def frac(n_, k_):
                    sel = [e for e in ent_h if e[0] < 10 and e[3] == (M_st, n_, k_)]
                    return (sum(e[2] for e in sel) / max(sum(e[1] for e in sel), 1e-9) / 1e9 / PEAK_TFLOPS["f16"]) if sel else None
                dom_h = [e for e in ent_h if e[0] == 3]
                ach_h = sum(e[2] for e in dom_h) / max(sum(e[1] for e in dom_h), 1e-9) / 1e9
                att_h = [e for e in ent_h if e[0] == 10 and e[3][0] == M_st]
                att_ms = (sum(e[1] for e in att_h) / len(att_h)) if att_h else None
                hbm_ms = M_st * Wv * 8.0 / (HBM_PEAK_GBS * 1e6)   # Q, K, V rows in + O rows out as plain f16: this kernel's own bound
                return {"residual_stream": "f16 rows, LayerNorms folded into the products (opt-in)" if fold else "f32 rows + layernorm_add_fwd (default)",
                        "images_per_s": 1e3 / ms_h, "ms_per_image": ms_h, "images_per_pass": pass_images,
                        "max_abs_dlogit_vs_split_f16": float((flx - flh).abs().max().item()),
                        "top1_agreement_vs_split_f16": float((top5x[:, 0] == top5h[:, 0]).float().mean().item()),
                        "dominant_gemm_tflops": ach_h, "dominant_gemm_frac_of_f16_peak": ach_h / PEAK_TFLOPS["f16"],
                        "in_proj_qkv_gemm_frac_of_f16_peak": frac(3 * Wv, Wv), "out_proj_gemm_frac_of_f16_peak": frac(Wv, Wv),
                        "c_fc_gemm_frac_of_f16_peak": frac(4 * Wv, Wv), "c_proj_gemm_frac_of_f16_peak": frac(Wv, 4 * Wv),
                        "attention_fwd_frac_of_f16_peak": (sum(e[2] for e in att_h) / max(sum(e[1] for e in att_h), 1e-9) / 1e9 / PEAK_TFLOPS["f16"]) if att_h else None,
                        "attention_fwd_hbm_roofline_ms": hbm_ms, "attention_fwd_avg_ms": att_ms,
                        "attention_fwd_frac_of_hbm_roofline": (hbm_ms / att_ms) if att_ms else None}
            f16_default, f16_fold = f16_form(False), f16_form(True)
            out["secondary_f16_single_pass"] = dict(
                f16_default,
                what="RLCF_PREC_F16: forward tower pipeline in plain f16, one MFMA per product (the reference's fp16-autocast arithmetic); "
                     "NOT parity-grade, not the headline.  Top level = the default form; `lnfold_opt_in` = the same pass with rlcf_engine_set_f16_lnfold(1)",
                lnfold_opt_in=f16_fold,
                kernels=("gemm_nt_f16_pp_kernel (persistent 256x256 eight-phase kernel, gemm_f16.hip; half of a tile's stores deferred under the next "
                         "tile's K loop: RLCF_F16_PP_DEFER) for the four block products; attention_fwd_pair_kernel SINGLE form"),
                notes="profiles/r6_notes.md")
            eh.close()
            log("secondary f16 line done")
        if a.full and world == 1 and a.precision == "f16x3" and a.config == 1 and not a.no_f16_line and not use_dist and a.weights == "fp32":
            # ---- secondary, parity-grade: the same step with the GEMM weights on the fp16 GRID, as every released CLIP checkpoint has them
            # (the archives the reference loads store Conv / Linear / attention / projection weights as fp16; TPT/clip/model.py:375-436
            # copies them into float32 parameters).  Their split-f16 lo halves are zero, the engine finds that out at finalize and the
            # 256x256 kernel drops the a_hi . w_lo pass: the SAME bits as three passes (tests/test_gpu_round5.py), two MFMAs per product.
            # `value` above stays on arbitrary float32 random weights (three passes): the conservative case.
            import ctypes
            eg = Engine(geo, rgeo, a.views * batch, a.classes, _lib.PREC_F16X3)
            eg.load_state_dict(_lib.STUDENT, synth.to_fp16_grid(ssd))
            eg.load_state_dict(_lib.REWARD, synth.to_fp16_grid(rsd))
            eg.finalize()
            off_g = ctypes.c_int(0)
            on_g = int(lib.rlcf_engine_f16_grid_weights(eg.h, _lib.STUDENT, ctypes.byref(off_g)))
            eg.set_class_bank(tokens, n_ctx, ctx0, mode)
            eg.tta_batch(views[:pass_images], cfg)
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = 5
            e0.record()
            for _ in range(reps):
                eg.tta_batch(views[:pass_images], cfg)
            e1.record()
            torch.cuda.synchronize()
            ms_g = e0.elapsed_time(e1) / (reps * pass_images)
            lib.rlcf_profile_gemm(1)
            eg.tta_batch(views[:pass_images], cfg)
            torch.cuda.synchronize()
            ent_g = profile_entries(lib)
            lib.rlcf_profile_gemm(0)
            dom_g = [e for e in ent_g if e[0] == 3]
            ach_g = sum(e[2] for e in dom_g) / max(sum(e[1] for e in dom_g), 1e-9) / 1e9
            out["secondary_checkpoint_grid_weights"] = {
                "what": "the same parity-grade step (RLCF_PREC_F16X3) with the GEMM weights rounded to fp16 values, as the released CLIP checkpoints "
                        "the reference loads store them: w_lo == 0, so the a_hi . w_lo MFMA pass is dropped — bit-identical to three passes on these "
                        "weights, two MFMAs per product; `value` is measured on arbitrary float32 weights",
                "images_per_s": 1e3 / ms_g, "ms_per_image": ms_g, "images_per_pass": pass_images,
                "student_gemm_weights_on_the_grid": on_g, "student_gemm_weights_off_the_grid": off_g.value,
                "dominant_gemm_tflops": ach_g, "dominant_gemm_frac": ach_g / PEAK_TFLOPS["f16"], "mfma_passes": 2,
                "dominant_gemm_frac_of_mfma_pipe": 2.0 * ach_g / PEAK_TFLOPS["f16"]}
            eg.close()
            log("secondary fp16-grid-weights line done")
        if a.full and world == 1 and a.config == 1 and is_default_wl and a.precision == "f16x3" and not a.no_harness_leg and not use_dist:
            eng.close()                                      # (the mirror builds its own engine: free this one's workspace first)
            eng = None
            out["harness"] = harness_leg(dev, student_arch, a.reward_arch, ssd, rsd, a.classes, a.views, wl["selection_p"], wl["lr"])
            if a.weights == "fp32":
                # the same loop on checkpoint-grid weights (see secondary_checkpoint_grid_weights): one image per pass only
                hg = harness_leg(dev, student_arch, a.reward_arch, synth.to_fp16_grid(ssd), synth.to_fp16_grid(rsd), a.classes, a.views,
                                 wl["selection_p"], wl["lr"], one_only=True)
                hg["what"] = "the harness leg above with the GEMM weights on the fp16 grid (as a released checkpoint holds them): one image per pass"
                out["harness_checkpoint_grid_weights"] = hg
            log("harness leg done")
        if a.full and world == 1 and not a.no_cpu_baseline and not use_dist:
            # the reference's CPU path runs BASELINE configs[0] (ViT-B/16, N = 8): timed for configs 0 / 1; the ViT-L/14 and RN50x64
            # configurations would take minutes per image on the host and get the same oracle leg only when asked for with a budget
            if a.config in (0, 1):
                out["cpu_baseline"] = cpu_baseline({k: v.cpu() for k, v in ssd.items()}, {k: v.cpu() for k, v in rsd.items()}, geo, a.classes,
                                                   budget_s=a.cpu_baseline_budget)
            # (configs 2 / 4: no `cpu_baseline` key — the oracle's CPU leg is BASELINE configs[0]; a ViT-L/14 or RN50x64 sample takes the
            # host minutes, and a null would read as a measurement)
        if a.full:
            # ---- flat copies of the numbers a review leans on, next to `value` (the driver's parsed record keeps top-level scalars)
            def _g(d, *ks):
                for k in ks:
                    d = d.get(k) if isinstance(d, dict) else None
                    if d is None:
                        return None
                return d
            out["value_sustained"] = _g(out, "sustained", "images_per_s_mean")
            out["roofline_frac"] = _g(out, "roofline", "frac")
            for row in _g(out, "roofline", "per_kernel") or []:
                if row["kernel"].startswith("K5"):
                    out["attention_fwd_frac_of_hbm_roofline"] = row.get("frac_of_hbm_roofline")
            for k_flat, ks in (("f16_images_per_s", ("secondary_f16_single_pass", "images_per_s")),
                               ("f16_in_proj_frac", ("secondary_f16_single_pass", "in_proj_qkv_gemm_frac_of_f16_peak")),
                               ("f16_c_fc_frac", ("secondary_f16_single_pass", "c_fc_gemm_frac_of_f16_peak")),
                               ("f16_c_proj_frac", ("secondary_f16_single_pass", "c_proj_gemm_frac_of_f16_peak")),
                               ("f16_out_proj_frac", ("secondary_f16_single_pass", "out_proj_gemm_frac_of_f16_peak")),
                               ("f16_attention_frac", ("secondary_f16_single_pass", "attention_fwd_frac_of_f16_peak")),
                               ("f16_attention_frac_of_hbm_roofline", ("secondary_f16_single_pass", "attention_fwd_frac_of_hbm_roofline")),
                               ("f16_top1_agreement", ("secondary_f16_single_pass", "top1_agreement_vs_split_f16")),
                               ("f16_lnfold_images_per_s", ("secondary_f16_single_pass", "lnfold_opt_in", "images_per_s")),
                               ("f16_lnfold_in_proj_frac", ("secondary_f16_single_pass", "lnfold_opt_in", "in_proj_qkv_gemm_frac_of_f16_peak")),
                               ("f16_lnfold_c_fc_frac", ("secondary_f16_single_pass", "lnfold_opt_in", "c_fc_gemm_frac_of_f16_peak")),
                               ("grid_weights_images_per_s", ("secondary_checkpoint_grid_weights", "images_per_s")),
                               ("harness_one_image_per_call", ("harness", "images_per_s_one_image_per_pass_staged_views")),
                               ("harness_one_image_per_call_views_in_loop", ("harness", "images_per_s_one_image_per_pass_views_in_loop")),
                               ("harness_three_in_flight", ("harness", "images_per_s_one_image_per_pass_three_in_flight_staged_views")),
                               ("harness_three_in_flight_views_in_loop", ("harness", "images_per_s_one_image_per_pass_three_in_flight_views_in_loop")),
                               ("harness_three_in_flight_legs_spread", ("harness", "three_in_flight_staged_legs_max_over_min")),
                               ("harness_three_in_flight_views_in_loop_legs_spread", ("harness", "three_in_flight_views_in_loop_legs_max_over_min")),
                               ("view_generation_ms_per_image", ("harness", "view_generation_ms_per_image")),
                               ("cpu_baseline_images_per_s", ("cpu_baseline", "value"))):
                out[k_flat] = _g(out, *ks)
        print(json.dumps(out))
    if eng is not None:
        eng.close()
    if use_dist:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
