"""Images per second of the zero-shot batch call (rlcf_zero_shot_batch: towers, one ensemble-logits launch, top-5, hit counts) on synthetic
weights: batches of 64 different images at 224 x 224, 1000 classes.
  b16            ViT-B/16 alone (CLIPCLS_TTA, the "CLIP zero-shot" row)
  b16_l14        ViT-B/16 + ViT-L/14, the default list of CLIPCLS_TTA_Multiple (the "zero-shot ensemble" row)
  mirror_b16     the same ViT-B/16 batch through what the package offered before this entry: CLIPCLS_TTA.forward + accuracy per batch
  tail_*         the part after the towers alone, per batch: rlcf_ensemble_logits on M = 1 / 2 models, and top-5 + hit counting
                 (rlcf_accuracy: the same top-5 kernel and a one-block counting kernel)
One call per batch; time per call over --iters calls after --warmup, HIP events on the stream.

    python tools/time_zero_shot.py [--iters 20] [--warmup 3] [--prec 2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlcf_amd import _lib as L, synth  # noqa: E402
from rlcf_amd.engine import Engine, ensemble_logits  # noqa: E402

BATCH, N_CLS, RES = 64, 1000, 224


def timed(fn, warmup, iters):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for i in range(iters):
        fn(i)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / iters


def build(archs, prec, dev):
    geos = [synth.GEOMETRIES[a] for a in archs]
    eng = Engine(geos[0], geos[1:] or None, BATCH, N_CLS, prec)
    for w, (g, seed) in enumerate(zip(geos, (11, 23))):
        eng.load_state_dict(w, synth.make_state_dict(g, seed, device=dev))
    eng.finalize()
    tokens = synth.make_token_bank(geos[0], N_CLS, seed=7, n_ctx=4)
    sd0 = synth.make_state_dict(geos[0], 11, device=dev)
    ctx = sd0["token_embedding.weight"][tokens[0][1:2].to(dev)].clone()       # as the mirrors publish the bank: the first prompt token's embedding
    eng.set_class_bank(tokens, 1, ctx, L.TEXT_SHARED)
    return eng, ctx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prec", type=int, default=L.PREC_F16X3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    images = [synth.make_views(3000 + i, BATCH, RES, device=dev) for i in range(2)]
    target = torch.arange(BATCH, device=dev, dtype=torch.int64)
    hits = torch.zeros(2, device=dev)
    res = {}
    for name, archs in (("b16", ("ViT-B/16",)), ("b16_l14", ("ViT-B/16", "ViT-L/14"))):
        eng, ctx = build(archs, a.prec, dev)
        ens = len(archs) > 1
        res[name] = timed(lambda i: eng.zero_shot_batch(images[i % 2], ensemble=ens, target=target, hits=hits, want_logits=False, want_top5=False),
                          a.warmup, a.iters)
        if ens:      # the tail alone, on this engine's features
            feats = [eng.encode_image(w, images[0]) for w in range(2)]
            cls = [eng.text_features(ctx), eng.reward_class_features(0)]
            scales = eng.logit_scales()
            out = torch.empty(BATCH, N_CLS, device=dev)
            t5, acc = torch.empty(BATCH, 5, dtype=torch.int32, device=dev), torch.empty(2, device=dev)
            st = torch.cuda.current_stream().cuda_stream
            res["tail_logits_m1"] = timed(lambda i: ensemble_logits(feats[:1], cls[:1], scales[:1], out=out), 10, 200)
            res["tail_logits_m2"] = timed(lambda i: ensemble_logits(feats, cls, scales, out=out), 10, 200)
            res["tail_top5_hits"] = timed(lambda i: eng.lib.rlcf_accuracy(out.data_ptr(), target.data_ptr(), BATCH, N_CLS, t5.data_ptr(), acc.data_ptr(), st), 10, 200)
        eng.close()
    # what the package offered before: the mirror's CLIPCLS_TTA.forward (tower, text features, logits GEMM) + accuracy, per batch
    from rlcf_amd import clip_store, custom_clip, runtime
    from rlcf_amd.tpt_cls_rl import accuracy
    runtime.reset_session()
    runtime.SESSION.max_views, runtime.SESSION.precision = BATCH, a.prec
    sg = synth.GEOMETRIES["ViT-B/16"]
    clip_store.register_checkpoint("ViT-B/16", sg, synth.make_state_dict(sg, 11))
    bank = clip_store.SyntheticBank(sg, N_CLS, 4, 7)
    clip_store.set_tokenizer(bank.tokenize)
    model = custom_clip.CLIPCLS_TTA("cpu", bank.classnames, arch="ViT-B/16", prompt_prefix="a_photo_of_a").eval()
    sums = torch.zeros(2, device=dev)

    def mirror(i):
        out = model(images[i % 2])
        acc1, acc5 = accuracy(out, target, topk=(1, 5))
        sums.add_(torch.cat([acc1, acc5]) * BATCH)

    res["mirror_b16"] = timed(mirror, a.warmup, a.iters)
    runtime.reset_session()
    for k, v in res.items():
        print(f"{k:16s} {v:9.3f} ms / batch" + (f"  {BATCH * 1000.0 / v:9.1f} images / s" if not k.startswith("tail") else f"  {1000.0 * v / BATCH:9.3f} us / image"), flush=True)
    print(json.dumps({"config": f"batch {BATCH}, {N_CLS} classes, {RES} x {RES}", "precision": a.prec, "ms_per_batch": {k: round(v, 3) for k, v in res.items()},
                      "images_per_s": {k: round(BATCH * 1000.0 / v, 1) for k, v in res.items() if not k.startswith("tail")}}))


if __name__ == "__main__":
    main()
