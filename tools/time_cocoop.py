"""Per-image time of the CoCoOp path (rlcf_tta_sample_cocoop: generator pass, prompt step from the generated prompt, final logits) next
to the plain TPT prompt step of the same build (rlcf_tta_sample with RLCF_F_TPT), on synthetic weights: ViT-B/16 student, no reward
model, N = 64 views (selection_p 0.1: 6 selected), 1000 classes, n_ctx 4, meta-net 512 -> 32 -> 512.
  cocoop_s0 / cocoop_s1   rlcf_tta_sample_cocoop at 0 and 1 steps (all the reference has: TPT/tpt_cls.py:60)
  tpt_s0 / tpt_s1         rlcf_tta_sample under RLCF_F_TPT at 0 and 1 steps, lr 5e-3
  meta_net                rlcf_cocoop_ctx alone on one feature row (a launch-latency figure)
One engine call per test image; time per call over --iters calls after --warmup, HIP events on the stream.

    python tools/time_cocoop.py [--iters 10] [--warmup 3] [--prec 2]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlcf_amd import _lib as L, synth  # noqa: E402
from rlcf_amd.engine import Engine, TTAConfig, cocoop_ctx_op  # noqa: E402


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prec", type=int, default=L.PREC_F16X3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sg = synth.GEOMETRIES["ViT-B/16"]
    n_views, n_cls, n_ctx = 64, 1000, 4
    eng = Engine(sg, None, n_views, n_cls, a.prec)
    eng.load_state_dict(L.STUDENT, synth.make_state_dict(sg, 11, device=dev))
    eng.finalize()
    state = {k: v.to(dev) for k, v in synth.make_cocoop_state(sg, 31, n_ctx).items()}
    net = [state["meta_net." + k] for k in ("linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias")]
    eng.set_class_bank(synth.make_token_bank(sg, n_cls, seed=7, n_ctx=n_ctx), n_ctx, state["ctx"], L.TEXT_SHARED)
    eng.set_meta_net(*net)
    views = [synth.make_views(1000 + i, n_views, sg.image_resolution, device=dev) for i in range(4)]
    res = {}
    for steps in (0, 1):
        cfg = TTAConfig(selection_p=0.1, tta_steps=steps, lr=5e-3, weight_decay=0.01, tpt=True)
        res[f"cocoop_s{steps}"] = timed(lambda i: eng.tta_sample_cocoop(views[i % 4], cfg, want_intermediates=False), a.warmup, a.iters)
        res[f"tpt_s{steps}"] = timed(lambda i: eng.tta_sample(views[i % 4], cfg, want_intermediates=False), a.warmup, a.iters)
    feats = eng.cocoop_gen_ctx(views[0], aug=True)[0]
    res["meta_net"] = timed(lambda i: cocoop_ctx_op(feats[:1], state["ctx"], *net), 10, 200)
    eng.close()
    for k, v in res.items():
        print(f"{k:10s} {v:9.3f} ms / call", flush=True)
    print(json.dumps({"config": "B/16 student, no reward model, N 64, 1000 classes, n_ctx 4", "precision": a.prec,
                      "ms_per_call": {k: round(v, 3) for k, v in res.items()}}))


if __name__ == "__main__":
    main()
