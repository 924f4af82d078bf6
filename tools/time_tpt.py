"""Per-image time of the TPT baseline (RLCF_F_TPT: avg_entropy of the selected views, no reward model run) next to the RL step of the
same build, on synthetic weights: ViT-B/16 student, ViT-L/14 reward, N = 64 views (selection_p 0.1: 6 selected), 1000 classes.
  prompt   rlcf_tta_sample, 1 step, lr 7e-3 (the BASELINE configs[1] geometry; scripts/rlcf-prompt.sh against tpt_cls.py with one step)
  ln       rlcf_tta_sample_ln, 3 steps, lr 1e-3 (LayerNorm tuning)
  visual   rlcf_tta_sample_visual, 3 steps, lr 1e-5 (every visual parameter: scripts/rlcf-tune.sh against scripts/tpt-tune.sh)
One engine call per test image; wall time per call over --iters calls after --warmup, HIP events on the stream.

    python tools/time_tpt.py [--iters 10] [--warmup 3] [--prec 2] [--settings prompt,ln,visual]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlcf_amd import _lib as L, synth  # noqa: E402
from rlcf_amd.engine import Engine, TTAConfig  # noqa: E402

SETTINGS = {"prompt": ("tta_sample", 1, 7e-3), "ln": ("tta_sample_ln", 3, 1e-3), "visual": ("tta_sample_visual", 3, 1e-5)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prec", type=int, default=L.PREC_F16X3)
    ap.add_argument("--settings", default="prompt,ln,visual")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    sg, rg = synth.GEOMETRIES["ViT-B/16"], synth.GEOMETRIES["ViT-L/14"]
    n_views, n_cls = 64, 1000
    eng = Engine(sg, rg, n_views, n_cls, a.prec)
    eng.load_state_dict(L.STUDENT, synth.make_state_dict(sg, 11, device=dev))
    eng.load_state_dict(L.REWARD, synth.make_state_dict(rg, 23, device=dev))
    eng.finalize()
    ssd_tok = synth.make_state_dict(sg, 11, device=dev)["token_embedding.weight"]
    ctx0 = ssd_tok[torch.tensor(synth.ctx_token_ids_default(sg, 4), device=dev)].clone()
    eng.set_class_bank(synth.make_token_bank(sg, n_cls, seed=7, n_ctx=4), 4, ctx0, L.TEXT_SHARED)
    views = [synth.make_views(1000 + i, n_views, sg.image_resolution, device=dev) for i in range(4)]
    res = {}
    for name in a.settings.split(","):
        fn, steps, lr = SETTINGS[name]
        call = getattr(eng, fn)
        for tpt in (False, True):
            cfg = TTAConfig(selection_p=0.1, tta_steps=steps, sample_k=3, lr=lr, weight_decay=5e-4, tpt=tpt)
            for i in range(a.warmup):
                call(views[i % len(views)], cfg)
            torch.cuda.synchronize()
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for i in range(a.iters):
                call(views[i % len(views)], cfg)
            t1.record()
            torch.cuda.synchronize()
            ms = t0.elapsed_time(t1) / a.iters
            res[f"{name}_{'tpt' if tpt else 'rl'}"] = round(ms, 2)
            print(f"{name:8s} {steps} step(s)  {'TPT (RLCF_F_TPT)' if tpt else 'RL (reward loss)'} {ms:8.2f} ms / image", flush=True)
    eng.close()
    print(json.dumps({"config": "B/16 student + L/14 reward, N 64, 1000 classes", "precision": a.prec, "ms_per_image": res}))


if __name__ == "__main__":
    main()
