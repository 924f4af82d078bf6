"""Per-image time of the two every-parameter tuning configurations of the paper's "CLIP reward vs. distillation" comparison:
scripts/rlcf-tune.sh (reward loss) and scripts/kd-tune.sh (--kd_loss KD / DKD / ATKD): ViT-B/16 student, ViT-L/14 reward, N = 64
views (selection_p 0.1: 6 selected), 3 steps, lr 1e-5, every visual parameter tuned, 1000 classes.  One rlcf_tta_sample_visual
call per test image on synthetic weights; wall time per call over --iters calls after --warmup, HIP events on the stream.

    python tools/time_kd_tune.py [--iters 10] [--warmup 3] [--prec 2] [--losses RL,KD,DKD,ATKD]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlcf_amd import _lib as L, synth  # noqa: E402
from rlcf_amd.engine import Engine, TTAConfig  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--prec", type=int, default=L.PREC_F16X3)
    ap.add_argument("--losses", default="RL,KD,DKD,ATKD")
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
    for kind in a.losses.split(","):
        cfg = TTAConfig(selection_p=0.1, tta_steps=3, sample_k=3, lr=1e-5, weight_decay=5e-4, kd_loss=None if kind == "RL" else kind)
        for i in range(a.warmup):
            eng.tta_sample_visual(views[i % len(views)], cfg)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for i in range(a.iters):
            eng.tta_sample_visual(views[i % len(views)], cfg)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / a.iters
        res[kind] = round(ms, 2)
        print(f"{'rlcf-tune.sh' if kind == 'RL' else 'kd-tune.sh --kd_loss ' + kind:28s} {ms:8.2f} ms / image", flush=True)
    eng.close()
    print(json.dumps({"config": "B/16 student + L/14 reward, N 64, 3 steps, every visual parameter, 1000 classes",
                      "precision": a.prec, "ms_per_image": res}))


if __name__ == "__main__":
    main()
