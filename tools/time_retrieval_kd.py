"""Per-query time of retrieval test-time tuning, distillation (retrieval/clip_ret_kd.py) next to the policy (clip_ret_policy.py), at
the scripts' setting (retrieval/scripts/tta_coco_ret*.sh): ViT-B/16 student, ViT-L/14 reward, 3 steps, lr 1e-6, a bank of 25 010
captions (image -> text, K = 20 for the policy) / 5 000 images (text -> image, K = 12).  Synthetic weights; the image bank is seeded
unit vectors, the caption bank a seeded token bank.  Each query is timed on its own with HIP events on the stream; the median of
--iters queries after --warmup is reported.  First the loss op alone, split-row against one workgroup per row, at n = 1: these are CALL times (stream-ordered allocation and the
wrapper's output tensors included), which dominate at small C — kernel times come from a kernel trace of `--ops-only --ops-c C`.

    python tools/time_retrieval_kd.py [--iters 7] [--warmup 2] [--prec 2] [--captions 25010] [--images 5000] [--skip-i2t] [--ops-only]
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rlcf_amd import _lib as L, synth  # noqa: E402
from rlcf_amd.engine import Engine, TTAConfig, kd_loss_op, kd_loss_split_op  # noqa: E402


def timed(fn, iters, warmup):
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for i in range(iters):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn(i)
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), min(ms), max(ms)


def ops(dev, iters, res, only_c=0):
    for Cn in ((only_c,) if only_c else (1000, 5000, 25010, 65536)):
        g = torch.Generator().manual_seed(Cn)
        s = (100.0 * (0.2 + 0.05 * torch.randn(1, Cn, generator=g))).to(dev)
        t = (100.0 * (0.2 + 0.05 * torch.randn(1, Cn, generator=g))).to(dev)
        one = timed(lambda i: kd_loss_op(s, t, L.KD_KD), iters * 5, 5)
        split = timed(lambda i: kd_loss_split_op(s, t), iters * 5, 5)
        res[f"loss_op_C{Cn}"] = dict(one_workgroup_us=round(one[0] * 1e3, 1), split_us=round(split[0] * 1e3, 1))
        print(f"loss op n=1 C={Cn:6d}: one workgroup {one[0] * 1e3:8.1f} us   split {split[0] * 1e3:8.1f} us   (call medians, allocation included)", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--prec", type=int, default=L.PREC_F16X3)
    ap.add_argument("--captions", type=int, default=25010)
    ap.add_argument("--images", type=int, default=5000)
    ap.add_argument("--skip-i2t", action="store_true")
    ap.add_argument("--ops-only", action="store_true")
    ap.add_argument("--ops-c", type=int, default=0, help="loss op at this C alone (one kernel trace per C)")
    ap.add_argument("--calls", default="both", choices=["both", "kd", "policy"])
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    res = {}
    ops(dev, a.iters, res, a.ops_c)
    if a.ops_only:
        print(json.dumps(res))
        return
    sg, rg = synth.GEOMETRIES["ViT-B/16"], synth.GEOMETRIES["ViT-L/14"]
    eng = Engine(sg, rg, 8, max(a.captions, a.images), a.prec)
    eng.load_state_dict(L.STUDENT, synth.make_state_dict(sg, 11, device=dev))
    eng.load_state_dict(L.REWARD, synth.make_state_dict(rg, 23, device=dev))
    eng.finalize()
    hp = dict(selection_p=1.0, tta_steps=3, lr=1e-6, weight_decay=5e-4, eps=1e-6)
    # text -> image
    gen = torch.Generator().manual_seed(5)
    sbank = torch.nn.functional.normalize(torch.randn(a.images, sg.embed_dim, generator=gen), dim=-1).to(dev)
    rbank = torch.nn.functional.normalize(torch.randn(a.images, rg.embed_dim, generator=gen), dim=-1).to(dev)
    eng.set_image_bank(sbank, rbank)
    queries = synth.make_token_bank(sg, 16, seed=7, n_ctx=4)
    none = (float("nan"),) * 3
    kd = timed(lambda i: eng.tta_retrieval_text_kd(queries[i % 16], TTAConfig(sample_k=1, **hp)), a.iters, a.warmup) if a.calls != "policy" else none
    rl = timed(lambda i: eng.tta_retrieval_text(queries[i % 16], TTAConfig(sample_k=12, **hp)), a.iters, a.warmup) if a.calls != "kd" else none
    res["t2i_ms_per_query"] = dict(kd=round(kd[0], 2), kd_min_max=[round(kd[1], 2), round(kd[2], 2)], policy=round(rl[0], 2),
                                   policy_min_max=[round(rl[1], 2), round(rl[2], 2)], bank=a.images)
    print(f"text -> image, {a.images} images: KD {kd[0]:.2f} ms / query [{kd[1]:.2f}, {kd[2]:.2f}]   policy {rl[0]:.2f} [{rl[1]:.2f}, {rl[2]:.2f}]", flush=True)
    if not a.skip_i2t:
        eng.set_class_bank(synth.make_token_bank(sg, a.captions, seed=7, n_ctx=4), 0, None, L.TEXT_SHARED)
        imgs = [synth.make_views(1000 + i, 1, sg.image_resolution, device=dev) for i in range(4)]
        kd = timed(lambda i: eng.tta_retrieval_image_kd(imgs[i % 4], TTAConfig(sample_k=1, **hp)), a.iters, a.warmup) if a.calls != "policy" else none
        rl = timed(lambda i: eng.tta_retrieval_image(imgs[i % 4], TTAConfig(sample_k=20, **hp)), a.iters, a.warmup) if a.calls != "kd" else none
        res["i2t_ms_per_query"] = dict(kd=round(kd[0], 2), kd_min_max=[round(kd[1], 2), round(kd[2], 2)], policy=round(rl[0], 2),
                                       policy_min_max=[round(rl[1], 2), round(rl[2], 2)], bank=a.captions)
        print(f"image -> text, {a.captions} captions: KD {kd[0]:.2f} ms / query [{kd[1]:.2f}, {kd[2]:.2f}]   policy {rl[0]:.2f} [{rl[1]:.2f}, {rl[2]:.2f}]", flush=True)
    eng.close()
    res.update(config="B/16 student + L/14 reward, 3 steps, lr 1e-6", precision=a.prec)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
