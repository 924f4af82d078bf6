"""Generate the zero-shot fixtures (TPT/zero_shot.py, CLIPCLS_TTA / CLIPCLS_TTA_Multiple of TPT/clip/custom_clip.py): the reference
itself, imported read-only as make_golden.py imports it, run on CPU in float32 on this repo's seeded synthetic weights, images and token
banks.  Only arrays and short meta strings are stored.

  zeroshot_ops.npz        the mixing expression custom_clip.py:561-565 — per model `logit_scale * img @ txt.t()`, then
                          torch.mean(torch.stack(...)) — in float64 (the bar) and float32 (for information: max|f32 - f64| is printed per
                          case) for the cases of OP_CASES.  Inputs come from a seed (zeroshot_ref.op_inputs, shared with the tests).
                          Large n x large C keeps the first and the last row (`_keep`).
  zeroshot_tiny / _tinyrn / _ens2 / _ens3res / _ens_student_res
                          five test images (a batch that fills no tile) and 16 classes through the reference's own classes: logits
                          [5, 16], top-5, per model the normalised image features and class features; _ens2 also the class features and
                          logits after reset_classnames_and_state with a second class list
  zeroshot_eval_tiny.npz  11 images with targets in batches of 4 (4 + 4 + 3) through the reference's test_time_adapt_eval, for the
                          single model and for ens2: the returned [acc1, acc5], per-image top-5, hit counts

The image seeds are searched upwards until, in the reference's logits, every gap that decides a stored top-5 entry or a counted hit
exceeds 2 x LOGIT_BAR (zeroshot_ref.margins); the condition is asserted on what is written.
Usage: python tests/golden/make_zeroshot_golden.py [--only ops,tuples,eval]
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402
from make_golden import synth  # noqa: E402
import zeroshot_ref as ZR  # noqa: E402

LOGIT_BAR = ZR.LOGIT_BAR
PREFIX = "a_photo_of_a"
MODEL_SEEDS = (11, 23, 29, 31, 37)      # student, further models
BANK_SEED, N_CLS, N_IMG = 7, 16, 5
CLASSES2 = (9, 2, 14, 5, 0, 11, 7)      # the second class list of reset_classnames_and_state

# ------------------------------------------------------------------ op level
OP_CASES = (      # name, widths, n, C
    ("m1_n1_c1", (64,), 1, 1),
    ("m1_n3_c4", (128,), 3, 4),
    ("m2_n16_c5", (512, 768), 16, 5),
    ("m2_n17_c7", (128, 64), 17, 7),
    ("m3_n17_c63", (640, 1024, 64), 17, 63),
    ("m5_n64_c1000", (512, 768, 1024, 640, 128), 64, 1000),
    ("m2_n64_c1003", (512, 768), 64, 1003),
    ("m3_n3_c1003", (768, 128, 640), 3, 1003),
    ("m1_n16_c1000", (1024,), 16, 1000),
    ("strided_m2_n3_c63", (128, 64), 3, 63),      # (the test lays both operands out with row strides D + 4 and the logits with C + 3)
    ("tie_m2_n3_c7", (128, 64), 3, 7),            # text rows 2 and 5 are the same row: both at the top, the lower index first
)
OP_TIE_GAP = 1e-4        # float64 gap between ranks 1 .. 6 of every row (the deliberate tie apart): ~1e4 float32 ulps of a logit of 10


def reference_mix(imgs, txts, scales, dtype):
    """custom_clip.py:560-565 on given features"""
    all_logits = []
    for a, t, s in zip(imgs, txts, scales):
        logit_scale = torch.tensor(s, dtype=dtype)
        all_logits.append(logit_scale * a.to(dtype) @ t.to(dtype).t())
    return torch.mean(torch.stack(all_logits, dim=0), dim=0)


def gen_ops():
    arrays, names = {}, []
    for k, (name, widths, n, C) in enumerate(OP_CASES):
        tie = name.startswith("tie")
        for seed in range(800 + 10 * k, 800 + 10 * k + 10):
            imgs, txts, scales = ZR.op_inputs(widths, n, C, seed, tie=tie)
            l64, l32 = reference_mix(imgs, txts, scales, torch.float64), reference_mix(imgs, txts, scales, torch.float32)
            x = l64.numpy().copy()
            if tie:
                t5 = ZR.top5(x)
                assert (t5[:, 0] == 2).all() and (t5[:, 1] == 5).all() and np.array_equal(x[:, 2], x[:, 5])
                x = np.delete(x, 5, axis=1)
            if ZR.margins(x) > OP_TIE_GAP or C == 1:
                break
        else:
            raise RuntimeError(f"{name}: no seed separates the top six entries of every row")
        assert np.abs(ZR.mix_f64(imgs, txts, scales) - l64.numpy()).max() < 1e-12
        keep = list(range(n)) if n * C <= 4096 else [0, n - 1]
        arrays[name + "_logits64"], arrays[name + "_logits32"] = l64[keep].numpy(), l32[keep].numpy()
        arrays[name + "_keep"], arrays[name + "_seed"] = np.asarray(keep, dtype=np.int64), np.int64(seed)
        arrays[name + "_widths"], arrays[name + "_n"], arrays[name + "_C"] = np.asarray(widths, dtype=np.int64), np.int64(n), np.int64(C)
        print(f"  {name:20s} seed {seed}  max|f32 - f64| {float((l32.double() - l64).abs().max()):.3g}  max|f64| {float(l64.abs().max()):.3g}")
        names.append(name)
    MG.save("zeroshot_ops", arrays, dict(cases=",".join(names), strided_pad=4, logits_pad=3))


# ------------------------------------------------------------------ the reference's classes
TUPLES = {      # name -> (archs, default_resolutions or None: CLIPCLS_TTA)
    "zeroshot_tiny": (("tiny",), None),
    "zeroshot_tinyrn": (("tiny-rn32",), None),
    "zeroshot_ens2": (("tiny", "tiny-r"), 32),
    "zeroshot_ens3res": (("tiny", "tiny-r64", "tiny-rn"), 32),
    "zeroshot_ens_student_res": (("tiny-r64", "tiny"), 32),
}


def build_model(ref, archs, default_res):
    geos = [synth.GEOMETRIES[a] for a in archs]
    MG.install_models(ref, {a: (g, synth.make_state_dict(g, seed=s)) for a, g, s in zip(archs, geos, MODEL_SEEDS)})
    bank = MG.Bank(geos[0], N_CLS, 4, seed=BANK_SEED)
    ref.custom.tokenize = bank.tokenize
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        if default_res is None:
            model = ref.custom.CLIPCLS_TTA("cpu", bank.classnames, arch=archs[0], prompt_prefix=PREFIX)
        else:
            model = ref.custom.CLIPCLS_TTA_Multiple("cpu", bank.classnames, arch=list(archs), prompt_prefix=PREFIX, default_resolutions=default_res)
    assert torch.equal(model.tokenized_prompts, bank.tokens)
    return model.eval(), geos, (default_res or geos[0].image_resolution)


def features_of(model, images):
    """per model: normalised image features and class features"""
    with torch.no_grad():
        if hasattr(model, "clip_models"):
            return model.extract_image_features(images), list(model.class_features)
        f = model.clip_model.encode_image(images)
        return [f / f.norm(dim=-1, keepdim=True)], [model.class_features]


def search_images(model, res, n, seed0, targets_of=None):
    """the first image seed from seed0 whose reference logits meet the margins -> (seed, images, logits, targets or None)"""
    for seed in range(seed0, seed0 + 200):
        images = synth.make_views(seed, n, res)
        with torch.no_grad():
            logits = model(images)
        targets = targets_of(logits) if targets_of else None
        gap = ZR.margins(logits.numpy(), targets)
        if gap > 2 * LOGIT_BAR:
            return seed, images, logits, targets
        print(f"    image seed {seed}: smallest deciding gap {gap:.3g}  REJECTED")
    raise RuntimeError("no image seed meets the margins")


def gen_tuples(ref):
    for name, (archs, default_res) in TUPLES.items():
        model, geos, res = build_model(ref, archs, default_res)
        seed, images, logits, _ = search_images(model, res, N_IMG, 3000)
        feats, cls = features_of(model, images)
        out = dict(logits=logits.numpy(), top5=ZR.top5(logits.numpy()))
        assert np.array_equal(out["top5"], torch.topk(logits, 5, dim=-1).indices.numpy())
        for m, (f, c) in enumerate(zip(feats, cls)):
            out[f"feat{m}"], out[f"cls{m}"] = f.numpy(), c.numpy()
        if name == "zeroshot_ens2":
            names2 = [f"c{i}" for i in CLASSES2]
            with torch.no_grad():
                model.reset_classnames_and_state(names2, list(archs))
                logits2 = model(images)
            assert ZR.margins(logits2.numpy()) > 2 * LOGIT_BAR and model.n_cls == len(CLASSES2)
            out["logits_reset"], out["top5_reset"] = logits2.numpy(), ZR.top5(logits2.numpy())
            for m, c in enumerate(model.class_features):
                out[f"cls{m}_reset"] = c.numpy()
        assert ZR.margins(out["logits"]) > 2 * LOGIT_BAR
        print(f"  {name}: image seed {seed}  smallest deciding gap {ZR.margins(out['logits']):.3g}  top5[0] {out['top5'][0].tolist()}")
        MG.save(name, out, dict(archs=",".join(archs), default_resolutions=int(default_res or 0), in_res=int(res), n_img=N_IMG, n_cls=N_CLS,
                                model_seeds=",".join(str(s) for s in MODEL_SEEDS[: len(archs)]), bank_seed=BANK_SEED, prefix=PREFIX,
                                image_seed=seed, classes_reset=",".join(str(i) for i in CLASSES2), kind="zeroshot"))


# ------------------------------------------------------------------ the evaluation loop
EVAL_N, EVAL_BATCH = 11, 4
EVAL_RANKS = (0, 0, 0, 0, 1, 2, 4, 7, 9, 0, 3)      # image i's target = the class at this rank of the SINGLE model's logits


def import_zero_shot():
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return importlib.import_module("zero_shot")


def run_eval(Z, model, images, targets):
    """the reference's test_time_adapt_eval over a list loader of EVAL_BATCH-image batches, on this CPU: `.cuda(...)` is the identity
    for the call's duration (the loop moves every batch with it, zero_shot.py:141-152)"""
    loader = [(images[i: i + EVAL_BATCH].clone(), targets[i: i + EVAL_BATCH].clone()) for i in range(0, images.shape[0], EVAL_BATCH)]
    args = types.SimpleNamespace(gpu=0, print_freq=1000)
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            return Z.test_time_adapt_eval(loader, model, None, None, None, args)
    finally:
        torch.Tensor.cuda = cuda


def gen_eval(ref):
    Z = import_zero_shot()
    single, _, res = build_model(ref, ("tiny",), None)

    def targets_of(logits):
        order = logits.argsort(dim=1, descending=True)
        return order[torch.arange(EVAL_N), torch.tensor(EVAL_RANKS)]

    seed = 4000
    while True:
        seed, images, logits_s, targets = search_images(single, res, EVAL_N, seed, targets_of)
        ens, _, _ = build_model(ref, ("tiny", "tiny-r"), 32)
        with torch.no_grad():
            logits_e = ens(images)
        if ZR.margins(logits_e.numpy(), targets) > 2 * LOGIT_BAR:
            break
        seed += 1
    out = dict(targets=targets.numpy(), image_seed=np.int64(seed))
    for tag, archs, dres, logits in (("single", ("tiny",), None, logits_s), ("ens2", ("tiny", "tiny-r"), 32, logits_e)):
        model, _, _ = build_model(ref, archs, dres)
        acc = run_eval(Z, model, images, targets)
        t5 = ZR.top5(logits.numpy())
        h1, h5 = ZR.hit_counts(t5, targets.numpy())
        assert acc == [round(100.0 * h1 / EVAL_N, 3), round(100.0 * h5 / EVAL_N, 3)]          # accuracy weighted by batch size = hits / images
        assert 0 < h1 < h5 < EVAL_N, (tag, h1, h5)
        assert ZR.margins(logits.numpy(), targets.numpy()) > 2 * LOGIT_BAR
        out.update({f"acc_{tag}": np.asarray(acc, dtype=np.float64), f"top5_{tag}": t5, f"hits_{tag}": np.asarray([h1, h5], dtype=np.int64),
                    f"logits_{tag}": logits.numpy()})
        print(f"  zeroshot_eval_tiny [{tag}]: image seed {seed}  acc {acc}  hits {h1}, {h5} of {EVAL_N}")
    MG.save("zeroshot_eval_tiny", out, dict(n_img=EVAL_N, batch=EVAL_BATCH, n_cls=N_CLS, in_res=int(res), bank_seed=BANK_SEED, prefix=PREFIX,
                                            model_seeds=",".join(str(s) for s in MODEL_SEEDS[:2]), archs_single="tiny", archs_ens2="tiny,tiny-r",
                                            kind="zeroshot_eval"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="ops,tuples,eval", help="comma list of ops / tuples / eval")
    a = ap.parse_args()
    torch.set_num_threads(min(os.cpu_count() or 1, 16))
    parts = a.only.split(",")
    if "ops" in parts:
        gen_ops()
    if "tuples" in parts or "eval" in parts:
        ref = MG.import_reference()
        if "tuples" in parts:
            gen_tuples(ref)
        if "eval" in parts:
            gen_eval(ref)


if __name__ == "__main__":
    main()
