"""Host-side mirror of the zero-shot entry (TPT/zero_shot.py): `main_worker` (:30-128) and `test_time_adapt_eval` (:131-172) with the
reference's signatures.  This is the "CLIP zero-shot" row of the paper's tables and, with CLIPCLS_TTA_Multiple, its "zero-shot
ensemble" row.

The loop differs from the tuning loops: a batch holds `args.batch_size` DIFFERENT test images, nothing is reset, no optimizer steps,
and accuracy is weighted by batch size (AverageMeter.update(acc, image.size(0)), :159-161), i.e. it is hits / images.  For a
CLIPCLS_TTA or CLIPCLS_TTA_Multiple model a batch is ONE engine call (rlcf_zero_shot_batch: towers, one ensemble-logits launch,
top-5, hit counts); the hit counts stay on the device and are read once per dataset (and once per `args.print_freq` batches for the
progress line).  Any other model goes through `model(image)` and
`accuracy`, batch by batch, as the reference does.

The reference chooses between the two classes by commenting a line out (:50-51); here `--ensemble_archs a,b,...` (or a comma-separated
`--arch`) selects CLIPCLS_TTA_Multiple over those archs at `--resolution`; unset (the default), CLIPCLS_TTA(args.arch) runs.
"""
from __future__ import annotations

import json
import os
import time

import torch

from .custom_clip import CLIPCLS_TTA, CLIPCLS_TTA_Multiple
from .tpt_cls_rl import accuracy


def ensemble_archs(args):
    """the archs of the ensemble switch, or None (the default: CLIPCLS_TTA(args.arch))"""
    spec = getattr(args, "ensemble_archs", None) or (args.arch if "," in str(getattr(args, "arch", "")) else None)
    return [a.strip() for a in spec.split(",") if a.strip()] if spec else None


def _read_back(t: torch.Tensor) -> torch.Tensor:
    """the loop's one device-to-host read"""
    return t.cpu()


def _fused(model) -> bool:
    """True: the batch is one rlcf_zero_shot_batch call.  A CLIPCLS_TTA qualifies while it is the checkpoint (its tunable tensors were
    never handed out) and its forward is the inference form the call runs (a ModifiedResNet with only_norm keeps its BatchNorms on
    batch statistics, custom_clip.py:487-497)."""
    if isinstance(model, CLIPCLS_TTA_Multiple):
        return True
    return isinstance(model, CLIPCLS_TTA) and model._ln is None and model._vis is None and not (model.resnet and model.only_norm)


def test_time_adapt_eval(val_loader, model, optimizer, optim_state, scaler, args, device=None, reward_model=None):
    """TPT/zero_shot.py:131-172.  `optimizer`, `optim_state`, `scaler` and `reward_model` are accepted and unused, as in the reference.
    Returns [top1, top5] in percent, rounded to three places."""
    model.eval()
    fused = _fused(model)
    ensemble = isinstance(model, CLIPCLS_TTA_Multiple) and model.n_model > 1
    acc = None          # device float32 [2]: hits (fused) or sum of batch accuracy x batch size (generic)
    n = 0
    end = time.time()
    for i, (images, target) in enumerate(val_loader):
        on_gpu = torch.cuda.is_available()
        assert args.gpu is not None
        if isinstance(images, list):                       # zero_shot.py:141-144
            image = images[0].cuda(args.gpu, non_blocking=True) if on_gpu else images[0]
        else:
            if images.dim() > 4:                           # (the ImageNet sampler's leading 1, :146-149)
                assert images.size(0) == 1
                images = images.squeeze(0)
            image = images.cuda(args.gpu, non_blocking=True) if on_gpu else images
        target = target.cuda(args.gpu, non_blocking=True) if on_gpu else target
        bs = image.size(0)
        if fused:
            eng = model._engine(bs) if isinstance(model, CLIPCLS_TTA_Multiple) else _student_engine(bs)
            if acc is None:
                acc = torch.zeros(2, device=eng.device)
            eng.zero_shot_batch(image, ensemble=ensemble, target=target.reshape(-1), hits=acc, want_logits=False, want_top5=False)
        else:
            with torch.no_grad():
                output = model(image)
            acc1, acc5 = accuracy(output, target, topk=(1, 5))
            if acc is None:
                acc = torch.zeros(2, device=output.device)
            acc += torch.cat([acc1.reshape(1), acc5.reshape(1)]).to(acc.dtype) * (bs / 100.0)     # batch accuracy x batch size = hits
        n += bs
        if (i + 1) % getattr(args, "print_freq", 500) == 0:
            h = _read_back(acc)
            print(f"Test: [{i + 1}/{len(val_loader)}] Time {time.time() - end:6.3f} Acc@1 {float(h[0]) * 100 / n:6.2f} Acc@5 {float(h[1]) * 100 / n:6.2f}")
        end = time.time()
    if acc is None:
        return [0.0, 0.0]
    h = _read_back(acc)
    top1, top5 = float(h[0]) * 100.0 / n, float(h[1]) * 100.0 / n
    print(f" *  Acc@1 {top1:.3f} Acc@5 {top5:.3f}")
    return [round(x, 3) for x in [top1, top5]]


def _student_engine(n_images: int):
    from . import runtime
    return runtime.SESSION.engine(n_images)


def main_worker(gpu, args, build_dataset=None, classnames_of=None):
    """TPT/zero_shot.py:30-128: the dataset loop and results.json.  The reference reads its class-name lists and datasets from its
    `data` package; here the caller supplies them, duck-typed as in the other mirrors:
      classnames_of(set_id) -> list of class names of that test set;
      build_dataset(set_id, args) -> a dataset of (image [3, R, R] or a list whose first item is one, target) items
    (images already resized / cropped to args.resolution and normalised, zero_shot.py:75-80)."""
    if build_dataset is None or classnames_of is None:
        raise NotImplementedError("rlcf_amd.zero_shot.main_worker needs build_dataset(set_id, args) and classnames_of(set_id): the dataset "
                                  "classes of TPT/data are not part of this package")
    args.gpu = gpu
    torch.manual_seed(args.seed)
    device = torch.device(f"cuda:{args.gpu}") if torch.cuda.is_available() else torch.device("cpu")
    if torch.cuda.is_available():
        torch.cuda.set_device(args.gpu)
    datasets = args.test_sets.split("/")
    archs = ensemble_archs(args)
    if archs:
        model = CLIPCLS_TTA_Multiple(device, classnames_of(datasets[0]), arch=archs, prompt_prefix=args.ctx_init, default_resolutions=args.resolution)
    else:
        model = CLIPCLS_TTA(device, classnames_of(datasets[0]), arch=args.arch, prompt_prefix=args.ctx_init)
    # the reference builds an AdamW over model.parameters() here (:54-57) and never steps it; asking the mirror for its parameters would
    # materialise the tunable tensors of a model that is only evaluated, so none is built
    optimizer = optim_state = scaler = None
    results = {}
    all_start = time.time()
    for set_id in datasets:
        data_start_time = time.time()
        print("evaluating: {}".format(set_id))
        model.reset_classnames_and_state(classnames_of(set_id), archs if archs else args.arch)
        val_dataset = build_dataset(set_id, args)
        print("number of test samples: {}".format(len(val_dataset)))
        val_loader = torch.utils.data.DataLoader(val_dataset, batch_size=args.batch_size, shuffle=False, num_workers=0, pin_memory=torch.cuda.is_available())
        results[set_id] = test_time_adapt_eval(val_loader, model, optimizer, optim_state, scaler, args, device=device)
        del val_dataset, val_loader
        print("=> Acc. on testset [{}]: @1 {} / @5 {}".format(set_id, results[set_id][0], results[set_id][1]))
        data_time = time.time() - data_start_time
        print("The running time for dataset {} is {:.1f} Hour {:.1f} Minute\n".format(set_id, data_time // 3600, data_time % 3600 / 60))
    os.makedirs(args.output, exist_ok=True)
    with open(os.path.join(args.output, "results.json"), "w") as fp:
        json.dump(results, fp, indent=4)
    print("======== Result Summary ========")
    print(args.output)
    print(results)
    all_time = time.time() - all_start
    print("The total running time of the program is {:.1f} Hour {:.1f} Minute\n".format(all_time // 3600, all_time % 3600 / 60))
    return results


if __name__ == "__main__":
    from .params import get_args
    _args = get_args()
    main_worker(_args.gpu, _args)
