"""Generate tests/golden/retkd_*.npz by running the REFERENCE's retrieval distillation entry (retrieval/clip_ret_kd.py, imported
read-only) on this repo's seeded synthetic weights / images / caption banks.  Build container only.

    python tests/golden/make_retrieval_kd_golden.py

What is imported from the reference and exercised: `kd_distill_loss_v2`, `tune_image`, `tune_text`, `test_time_tune`
(retrieval/clip_ret_kd.py:37-150) with `CLIPRet_TTA` and `CLIPRewards` (calulate_similarity, retrieval/clip_reward.py:218-227), and
`RetrievalTask._report_metrics` (retrieval/lavis/tasks/retrieval.py:54-107, loaded by path with its LAVIS imports stubbed; only the
returned numbers are kept).  The LAVIS stubs and the synthetic tokenizer are make_retrieval_golden.py's.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import tempfile
import types
import warnings
from copy import deepcopy

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_retrieval_golden as MG  # noqa: E402
from make_retrieval_golden import REF, STATE, save, setup, synth, RR, RT  # noqa: E402
sys.path.insert(0, os.path.dirname(HERE))
from retrieval_kd_ref import METRIC_KEYS, OPS_CASES, ops_rows, random_scores  # noqa: E402  (seeded inputs shared with the tests)

def import_kd(ref):
    """retrieval/clip_ret_kd.py imports `retrieval.clip_reward` (the reference root on sys.path) and `params`; the /YOUR/PATH gate of
    clip_reward is opened again for that second import."""
    sys.path.insert(0, REF)
    _exists = os.path.exists
    os.path.exists = lambda p: True if p == "/YOUR/PATH" else _exists(p)
    try:
        import clip_ret_kd
    finally:
        os.path.exists = _exists
    return clip_ret_kd


def import_report_metrics():
    tmp = tempfile.mkdtemp()
    reg = types.SimpleNamespace(get_path=lambda k: tmp, register_task=lambda name: (lambda cls: cls))
    for name, attrs in [("lavis.common.registry", dict(registry=reg)), ("lavis.tasks.base_task", dict(BaseTask=object)),
                        ("lavis.common.dist_utils", dict(is_main_process=lambda: True, get_rank=lambda: 0, init_distributed_mode=lambda *a: None))]:
        m = types.ModuleType(name)
        for k, v in attrs.items():
            setattr(m, k, v)
        sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("ref_lavis_retrieval", os.path.join(REF, "retrieval/lavis/tasks/retrieval.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.RetrievalTask._report_metrics


def hook_first(pmap, names):
    first = {}

    def keep_first(n):
        def hook(g):                         # must return None: a returned tensor would REPLACE the gradient
            first.setdefault(n, g.detach().clone())
        return hook

    for n in names:
        pmap[n].register_hook(keep_first(n))
    return first


def grab_forward(model, which):
    """first-step logits (which = 0: logits_per_image, 1: logits_per_text) and their gradient"""
    grabbed, orig = {}, model.forward

    def forward(images=None, text=None, tokenized_prompts=None):
        out = orig(images=images, text=text, tokenized_prompts=tokenized_prompts)
        lt = out[which]
        if "logits" not in grabbed and lt.requires_grad:
            grabbed["logits"] = lt.detach().clone()

            def hook(g):
                grabbed.setdefault("dlogits", g.detach().clone())
            lt.register_hook(hook)
        return out

    model.forward = forward
    return grabbed, orig


def tap_teacher(rm, taps):
    orig = rm.calulate_similarity

    def sim():
        li, lt = orig()
        taps.setdefault("per_image", li.detach().clone())
        return li, lt

    rm.calulate_similarity = sim


def gen_i2t(ref, kd, name, n_img, steps, lr, n_bank=300):
    s_geo, r_geo, s_sd, r_sd, scaler, rm = setup(ref, "tiny", "tiny-r", n_bank, 1)
    bank = STATE["bank"]
    model = ref.models.CLIPRet_TTA("cpu", arch="student", only_visual=True, momentum_update=False)
    with torch.no_grad():
        text_ids = ref.policy.tokenize_all_text(bank.texts, types.SimpleNamespace(device="cpu"), 128)
        model.set_text_features(text_features=ref.policy.get_all_text_embeds(text_ids, model, 128))
        rm.set_many_text_features(bank.texts, text_bs=128)
    optimizer = torch.optim.AdamW(model.parameters(), lr=lr, eps=1e-06, weight_decay=5e-4)
    names = [n for n, _ in model.clip_model.visual.named_parameters()]
    assert ["visual." + n for n in names] == RR.visual_param_keys(s_sd)
    pmap = dict(model.clip_model.visual.named_parameters())
    pristine = {n: p.detach().clone() for n, p in pmap.items()}
    first = hook_first(pmap, names)
    taps = {}
    tap_teacher(rm, taps)
    grabbed, orig_forward = grab_forward(model, 0)
    image = synth.make_views(1000, n_img, s_geo.image_resolution)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kd.tune_image(image, model, rm, optimizer, scaler, args=types.SimpleNamespace(tta_steps=steps))
    model.eval()
    with torch.no_grad():
        logits_per_image, _ = orig_forward(image)
    loss = kd.kd_distill_loss_v2(grabbed["logits"], taps["per_image"])
    arrays = dict(logits=grabbed["logits"], teacher=taps["per_image"], loss=loss, dlogits=grabbed["dlogits"], final_logits=logits_per_image[:1],
                  grad_l2=torch.stack([first[n].double().norm() for n in names]).float(),
                  delta_l2=torch.stack([(pmap[n].detach() - pristine[n]).double().norm() for n in names]).float(),
                  grad_sample=torch.cat([first[n].reshape(-1) for n in names])[::7].clone(),
                  after_sample=torch.cat([pmap[n].detach().reshape(-1) for n in names])[::7].clone())
    save(name, arrays, dict(student="tiny", reward="tiny-r", n_bank=n_bank, n_img=n_img, tta_steps=steps, lr=lr, eps=1e-6, weight_decay=5e-4,
                            student_seed=11, reward_seed=23, bank_seed=7, view_seed=1000))
    print(f"  {name}: loss={float(loss):.6f} |g|={float(arrays['grad_l2'].norm()):.3e} |dlogits|={float(grabbed['dlogits'].norm()):.3e}")


def gen_t2i(ref, kd, name, steps, lr, n_images=200, query="c5."):
    s_geo, r_geo, s_sd, r_sd, scaler, rm = setup(ref, "tiny", "tiny-r", 64, 1)
    model = ref.models.CLIPRet_TTA("cpu", arch="student", only_visual=False, momentum_update=False)
    images = synth.make_views(3000, n_images, s_geo.image_resolution)
    with torch.no_grad():
        model.set_image_features(image_features=model.get_image_features(images))
        rm.set_image_features(images=images)
    optimizer = torch.optim.AdamW(model.parameters(), lr=lr, eps=1e-06, weight_decay=5e-4)
    pmap = {n: p for n, p in model.clip_model.named_parameters() if "visual" not in n}
    names = list(pmap)
    assert names == RT.text_param_keys(s_sd), names
    pristine = {n: p.detach().clone() for n, p in pmap.items()}
    first = hook_first(pmap, names)
    taps = {}
    tap_teacher(rm, taps)
    grabbed, orig_forward = grab_forward(model, 1)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        kd.tune_text(query, model, rm, optimizer, scaler, args=types.SimpleNamespace(tta_steps=steps))
    model.eval()
    with torch.no_grad():
        _, final = orig_forward(images=None, text=query)
    teacher = taps["per_image"].t().contiguous()
    loss = kd.kd_distill_loss_v2(grabbed["logits"], teacher)
    zero = torch.zeros(())
    arrays = dict(logits=grabbed["logits"], teacher=teacher, loss=loss, dlogits=grabbed["dlogits"], final_logits=final, reward_text=rm.text_features,
                  grad_l2=torch.stack([first.get(n, zero).double().norm() for n in names]).float(),
                  delta_l2=torch.stack([(pmap[n].detach() - pristine[n]).double().norm() for n in names]).float(),
                  grad_sample=torch.cat([first[n].reshape(-1) for n in names])[::7].clone(),
                  after_sample=torch.cat([pmap[n].detach().reshape(-1) for n in names])[::7].clone())
    save(name, arrays, dict(student="tiny", reward="tiny-r", n_images=n_images, tta_steps=steps, lr=lr, eps=1e-6, weight_decay=5e-4, student_seed=11,
                            reward_seed=23, bank_seed=7, bank_size=64, image_seed=3000, query_row=int(query[1:-1])))
    print(f"  {name}: loss={float(loss):.6f} |g|={float(arrays['grad_l2'].norm()):.3e} max|final-first|={float((final - grabbed['logits']).abs().max()):.3e}")


def gen_ops(kd, name):
    arrays = {}
    for i, (n, C, ts, tt, seed) in enumerate(OPS_CASES):
        s, t = ops_rows(n, C, seed)
        s64 = s.double().requires_grad_(True)
        loss = kd.kd_distill_loss_v2(s64, t.double(), T_stu=ts, T_tea=tt)
        loss.backward()
        g = s64.grad.reshape(-1)
        arrays[f"loss_{i}"] = loss.detach()
        arrays[f"grad_sample_{i}"] = g[::7].clone()
        arrays[f"grad_norm_{i}"] = g.norm()
    save(name, arrays, dict(cases=np.asarray(OPS_CASES, dtype=np.float64)))


class Loader:
    """about 6 images x 3 captions, one image per item"""

    def __init__(self, images, texts):
        self.dataset = types.SimpleNamespace(image=[f"i{k}.jpg" for k in range(images.shape[0])], text=texts, vis_root="/nowhere")
        self.images = images

    def __iter__(self):
        for k in range(self.images.shape[0]):
            yield {"image": self.images[k: k + 1]}

    def __len__(self):
        return self.images.shape[0]


def gen_loop(ref, kd, report, name, n_img=6, per=3, steps=1, lr=1e-4):
    n_txt = n_img * per
    out = {}
    for direction in ("image2text", "text2image"):
        s_geo, r_geo, s_sd, r_sd, scaler, rm = setup(ref, "tiny", "tiny-r", n_txt, 1)
        bank = STATE["bank"]
        model = ref.models.CLIPRet_TTA("cpu", arch="student", only_visual=direction == "image2text", momentum_update=False)
        loader = Loader(synth.make_views(4000, n_img, s_geo.image_resolution), bank.texts)
        optimizer = torch.optim.AdamW(model.parameters(), lr=lr, eps=1e-06, weight_decay=5e-4)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            i2t, t2i = kd.test_time_tune(loader, "cpu", model, reward_model=rm, scaler=scaler, optimizer=optimizer,
                                         optim_state=deepcopy(optimizer.state_dict()), text_bs=128, args=types.SimpleNamespace(tta_steps=steps))
        out[direction] = (i2t, t2i)
    i2t, t2i = out["image2text"][0], out["text2image"][1]
    assert (out["image2text"][1] == -100).all() and (out["text2image"][0] == -100).all()
    txt2img = [k // per for k in range(n_txt)]
    img2txt = [list(range(k * per, (k + 1) * per)) for k in range(n_img)]
    arrays = dict(score_i2t=i2t, score_t2i=t2i, txt2img=np.asarray(txt2img), img2txt=np.asarray(img2txt))
    m = report(i2t, t2i, txt2img, img2txt)
    arrays["metrics_loop"] = np.asarray([m[k] for k in METRIC_KEYS], dtype=np.float64)
    # two seeded tie-free random matrices at a size where recall@1/5/10 differ: 40 images x 5 captions (regenerated in the test)
    for j, seed in enumerate((31, 32)):
        a, b, t2, i2 = random_scores(seed)
        m = report(a, b, t2, i2)
        arrays[f"metrics_rand{j}"] = np.asarray([m[k] for k in METRIC_KEYS], dtype=np.float64)
    save(name, arrays, dict(n_img=n_img, per=per, tta_steps=steps, lr=lr, eps=1e-6, weight_decay=5e-4, student_seed=11, reward_seed=23, bank_seed=7,
                            view_seed=4000, rand_seeds=np.asarray([31, 32]), rand_n_img=40, rand_per=5))
    print(f"  {name}: loop metrics {arrays['metrics_loop'].round(2).tolist()}  rand0 {arrays['metrics_rand0'].round(2).tolist()}")


def main():
    torch.set_num_threads(min(os.cpu_count(), 16))
    ref = MG.import_reference()
    kd = import_kd(ref)
    report = import_report_metrics()
    gen_ops(kd, "retkd_ops")
    gen_i2t(ref, kd, "retkd_i2t_tiny", n_img=1, steps=2, lr=1e-4)
    gen_i2t(ref, kd, "retkd_i2t_tiny_b2", n_img=2, steps=1, lr=1e-4)
    gen_t2i(ref, kd, "retkd_t2i_tiny", steps=2, lr=1e-4)
    gen_loop(ref, kd, report, "retkd_loop_tiny")


if __name__ == "__main__":
    main()
