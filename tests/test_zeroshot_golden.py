"""CPU: the zero-shot fixtures (tests/golden/zeroshot_*.npz, written by tests/golden/make_zeroshot_golden.py from the reference's own
CLIPCLS_TTA / CLIPCLS_TTA_Multiple and TPT/zero_shot.py) against the numpy restatement of the mixing expression (tests/zeroshot_ref.py),
their own consistency (top-5, margins), the batch-size weighting of rlcf_amd.zero_shot.test_time_adapt_eval on a duck-typed CPU model,
and the params switch.  No engine is built here."""
import types

import numpy as np
import pytest
import torch

import zeroshot_ref as ZR

OPS, OPS_META = ZR.op_cases()
TUPLES = ["zeroshot_tiny", "zeroshot_tinyrn", "zeroshot_ens2", "zeroshot_ens3res", "zeroshot_ens_student_res"]


@pytest.mark.parametrize("name,shape,g", OPS, ids=[c[0] for c in OPS])
def test_numpy_mix_reproduces_the_reference_float64(name, shape, g):
    """(1 / M) sum_m s_m img_m txt_m^T in float64 against the reference expression in float64: only the summation order inside the
    products differs (sums of <= 1024 terms of size <= 1e-2 each, scaled by <= 100: a few 1e-14); the float32 result of the reference
    expression is stored for information and sits ~1e-5 away"""
    widths, n, C = shape
    imgs, txts, scales = ZR.op_inputs(widths, n, C, int(g["seed"]), tie=name.startswith("tie"))
    keep = g["keep"].tolist()
    mix = ZR.mix_f64(imgs, txts, scales)
    assert mix.shape == (n, C) and tuple(g["logits64"].shape) == (len(keep), C) and g["logits64"].dtype == torch.float64
    assert np.abs(mix[keep] - g["logits64"].numpy()).max() < 1e-12
    assert g["logits32"].dtype == torch.float32 and np.abs(g["logits32"].numpy() - mix[keep]).max() < 1e-4
    for a in imgs + txts:                                 # the rows arrive L2-normalised
        assert float((a.double().norm(dim=1) - 1).abs().max()) < 1e-6
    if name.startswith("tie"):
        t5 = ZR.top5(mix)
        assert np.array_equal(mix[:, 2], mix[:, 5]) and (t5[:, 0] == 2).all() and (t5[:, 1] == 5).all()      # the lower index first


def test_op_cases_cover_what_the_kernel_can_get_wrong():
    shapes = [c[1] for c in OPS]
    assert {len(w) for w, _, _ in shapes} == {1, 2, 3, 5}
    assert {d for w, _, _ in shapes for d in w} == {64, 128, 512, 640, 768, 1024}
    assert {n for _, n, _ in shapes} == {1, 3, 16, 17, 64} and {C for _, _, C in shapes} == {1, 4, 5, 7, 63, 1000, 1003}
    names = [c[0] for c in OPS]
    assert sum(x.startswith("strided") for x in names) == 1 and sum(x.startswith("tie") for x in names) == 1
    assert int(OPS_META["strided_pad"]) == 4 and int(OPS_META["logits_pad"]) == 3


def test_top5_restatement_sends_ties_to_the_lower_index():
    x = np.array([[1.0, 3.0, 3.0, 0.0, 3.0, 2.0, -1.0], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    assert ZR.top5(x).tolist() == [[1, 2, 4, 5, 0], [0, 1, 2, 3, 4]]
    assert ZR.top5(np.array([[2.0, 5.0, 5.0]])).tolist() == [[1, 2, 0]]


@pytest.mark.parametrize("case", TUPLES)
def test_tuple_fixtures_are_consistent_and_hold_their_margins(case):
    """the stored top-5 is the top-5 of the stored logits, every deciding gap exceeds 2 x LOGIT_BAR, and the stored logits ARE the mix
    of the stored per-model features (to float32 rounding of the reference's own float32 products)"""
    g, meta = ZR.load_golden(case)
    archs = meta["archs"].split(",")
    assert tuple(g["logits"].shape) == (5, 16) and np.array_equal(ZR.top5(g["logits"].numpy()), g["top5"].numpy())
    assert ZR.margins(g["logits"].numpy()) > 2 * ZR.LOGIT_BAR
    from rlcf_amd import synth
    scales = [float(synth.make_state_dict(synth.GEOMETRIES[a], seed=int(s))["logit_scale"].exp()) for a, s in zip(archs, meta["model_seeds"].split(","))]
    mix = ZR.mix_f64([g[f"feat{m}"] for m in range(len(archs))], [g[f"cls{m}"] for m in range(len(archs))], scales)
    assert np.abs(mix - g["logits"].numpy()).max() < 1e-4
    for m, a in enumerate(archs):
        D = synth.GEOMETRIES[a].embed_dim
        assert tuple(g[f"feat{m}"].shape) == (5, D) and tuple(g[f"cls{m}"].shape) == (16, D)
    if case == "zeroshot_ens2":
        assert tuple(g["logits_reset"].shape) == (5, 7) and np.array_equal(ZR.top5(g["logits_reset"].numpy()), g["top5_reset"].numpy())
        assert ZR.margins(g["logits_reset"].numpy()) > 2 * ZR.LOGIT_BAR
        idx = [int(i) for i in meta["classes_reset"].split(",")]
        for m in range(2):                                 # the second list's class features are rows of the first bank's
            torch.testing.assert_close(g[f"cls{m}_reset"], g[f"cls{m}"][idx], atol=1e-6, rtol=0)


def test_eval_fixture_is_consistent_and_not_degenerate():
    g, meta = ZR.load_golden("zeroshot_eval_tiny")
    n = int(meta["n_img"])
    assert n == 11 and int(meta["batch"]) == 4
    for tag in ("single", "ens2"):
        t5 = ZR.top5(g[f"logits_{tag}"].numpy())
        assert np.array_equal(t5, g[f"top5_{tag}"].numpy())
        h1, h5 = ZR.hit_counts(t5, g["targets"].numpy())
        assert [h1, h5] == g[f"hits_{tag}"].tolist() and 0 < h1 < h5 < n
        assert g[f"acc_{tag}"].tolist() == [round(100.0 * h1 / n, 3), round(100.0 * h5 / n, 3)]
        assert ZR.margins(g[f"logits_{tag}"].numpy(), g["targets"].numpy()) > 2 * ZR.LOGIT_BAR


class _FixtureModel:
    """duck-typed model without an engine: returns the fixture's logits of the images it is handed (recognised by their first pixel)"""

    def __init__(self, images, logits):
        self.keys, self.logits, self.batches = [float(im[0, 0, 0]) for im in images], logits, []

    def eval(self):
        return self

    def __call__(self, image):
        self.batches.append(image.shape[0])
        return torch.stack([self.logits[self.keys.index(float(im[0, 0, 0]))] for im in image]).to(image.device)


@pytest.mark.parametrize("tag", ["single", "ens2"])
@pytest.mark.parametrize("form", ["list", "5d", "plain"])
def test_eval_harness_weights_accuracy_by_batch_size(tag, form):
    """rlcf_amd.zero_shot.test_time_adapt_eval over 4 + 4 + 3 images reproduces the reference's [acc1, acc5] — hits / images; a mean of
    the three per-batch percentages would not (the last batch is smaller) — for list items, 5-D tensors with a leading 1 and plain
    batches"""
    from rlcf_amd import synth
    from rlcf_amd.zero_shot import test_time_adapt_eval
    g, meta = ZR.load_golden("zeroshot_eval_tiny")
    images = synth.make_views(int(g["image_seed"]), int(meta["n_img"]), int(meta["in_res"]))
    model = _FixtureModel(images, g[f"logits_{tag}"])
    b = int(meta["batch"])
    wrap = {"list": lambda x: [x, x.flip(0)], "5d": lambda x: x.unsqueeze(0), "plain": lambda x: x}[form]
    loader = [(wrap(images[i: i + b]), g["targets"][i: i + b]) for i in range(0, images.shape[0], b)]
    args = types.SimpleNamespace(gpu=0, print_freq=1000)
    acc = test_time_adapt_eval(loader, model, None, None, None, args)
    assert model.batches == [4, 4, 3]
    assert acc == g[f"acc_{tag}"].tolist()
    per_batch = []
    for i in range(0, 11, b):
        h1, _ = ZR.hit_counts(g[f"top5_{tag}"][i: i + b].numpy(), g["targets"][i: i + b].numpy())
        per_batch.append(100.0 * h1 / len(g["targets"][i: i + b]))
    assert round(float(np.mean(per_batch)), 3) != acc[0]          # the fixture tells the two weightings apart


def test_params_switch_defaults_off():
    from rlcf_amd import params, zero_shot
    a = params.get_args([])
    assert a.ensemble_archs is None and zero_shot.ensemble_archs(a) is None and a.arch == "RN50" and a.resolution == 224 and a.batch_size == 64
    assert zero_shot.ensemble_archs(params.get_args(["--ensemble_archs", "ViT-B/16,ViT-L/14"])) == ["ViT-B/16", "ViT-L/14"]
    assert zero_shot.ensemble_archs(params.get_args(["-a", "ViT-B/16,ViT-L/14"])) == ["ViT-B/16", "ViT-L/14"]
    assert zero_shot.ensemble_archs(params.get_args(["-a", "ViT-B/16"])) is None


def test_multiple_refuses_more_than_five_models():
    from rlcf_amd.custom_clip import CLIPCLS_TTA_Multiple
    with pytest.raises(NotImplementedError, match="at most 5"):
        CLIPCLS_TTA_Multiple("cpu", ["c0"], arch=["tiny"] * 6, prompt_prefix="a_photo_of_a")
