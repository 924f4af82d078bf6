"""CPU: the CoCoOp fixtures (tests/golden/cocoop_*.npz, written by tests/golden/make_cocoop_golden.py from the reference's own
TPT/clip/cocoop.py) against a numpy restatement of the meta-net, the state-dict keys and checkpoint loading of the mirror
(rlcf_amd.cocoop), and the refusals of the mirror's --cocoop path (rlcf_amd.tpt_cls).  No engine is built here."""
import types

import numpy as np
import pytest
import torch

import cocoop_ref as CR
from rlcf_amd import synth

OPS, OPS_META = CR.op_cases()


@pytest.mark.parametrize("name,shape,x,g", OPS, ids=[c[0] for c in OPS])
def test_numpy_meta_net_reproduces_the_reference_float64(name, shape, x, g):
    """ctx + W2 relu(W1 f + b1) + b2 in float64, rows and mean form, against the reference's float64 module: only the summation order
    differs (a few ulp of float64 on sums of |terms| <= 1); the reference's own float32 result sits ~1e-8 away"""
    D, H, W, n_ctx, n = shape
    keep = g["keep"].tolist()
    rows, mean = CR.meta_net_f64(x)[keep], CR.meta_net_f64(x, mean=True)
    assert rows.shape == (len(keep), n_ctx, W) == tuple(g["rows64"].shape) and mean.shape == (1, n_ctx, W) == tuple(g["mean64"].shape)
    assert np.abs(rows - g["rows64"].numpy()).max() < 1e-14 and np.abs(mean - g["mean64"].numpy()).max() < 1e-14
    assert g["mean32"].dtype == torch.float32 and np.abs(g["mean32"].numpy() - mean).max() < 1e-6
    # the cases are what the issue lists, and each has clamped and unclamped hidden units in both forms
    for f in (x["feats"].double().numpy(), x["feats"].double().numpy().mean(axis=0, keepdims=True)):
        hid = f @ x["w1"].double().numpy().T + x["b1"].double().numpy()
        assert (hid <= 0).any() and (hid > 0).any()
    assert H == D // 16


def test_op_cases_are_the_listed_shapes():
    shapes = {CR.case_shape(c[0]) for c in OPS if not c[0].startswith("strided")}
    assert shapes == {(64, 4, 64, 4, 1), (128, 8, 128, 1, 3), (256, 16, 256, 4, 1), (640, 40, 640, 16, 2), (768, 48, 768, 4, 64), (1024, 64, 512, 4, 7)}
    assert sum(c[0].startswith("strided") for c in OPS) == 1 and int(OPS_META["strided_pad"]) == 3


@pytest.mark.parametrize("case", ["cocoop_tiny_s0", "cocoop_tiny_s1", "cocoop_small_s1", "cocoop_tinyrn_s1"])
def test_e2e_fixtures_hold_their_margins(case):
    """what make_cocoop_golden.py asserted when it chose the view seed, re-derived from the stored arrays: the generated prompt is the
    seeded state's ctx plus one shift broadcast over the rows, the step moved it, top-5 is stable against the 1e-3 logits bar"""
    g, meta = CR.load_golden(case)
    geo = synth.GEOMETRIES[meta["student"]]
    state = synth.make_cocoop_state(geo, meta["cocoop_seed"], meta["n_ctx"])
    x = dict(feats=g["image_features"][:1], ctx=state["ctx"], w1=state["meta_net.linear1.weight"], b1=state["meta_net.linear1.bias"],
             w2=state["meta_net.linear2.weight"], b2=state["meta_net.linear2.bias"])
    np.testing.assert_allclose(g["ctx_gen"].numpy(), CR.meta_net_f64(x)[0], rtol=0, atol=1e-6)
    assert g["image_features"].shape == (meta["n_views"], geo.embed_dim) and float(g["image_features"].norm(dim=1).min()) > 2.0   # un-normalised
    fl = g["final_logits"][0].sort(descending=True)
    assert fl.indices[:5].tolist() == g["top5"].tolist() and float(fl.values[4] - fl.values[5]) > 0.02
    if meta["tta_steps"] == 0:
        assert torch.equal(g["ctx_after"], g["ctx_gen"]) and "loss" not in g
    else:
        assert not torch.equal(g["ctx_after"], g["ctx_gen"])
        assert g["selected_idx"].numel() == int(meta["n_views"] * meta["selection_p"])


# ------------------------------------------------------------------------------ the mirror, without an engine
@pytest.fixture()
def model():
    from rlcf_amd import clip_store, cocoop, runtime
    runtime.reset_session()
    sg = synth.GEOMETRIES["tiny"]
    clip_store.register_checkpoint("tiny", sg, synth.make_state_dict(sg, 11))
    bank = clip_store.SyntheticBank(sg, 16, 4, 7)
    clip_store.set_tokenizer(bank.tokenize)
    m = cocoop.get_cocoop("tiny", "I", "cpu", 4, classnames=bank.classnames)
    yield m
    runtime.reset_session()


def test_state_dict_keys_equal_the_reference(model):
    keys = OPS_META["state_dict_keys"].split(",")
    assert list(model.prompt_generator.state_dict().keys()) == keys
    assert [k for k in model.state_dict().keys()] == ["prompt_generator." + k for k in keys]
    pg = model.prompt_generator
    assert pg.n_ctx == 4 and pg.n_cls == 16 and tuple(pg.tokenized_prompts.shape) == (16, 77) and model.tokenized_prompts is pg.tokenized_prompts
    assert tuple(pg.ctx.shape) == (4, 128) and tuple(pg.meta_net.linear1.weight.shape) == (8, 128) and tuple(pg.meta_net.linear2.weight.shape) == (128, 8)
    assert tuple(pg.token_prefix.shape) == (16, 1, 128) and tuple(pg.token_suffix.shape) == (16, 72, 128)
    pg.reset_classnames(["c3", "c5"], "tiny")
    assert pg.n_cls == 2 and tuple(pg.token_suffix.shape) == (2, 72, 128) and list(pg.state_dict().keys()) == keys


def test_load_cocoop_weights_drops_the_token_vectors(model, tmp_path):
    from rlcf_amd import cocoop, runtime
    pg = model.prompt_generator
    state = synth.make_cocoop_state(synth.GEOMETRIES["tiny"], 31, 4)
    prefix0 = pg.token_prefix.clone()
    sd = dict(state, token_prefix=torch.zeros(3, 1, 128), token_suffix=torch.zeros(3, 5, 128))      # (another class list's: wrong shapes)
    loaded = cocoop.load_cocoop_weights({"state_dict": sd, "epoch": 1}, model)
    assert loaded == sorted(state) and torch.equal(pg.token_prefix, prefix0)
    for k, v in state.items():
        assert torch.equal(pg.state_dict()[k].cpu(), v), k
    # a file, a bare state dict and whole-model key names load the same way
    path = tmp_path / "cocoop.pth"
    torch.save({"state_dict": {"prompt_generator." + k: v * 2 for k, v in sd.items()}}, path)
    assert cocoop.load_cocoop_weights(str(path), model) == sorted(state)
    assert torch.equal(pg.ctx.detach().cpu(), state["ctx"] * 2)
    assert cocoop.load_cocoop_weights(state, model) == sorted(state) and torch.equal(pg.ctx.detach().cpu(), state["ctx"])
    # the session's copies follow the Parameters: a load or an in-place edit is seen, a second look without a write is not
    pg._sync_engine()
    v0 = (runtime.SESSION._bank_version, runtime.SESSION._meta_version)
    pg._sync_engine()
    assert (runtime.SESSION._bank_version, runtime.SESSION._meta_version) == v0
    with torch.no_grad():
        pg.meta_net.linear2.bias.add_(1.0)
    pg._sync_engine()
    assert runtime.SESSION._meta_version == v0[1] + 1 and torch.equal(runtime.SESSION.meta_net[3].cpu(), state["meta_net.linear2.bias"] + 1.0)
    assert torch.equal(runtime.SESSION.ctx_init.cpu(), state["ctx"])


def _args(**kw):
    base = dict(cocoop=True, tpt=True, tta_steps=1, selection_p=0.5, lr=5e-3, gpu=0, print_freq=1000)
    base.update(kw)
    return types.SimpleNamespace(**base)


def test_mirror_refusals(model):
    from rlcf_amd import tpt_cls
    inputs = (torch.zeros(8, 128), torch.zeros(1, 4, 128))
    with pytest.raises(NotImplementedError, match="tpt_cls.py:60"):
        tpt_cls.test_time_tuning(model, inputs, None, None, _args(tta_steps=2))
    with pytest.raises(NotImplementedError, match="tpt_cls.py:60"):
        tpt_cls.test_time_adapt_eval([], model, None, None, None, None, _args(tta_steps=2))
    with pytest.raises(NotImplementedError, match="images_per_pass"):
        tpt_cls.test_time_adapt_eval([], model, None, None, None, None, _args(images_per_pass=2))
    with pytest.raises(NotImplementedError, match="in_flight"):
        tpt_cls.test_time_adapt_eval([], model, None, None, None, None, _args(in_flight=2))
    with pytest.raises(NotImplementedError, match="args.tpt = False"):
        tpt_cls.test_time_adapt_eval([], model, None, None, None, None, _args(tpt=False))
    for other in (None, object()):
        with pytest.raises(NotImplementedError, match="get_cocoop"):
            tpt_cls.test_time_tuning(other, inputs, None, None, _args())
        with pytest.raises(NotImplementedError, match="get_cocoop"):
            tpt_cls.test_time_adapt_eval([], other, None, None, None, None, _args())
    # zero steps: the generated prompt comes back untouched, no engine needed
    assert tpt_cls.test_time_tuning(model, inputs, None, None, _args(tta_steps=0)) is inputs[1]
