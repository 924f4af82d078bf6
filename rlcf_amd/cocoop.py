"""Host-side mirror of the reference's CoCoOp surface (TPT/clip/cocoop.py): `CoCoOpPromptLearner` (:19-137), `CoCoOpCLIP` (:139-224),
`get_cocoop` (:226-234), and `load_cocoop_weights`, the CoCoOp part of `load_model_weight` (TPT/utils/tools.py:101-131).  Same names,
argument meaning and state-dict keys; the towers, the meta-net and the prompt step run in librlcf_hip.so (rlcf_amd.engine) — these
classes hold parameters and bookkeeping only.

CoCoOp exists in the reference for `tta_steps` 0 and 1 only: at a second step its test_time_tuning indexes the (features, ctx) tuple
(TPT/tpt_cls.py:60) and stops with a TypeError."""
from __future__ import annotations

from collections import OrderedDict
from typing import List, Optional

import torch
import torch.nn as nn

from . import clip_store, runtime
from . import _lib as L
from .engine import cocoop_ctx_op, l2norm_rows


class CoCoOpPromptLearner(nn.Module):
    """TPT/clip/cocoop.py:19-137.  `ctx` [n_ctx, W] and `meta_net` = Linear(D, D // 16) -> ReLU -> Linear(D // 16, W) are real
    Parameters (a CoCoOp checkpoint loads by name); `token_prefix` / `token_suffix` are the reference's buffers.  The engine holds
    copies of ctx (as the class bank's reset prompt) and of the meta-net: they follow the Parameters at every entry point of the mirror
    — in-place edits and load_state_dict are seen through the Parameters' versions, an edit through `.data` needs `wrote()`."""

    def __init__(self, clip_model, classnames, n_ctx=4, ctx_init="a_photo_of_a", ctx_position="end"):
        super().__init__()
        self.clip_model = clip_model
        sd = clip_model.state_dict
        self.device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.dtype = torch.float32
        ctx_dim = sd["ln_final.weight"].shape[0]
        embed_dim = sd["text_projection"].shape[1]
        self.ctx_dim = ctx_dim
        table = sd["token_embedding.weight"]
        if ctx_init:                                   # cocoop.py:30-39
            ctx_init = ctx_init.replace("_", " ")
            n_ctx = len(ctx_init.split(" "))
            prompt = clip_store.tokenize(ctx_init)
            ctx_vectors = table[prompt[0, 1:1 + n_ctx].to(table.device)].float()
            prompt_prefix = ctx_init
        else:                                          # cocoop.py:41-45
            ctx_vectors = torch.empty(n_ctx, ctx_dim)
            nn.init.normal_(ctx_vectors, std=0.02)
            prompt_prefix = " ".join(["X"] * n_ctx)
        self.prompt_prefix = prompt_prefix
        self.ctx = nn.Parameter(ctx_vectors.detach().to(self.device).clone())
        self.meta_net = nn.Sequential(OrderedDict([
            ("linear1", nn.Linear(embed_dim, embed_dim // 16)),
            ("relu", nn.ReLU(inplace=True)),
            ("linear2", nn.Linear(embed_dim // 16, ctx_dim)),
        ])).to(self.device)
        self.ctx_init, self.class_token_position, self.n_ctx = ctx_init, ctx_position, n_ctx
        self._gen, self._pushed = 0, None
        self._set_classnames(classnames, register=True)

    def _tracked(self):
        m = self.meta_net
        return (self.ctx, m.linear1.weight, m.linear1.bias, m.linear2.weight, m.linear2.bias)

    def wrote(self) -> None:
        """tell the mirror that ctx or the meta-net was edited in a way a Parameter's version does not show (through `.data`)"""
        self._gen += 1

    def _set_classnames(self, classnames: List[str], register: bool = False) -> None:
        classnames = [name.replace("_", " ") for name in classnames]
        prompts = [self.prompt_prefix + " " + name + "." for name in classnames]
        self.tokenized_prompts = clip_store.tokenize(prompts).to(self.device)          # cocoop.py:62
        self.n_cls, self.classnames = len(classnames), classnames
        eot = self.tokenized_prompts.argmax(dim=-1)
        self.name_lens = [int(e) - 1 - self.n_ctx - 1 for e in eot]
        enc = getattr(getattr(clip_store._TOKENIZER, "__self__", None), "encode", None)
        if callable(enc):                              # len(_tokenizer.encode(name)), cocoop.py:59
            self.name_lens = [len(enc(name)) for name in classnames]
        table = self.clip_model.state_dict["token_embedding.weight"]
        emb = table[self.tokenized_prompts.to(table.device)].float().to(self.device)
        if register:                                   # cocoop.py:69-70
            self.register_buffer("token_prefix", emb[:, :1, :])
            self.register_buffer("token_suffix", emb[:, 1 + self.n_ctx:, :])
        else:                                          # cocoop.py:112-113
            self.token_prefix, self.token_suffix = emb[:, :1, :], emb[:, 1 + self.n_ctx:, :]
        self._pushed = None

    def reset_classnames(self, classnames, arch):      # cocoop.py:100-116 (without re-loading CLIP from disk)
        self._set_classnames(classnames)

    def _sync_engine(self) -> None:
        """the session's class bank (reset prompt = ctx) and meta-net follow the Parameters"""
        stamp = (self._gen,) + tuple(p._version for p in self._tracked()) + tuple(id(p) for p in self._tracked())
        if stamp == self._pushed:
            return
        ctx, w1, b1, w2, b2 = [p.detach() for p in self._tracked()]
        runtime.SESSION.set_bank(self.tokenized_prompts, self.n_ctx, ctx)
        runtime.SESSION.set_meta_net(w1, b1, w2, b2)
        self._pushed = stamp

    def forward(self, im_features, ctx_only=False):
        """cocoop.py:118-137: ctx + meta_net(im_features)[:, None, :] -> [batch, n_ctx, W] (rlcf_cocoop_ctx, one prompt per row);
        with ctx_only=False the prompts [batch, n_cls, 77, W] = [SOS | shifted ctx | class tokens] are materialised as well (the HIP
        text tower never needs that tensor; provided for API completeness)."""
        m = self.meta_net
        feats = im_features.detach().to(self.device, torch.float32)
        shifted = cocoop_ctx_op(feats if feats.stride(-1) == 1 else feats.contiguous(), self.ctx, m.linear1.weight, m.linear1.bias,
                                m.linear2.weight, m.linear2.bias, mean=False)
        if ctx_only:
            return shifted
        return torch.stack([torch.cat([self.token_prefix, c.unsqueeze(0).expand(self.n_cls, -1, -1), self.token_suffix], dim=1)
                            for c in shifted])


class _CtxLogitsFn(torch.autograd.Function):
    """forward_ctx (cocoop.py:184-217): logits = exp(logit_scale) * norm(image_features) @ norm(txt(ctx))^T, differentiable with respect
    to ctx; backward = rlcf_text_backward_dense (what loss.backward() does at TPT/tpt_cls.py:71).  The features are constants (they come
    from gen_ctx, which runs under no_grad)."""

    @staticmethod
    def forward(fn_ctx, ctx, image_features):
        eng = runtime.SESSION.engine(image_features.shape[0])
        ctx2 = ctx.detach().reshape(eng.n_ctx, -1).to(eng.device, torch.float32).contiguous()
        img = l2norm_rows(image_features.to(eng.device))
        fn_ctx.save_for_backward(ctx2, img)
        fn_ctx.ctx_shape = ctx.shape
        return eng.logits(img, eng.text_features(ctx2))

    @staticmethod
    def backward(fn_ctx, dlogits):
        ctx2, img = fn_ctx.saved_tensors
        eng = runtime.SESSION.engine(img.shape[0])
        return eng.text_backward_dense(ctx2, img, dlogits.contiguous().float()).reshape(fn_ctx.ctx_shape), None


class CoCoOpCLIP(nn.Module):
    """TPT/clip/cocoop.py:139-224."""

    def __init__(self, device, classnames, criterion="cosine", arch="ViT-L/14", n_ctx=16, ctx_init="a_photo_of_a", ctx_position="end"):
        super().__init__()
        clip, _, _ = clip_store.load(arch, device=device)
        self.clip = clip
        runtime.SESSION.set_student(clip)
        self.logit_scale = clip.state_dict["logit_scale"].detach().clone()
        self.prompt_generator = CoCoOpPromptLearner(clip, classnames, n_ctx, ctx_init, ctx_position)
        self.criterion = criterion
        self.dtype = torch.float32

    @property
    def tokenized_prompts(self):
        return self.prompt_generator.tokenized_prompts

    def _engine(self, n_views: int = 1):
        self.prompt_generator._sync_engine()
        return runtime.SESSION.engine(n_views)

    @torch.no_grad()
    def gen_ctx(self, image, aug=False):
        """cocoop.py:172-182 -> (un-normalised image features [N, D], generated prompt [1, n_ctx, W]): the meta-net reads row 0 (aug)
        or the mean over the rows."""
        eng = self._engine(image.shape[0])
        feats, ctx = eng.cocoop_gen_ctx(image, aug=bool(aug))
        return feats, ctx.unsqueeze(0).detach().clone()

    def forward_ctx(self, image_features, ctx):
        self._engine(image_features.shape[0])
        return _CtxLogitsFn.apply(ctx, image_features)

    @torch.no_grad()
    def inference(self, image, label=None):
        """cocoop.py:153-170: every image of the batch gets the prompt generated from its own (normalised) features — the rows form of
        rlcf_cocoop_ctx, then one text pass per image."""
        eng = self._engine(image.shape[0])
        img = l2norm_rows(eng.cocoop_gen_ctx(image, aug=True)[0])
        prompts = self.prompt_generator(img, ctx_only=True)
        return torch.cat([eng.logits(img[i:i + 1], eng.text_features(prompts[i])) for i in range(img.shape[0])])

    def forward(self, input):
        if isinstance(input, tuple):
            image_features, ctx = input
            return self.forward_ctx(image_features, ctx)
        return self.inference(input)


def get_cocoop(clip_arch, test_set, device, n_ctx, classnames: Optional[List[str]] = None):
    """TPT/clip/cocoop.py:226-234.  The reference picks the class-name list from its data package by `test_set`; here the caller
    passes it (default: a placeholder until prompt_generator.reset_classnames)."""
    if classnames is None:
        classnames = ["c0"]
    return CoCoOpCLIP(device, classnames, arch=clip_arch, n_ctx=n_ctx)


def load_cocoop_weights(path_or_state_dict, model: CoCoOpCLIP):
    """The CoCoOp part of load_model_weight (TPT/utils/tools.py:101-131): a checkpoint `{'state_dict': ...}` (or the state dict itself,
    or a path to either), without the fixed token vectors `token_prefix` / `token_suffix` (those follow the current class names), loaded
    into model.prompt_generator: `ctx` and the meta-net.  Keys may carry the `prompt_generator.` prefix of a whole-model checkpoint.
    Returns the keys that were loaded; the engine's copies follow at the next call into the mirror."""
    ckpt = torch.load(path_or_state_dict, map_location="cpu") if isinstance(path_or_state_dict, (str, bytes)) or hasattr(path_or_state_dict, "__fspath__") \
        else path_or_state_dict
    sd = dict(ckpt["state_dict"] if "state_dict" in ckpt else ckpt)
    sd = {(k[len("prompt_generator."):] if k.startswith("prompt_generator.") else k): v for k, v in sd.items()}
    for k in ("token_prefix", "token_suffix"):
        sd.pop(k, None)
    own = model.prompt_generator.state_dict()
    sd = {k: v for k, v in sd.items() if k in own}
    model.prompt_generator.load_state_dict(sd, strict=False)          # (as the reference's fallback, tools.py:125)
    model.prompt_generator.wrote()
    return sorted(sd)
