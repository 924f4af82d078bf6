"""Host-side mirror of the reference prompt-tuning model surface (TPT/clip/custom_clip.py):
`PromptLearner` (:76-289), `TextEncoder` (:53-73), `ClipTestTimeTuning` (:292-344), `get_coop`
(:347-361), `CLIPCLS_TTA` (:364-497), `CLIPCLS_TTA_Multiple` (:500-583).  Same names, argument meaning and error behaviour; every FLOP of the towers runs in
librlcf_hip.so (rlcf_amd.engine) — these classes hold parameters and bookkeeping only."""
from __future__ import annotations

from typing import List, Optional

import torch
import torch.nn as nn

from . import clip_store, runtime
from . import _lib as L


class _ResetTracker:
    """Host-side knowledge "these tunable tensors ARE the reset state right now" without a device round trip per test image.

    `Parameter._version` does not see edits made through `.data` (the idiom this mirror itself — and the reference — use), so the
    knowledge is kept explicitly: every mirror-side write goes through `wrote()` (a generation counter), `mark_reset()` records the
    generation and the versions at which the tensors were set to the reset state, and `at_reset()` holds only while neither moved.
    An edit that bypasses both (a foreign `p.data.copy_(...)` between reset() and test_time_tuning) cannot be seen from the host; it is
    caught on the DEVICE instead: whoever takes the fast path calls `guard(tensor, expected)`, an asynchronous comparison whose
    one-byte result is read at the NEXT entry point (long finished by then: no wait) and raises — a silent wrong result becomes a
    loud error one sample later."""

    def __init__(self):
        self.gen = 0
        self._reset_gen = -1
        self._reset_versions = None
        self._guards = []

    def wrote(self):
        self.gen += 1

    def mark_reset(self, *tensors):
        self.gen += 1
        self._reset_gen = self.gen
        self._reset_versions = tuple(None if t is None else t._version for t in tensors)

    def at_reset(self, *tensors) -> bool:
        return self._reset_gen == self.gen and self._reset_versions == tuple(None if t is None else t._version for t in tensors)

    def guard(self, tensor: torch.Tensor, expected: torch.Tensor, what: str):
        """queue `tensor == expected` on the device (no synchronisation); checked by check().  The one-byte result travels to a pinned
        host byte by an asynchronous copy with an event behind it, so that reading it later never makes the host wait for the device."""
        flag = (tensor.detach() != expected.detach()).any()
        if flag.is_cuda:
            host = torch.empty(1, dtype=torch.bool, pin_memory=True)
            host.copy_(flag.reshape(1), non_blocking=True)
            ev = torch.cuda.Event()
            ev.record()
            self._guards.append((host, what, ev))
        else:
            self._guards.append((flag.reshape(1), what, None))

    def check(self, wait: bool = False):
        """called at every entry point: reads the comparisons queued by EARLIER calls that have FINISHED (event query, no wait — round 5: a
        blocking read here made the host wait for the previous image's step at every image and cost the harness loop its host / device
        overlap: 76 -> 68 images/s with the views made in the loop); an unfinished one stays queued for the next entry point.  wait=True
        (end of an evaluation loop) drains the queue."""
        pending, self._guards = self._guards, []
        for host, what, ev in pending:
            if ev is not None and not wait and not ev.query():
                self._guards.append((host, what, ev))
                continue
            if ev is not None and wait:
                ev.synchronize()
            if bool(host[0]):
                raise RuntimeError(f"rlcf_amd mirror: {what} — the tensor was edited behind the mirror's back (through `.data` or a raw "
                                   "pointer) after the state an earlier call assumed; that call's result was computed from the "
                                   "unedited state.  Edit through the mirror (reset(), ctx_init_state = ..., in-place ops on the Parameter).")


class PromptLearner(nn.Module):
    """TPT/clip/custom_clip.py:76-289.  Holds the learnable context `ctx` [n_ctx, W], its pristine copy
    `ctx_init_state`, and `tokenized_prompts` int64 [C, 77] of "<prefix> <class>."."""

    def __init__(self, clip_model, classnames, batch_size=None, n_ctx=16, ctx_init=None, ctx_position="end",
                 learned_cls=False):
        super().__init__()
        if batch_size is not None or learned_cls:
            raise NotImplementedError("batch-wise ctx and learned_cls are not built (never set by TPT/scripts/rlcf-*.sh)")
        if ctx_position not in ("end", "middle", "front"):
            raise ValueError(ctx_position)
        self.clip_model = clip_model
        self.learned_cls, self.batch_size, self.class_token_position = learned_cls, batch_size, ctx_position
        sd = clip_model.state_dict
        self.device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.ctx_dim = sd["ln_final.weight"].shape[0]
        self.dtype = torch.float32
        if ctx_init:                                   # custom_clip.py:90-107
            ctx_init = ctx_init.replace("_", " ")
            if "[CLS]" in ctx_init:                    # custom_clip.py:92-97: the class tokens go where [CLS] stands
                self.split_idx = ctx_init.split(" ").index("[CLS]")
                ctx_init = ctx_init.replace("[CLS] ", "")
                self.class_token_position = "middle"
            else:
                self.split_idx = None
            n_ctx = len(ctx_init.split(" "))
            prompt = clip_store.tokenize(ctx_init)
            ctx_vectors = sd["token_embedding.weight"][prompt[0, 1:1 + n_ctx].to(sd["token_embedding.weight"].device)].float()
            prompt_prefix = ctx_init
        else:                                          # custom_clip.py:108-112
            self.split_idx = None
            ctx_vectors = torch.empty(n_ctx, self.ctx_dim)
            nn.init.normal_(ctx_vectors, std=0.02)
            prompt_prefix = " ".join(["X"] * n_ctx)
        self.prompt_prefix, self.n_ctx, self.ctx_init = prompt_prefix, n_ctx, ctx_init
        ctx_vectors = ctx_vectors.detach().to(self.device).clone()
        self.tokenized_prompts = None
        self._track = _ResetTracker()
        self._ctx_init_state = ctx_vectors.detach().clone()
        self.ctx = nn.Parameter(ctx_vectors)
        self._set_classnames(classnames)

    @property
    def ctx_init_state(self) -> torch.Tensor:
        return self._ctx_init_state

    @ctx_init_state.setter
    def ctx_init_state(self, value: torch.Tensor) -> None:
        """The harness assigns a pre-trained (CoOp) prompt here (`--load`, tpt_cls_rl.py:95-101): the engine's reset state and
        its cached step-0 text features follow."""
        self._ctx_init_state = value.detach().to(self.device, torch.float32).clone()
        self._track.wrote()                               # (the reset state itself moved: reset() establishes it again)
        if self.tokenized_prompts is not None:
            self._publish_bank()

    def _set_classnames(self, classnames: List[str]) -> None:
        classnames = [name.replace("_", " ") for name in classnames]
        prompts = [self.prompt_prefix + " " + name + "." for name in classnames]
        self.tokenized_prompts = clip_store.tokenize(prompts).to(self.device)      # custom_clip.py:154
        self.n_cls, self.classnames = len(classnames), classnames
        # name_lens (custom_clip.py:127): tokens between the context words and the final '.', read off the tokenised prompt ...
        eot = self.tokenized_prompts.argmax(dim=-1)
        self.name_lens = [int(e) - 1 - self.n_ctx - 1 for e in eot]
        # ... and, when the installed tokenizer is a BPE with an `encode` (rlcf_amd.bpe.ClipBPE, the reference's SimpleTokenizer), as the
        # reference counts them: len(_tokenizer.encode(name)).  The two differ when BPE merges the trailing '.' into the name ("St.") or
        # a prompt is truncated at 77 tokens; the bare-name count is what places the class rows in the 'front' / 'middle' layouts.
        enc = getattr(getattr(clip_store._TOKENIZER, "__self__", None), "encode", None)
        if callable(enc):
            self.name_lens = [len(enc(name)) for name in classnames]
        self._publish_bank()

    def _arrangement(self):
        """-> (student_tokens [C, L], ctx_pos [C, n_ctx]) for class_token_position 'front' / 'middle' (custom_clip.py:239-284): the
        token ids in the order PromptLearner.forward concatenates the pieces, and where each learnable vector lands; None for 'end'."""
        if self.class_token_position == "end":
            return None, None
        tok = self.tokenized_prompts.cpu()
        C, n = tok.shape[0], self.n_ctx
        half = (self.split_idx if self.split_idx is not None else n // 2) if self.class_token_position == "middle" else 0
        stok, pos = tok.clone(), torch.zeros(C, n, dtype=torch.int64)
        for i in range(C):
            nl = self.name_lens[i]
            cls_ids = tok[i, 1 + n: 1 + n + nl]
            stok[i, 1 + half: 1 + half + nl] = cls_ids                       # [SOS | ctx[:half] | class | ctx[half:] | rest]
            stok[i, 1: 1 + half] = 0
            stok[i, 1 + half + nl: 1 + n + nl] = 0
            pos[i, :half] = torch.arange(1, 1 + half)
            pos[i, half:] = torch.arange(1 + half + nl, 1 + n + nl)
        return stok, pos

    def _publish_bank(self) -> None:
        stok, pos = self._arrangement()
        runtime.SESSION.set_bank(self.tokenized_prompts, self.n_ctx, self.ctx_init_state, stok, pos)

    def reset(self):                                   # custom_clip.py:161-167
        self.ctx.data.copy_(self.ctx_init_state)
        # (host-side note that ctx IS the reset state now — rlcf_amd.tpt_cls_rl.test_time_tuning then need not compare the two tensors,
        # which would make the host wait for the device once per test image; an in-place edit of the Parameter bumps its version)
        self._track.mark_reset(self.ctx)

    def reset_classnames(self, classnames, arch):      # custom_clip.py:169-196 (without re-loading CLIP from disk)
        self._track.wrote()
        self._set_classnames(classnames)

    def forward(self, init=None):
        """Materialised prompts [C, 77, W] = [SOS | ctx | class tokens . EOS pad] (custom_clip.py:198-238).
        The HIP text tower never needs this tensor; provided for API completeness."""
        ctx = init if init is not None else self.ctx
        table = self.clip_model.state_dict["token_embedding.weight"].to(ctx.device)
        stok, pos = self._arrangement()
        if stok is None:
            emb = table[self.tokenized_prompts]
            return torch.cat([emb[:, :1], ctx.unsqueeze(0).expand(self.n_cls, -1, -1), emb[:, 1 + self.n_ctx:]], dim=1)
        emb = table[stok.to(ctx.device)].clone()
        emb[torch.arange(self.n_cls)[:, None], pos.to(ctx.device)] = ctx.unsqueeze(0).expand(self.n_cls, -1, -1)
        return emb


class TextEncoder(nn.Module):
    """TPT/clip/custom_clip.py:53-73 — kept as a named sub-module; its arithmetic is rlcf_text_features."""

    def __init__(self, clip_model):
        super().__init__()
        self.clip_model = clip_model

    def forward(self, prompts, tokenized_prompts):
        raise NotImplementedError("call ClipTestTimeTuning.get_text_features(): the HIP text tower consumes ctx directly")


class _LogitsFn(torch.autograd.Function):
    """logits = exp(logit_scale) * norm(img) @ norm(txt(ctx))^T; image tower under no_grad
    (custom_clip.py:325-335).  backward = rlcf_text_backward_dense (what loss.backward() does at tpt_cls_rl.py:77)."""

    @staticmethod
    def forward(fn_ctx, ctx, images, model):
        eng = runtime.SESSION.engine(images.shape[0])
        img = eng.encode_image(L.STUDENT, images)
        txt = eng.text_features(ctx)
        fn_ctx.save_for_backward(ctx.detach().clone(), img)
        return eng.logits(img, txt)

    @staticmethod
    def backward(fn_ctx, dlogits):
        ctx, img = fn_ctx.saved_tensors
        eng = runtime.SESSION.engine(img.shape[0])
        return eng.text_backward_dense(ctx, img, dlogits.contiguous().float()), None, None


class ClipTestTimeTuning(nn.Module):
    """TPT/clip/custom_clip.py:292-344."""

    def __init__(self, device, classnames, batch_size, criterion="cosine", arch="ViT-L/14", n_ctx=16, ctx_init=None,
                 ctx_position="end", learned_cls=False):
        super().__init__()
        clip, _, _ = clip_store.load(arch, device=device)
        self.clip = clip
        runtime.SESSION.set_student(clip)
        self.text_encoder = TextEncoder(clip)
        self.logit_scale = clip.state_dict["logit_scale"].detach().clone()
        self.prompt_learner = PromptLearner(clip, classnames, batch_size, n_ctx, ctx_init, ctx_position, learned_cls)
        self.criterion = criterion

    @property
    def dtype(self):
        return torch.float32

    def reset(self):
        self._tuned_view_cache = None
        self.prompt_learner.reset()

    def reset_classnames(self, classnames, arch):
        self._tuned_view_cache = None
        self.prompt_learner.reset_classnames(classnames, arch)

    def get_text_features(self):
        return runtime.SESSION.engine().text_features(self.prompt_learner.ctx)

    def inference(self, image):
        pl = self.prompt_learner
        pl._track.check()
        cache = getattr(self, "_tuned_view_cache", None)
        if cache is not None and not torch.is_grad_enabled():
            view0, gen, version, ctx_after, logits, hint_key = cache
            # the clean view rlcf_amd.tpt_cls_rl.test_time_tuning just tuned on, with the prompt it left behind: the fused step already
            # computed these logits (same arithmetic: frozen image tower, text tower of the adapted prompt).  Valid only while the prompt is
            # the one that call wrote: every mirror-side write bumps the tracker's generation, in-place edits of the Parameter bump its
            # version, and an edit through `.data` is caught by the device-side guard below (loudly, at the next entry point).  The mirror's
            # own loop names the tensor it will ask about (same storage, shape, version: no device round trip); any other caller is
            # answered after comparing the contents (torch.equal: the host waits for the device once)
            if pl._track.gen == gen and pl.ctx._version == version and image.shape == view0.shape and image.device == view0.device:
                same = hint_key is not None and hint_key == (image.data_ptr(), tuple(image.shape), image._version)
                if same or torch.equal(image, view0):
                    pl._track.guard(pl.ctx.data, ctx_after, "the prompt changed between test_time_tuning and model(image)")
                    return logits.clone()
        return _LogitsFn.apply(pl.ctx, image, self)

    def forward(self, input):
        if isinstance(input, tuple) or input.dim() == 2:
            # the reference dispatches these to methods it never defines (custom_clip.py:338-342)
            raise AttributeError("contrast_prompt_tuning / directional_prompt_tuning are undefined in the reference")
        return self.inference(input)


def get_coop(clip_arch, test_set, device, n_ctx, ctx_init, learned_cls=False, classnames: Optional[List[str]] = None):
    """TPT/clip/custom_clip.py:347-361.  The reference picks class-name lists from its data package by
    `test_set`; here the caller passes them (default: placeholders until reset_classnames)."""
    if classnames is None:
        classnames = ["c0"]
    return ClipTestTimeTuning(device, classnames, None, arch=clip_arch, n_ctx=n_ctx, ctx_init=ctx_init, learned_cls=learned_cls)


class CLIPCLS_TTA(nn.Module):
    """TPT/clip/custom_clip.py:364-497 — CLIP classification with test-time adaptation of the image encoder.
    only_norm=True (BASELINE configs[2], the `--tune_norm 1` setting): the tunable set is every
    visual LayerNorm weight/bias and `parameters()` returns ONE flat tensor holding them in named_parameters order
    ([ln_pre.w, ln_pre.b, (ln_1.w, ln_1.b, ln_2.w, ln_2.b) x layers, ln_post.w, ln_post.b]) instead of 4L+4 tensors.
    only_norm=False (the reference default, what scripts/rlcf-tune.sh runs): every visual parameter is tuned; `parameters()`
    returns that LayerNorm tensor plus ONE flat tensor with all other visual tensors (Engine.visual_layout())."""

    def __init__(self, device, classnames, arch="ViT-L/14", prompt_prefix=None, only_visual=True, momentum_update=False,
                 update_freq=256, update_w=1.0, momentum=0.9999, only_norm=False):
        super().__init__()
        # only_visual=False changes NOTHING the reference computes: parameters() returns clip_model.visual's tensors whatever only_visual is
        # (custom_clip.py:477-485), forward() reads the class features cached under no_grad (:405-409, :423-432), freeze_parameters only
        # skips a requires_grad_(False) on tensors no optimizer ever sees (:411-421), and reset_classnames_and_state re-reads the SAME
        # checkpoint for the class features (:442-447).  Verified against the reference itself: its runs with only_visual=False are
        # bit-identical to the committed only_visual=True fixtures (tests/golden/make_golden.py --only onlyvisual).  Accepted, same path.
        self.clip_model, _, _ = clip_store.load(arch, device=device)
        # a ModifiedResNet student (RN50 .. RN50x64): the norm layers are BatchNorms; `ln` then holds their weights / biases and the
        # forward runs them on batch statistics, as the reference's does even after model.eval() (custom_clip.py:481-497)
        self.resnet = "visual.layer1.0.conv1.weight" in self.clip_model.state_dict
        runtime.SESSION.set_student(self.clip_model)
        self.device, self.prompt_prefix = device, prompt_prefix
        self.only_visual, self.only_norm, self.momentum_update = only_visual, only_norm, momentum_update
        self.update_freq, self.update_w, self.momentum, self.update_counter = update_freq, update_w, momentum, 0
        self._ln = self._vis = None
        self._track = _ResetTracker()
        self._set_classnames(classnames)

    def _set_classnames(self, classnames):
        sd = self.clip_model.state_dict
        self.classnames = [name.replace("_", " ") for name in classnames]
        self.n_cls = len(classnames)
        prompts = [self.prompt_prefix + " " + name + "." for name in self.classnames]     # prefix used raw (custom_clip.py:377-380)
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.tokenized_prompts = clip_store.tokenize(prompts).to(dev)
        # the engine's "prompt" is the raw prefix: its first token after SOT, looked up in the embedding table, so the
        # cached text features are exactly encode_text(tokenized_prompts) (get_class_features, custom_clip.py:405-409)
        tok0 = self.tokenized_prompts[0]
        emb = sd["token_embedding.weight"]
        ctx = emb[tok0[1:2].to(emb.device)].float()
        runtime.SESSION.set_bank(self.tokenized_prompts, 1, ctx)

    @property
    def ln(self) -> nn.Parameter:
        if self._ln is None:
            eng = runtime.SESSION.engine()
            self._ln_init = eng.ln_params(pristine=True)
            self._ln = nn.Parameter(self._ln_init.clone())
        return self._ln

    @property
    def vis(self) -> nn.Parameter:
        """every non-LayerNorm visual parameter in one flat tensor (only_norm=False)"""
        if self._vis is None:
            eng = runtime.SESSION.engine()
            self._vis_init = eng.visual_params(1)
            self._vis = nn.Parameter(self._vis_init.clone())
        return self._vis

    def set_prior_strength(self, prior_strength: int):
        """`--prior_strength` of tune_cls_rl.py (:73-76 swaps nn.BatchNorm2d.forward for `_modified_bn_forward` when >= 0); ResNet students only."""
        if self.resnet:
            runtime.SESSION.set_bn_prior_strength(prior_strength)

    def parameters(self, recurse: bool = True):            # custom_clip.py:477-485
        return [self.ln] if self.only_norm else [self.ln, self.vis]

    @torch.no_grad()
    def reset(self):                                       # custom_clip.py:456-458
        self.ln.data.copy_(self._ln_init)
        if not self.only_norm:
            self.vis.data.copy_(self._vis_init)
        # (host-side note that the tunable tensors ARE the reset state: rlcf_amd.tpt_cls_rl.test_time_tuning then skips its tensor
        # comparisons — one host-device round trip per test image; in-place edits of the Parameters bump the stamped versions)
        self._track.mark_reset(self.ln, None if self.only_norm else self.vis)

    @torch.no_grad()
    def reset_classnames_and_state(self, classnames, arch):   # custom_clip.py:434-454
        """New class bank AND the visual state back to the checkpoint: visual.load_state_dict(clip_state_dict), then
        initial_state_dict / momentum_state_dict re-initialised from it (:449-454) — the EMA of one dataset does not leak into the next."""
        self._set_classnames(classnames)
        eng = runtime.SESSION.engine()
        eng.reset_visual_state()
        if self._ln is not None:
            self._ln_init = eng.ln_params(pristine=True)
        if self._vis is not None:
            self._vis_init = eng.visual_params(1)
        if self._ln is not None:
            self.reset()

    @torch.no_grad()
    def momentum_update_model(self):                       # custom_clip.py:460-475
        """EMA of the tuned LayerNorm parameters over test samples; every update_freq samples the reset state becomes
        (1-update_w)*checkpoint + update_w*EMA.  (The frozen tensors of the visual state dict are fixed points of the EMA.)
        Samples become order-dependent: run on one replica."""
        if not self.momentum_update:
            return
        if self.resnet and not self.only_norm:
            # the reference EMAs the WHOLE visual state dict — BatchNorm running_mean / running_var included (custom_clip.py:460-475) — and
            # in this mode the clean-view inference runs the BatchNorms in eval form on those statistics: the engine's EMA covers the
            # parameters only, so the combination is refused rather than left to drift from the reference after update_freq samples
            raise NotImplementedError("momentum_update with only_norm=False on a ModifiedResNet student: the EMA of the BatchNorm running "
                                      "statistics is not built (use only_norm=True, or momentum_update=False)")
        self.update_counter += 1
        apply = self.update_counter >= self.update_freq
        if apply:
            self.update_counter = 0
        eng = runtime.SESSION.engine()
        eng.momentum_update(self.ln.data, self.momentum, self.update_w, apply)
        if not self.only_norm:
            eng.momentum_update_visual(self.vis.data, self.momentum, self.update_w, apply)
        if apply:
            self._ln_init = eng.ln_params(pristine=True)
            if not self.only_norm:
                self._vis_init = eng.visual_params(1)
            self._track.wrote()                              # (the reset state itself moved: reset() establishes it again)

    @torch.no_grad()
    def forward(self, image):
        """custom_clip.py:423-432 with the current LayerNorm parameters (inference only: the training-time forward and
        backward are fused inside rlcf_tta_sample_ln, called by rlcf_amd.tpt_cls_rl.test_time_tuning)."""
        eng = runtime.SESSION.engine(image.shape[0])
        eng.set_ln_params(self.ln.data)
        if self.resnet:
            # norm-layer tuning: CLIPCLS_TTA.train(mode) keeps the BatchNorms in train mode whatever `mode` is; every-parameter tuning:
            # train(mode) is plain nn.Module.train(mode) (custom_clip.py:487-497), so after model.eval() they run in eval form on the
            # running statistics the tuning passes left behind
            adapted = not self.only_norm and not torch.equal(self.vis.data, self._vis_init)
            if adapted:
                eng.set_visual_params(self.vis.data)
            img = eng.encode_image_bn(image, eval_form=(not self.only_norm) and not self.training)
            out = eng.logits(img, eng.text_features(runtime.SESSION.ctx_init.to(img.device)))
            eng.set_ln_params(self._ln_init)
            if adapted:
                eng.set_visual_params(self._vis_init)
            return out
        adapted = not self.only_norm and not torch.equal(self.vis.data, self._vis_init)
        if adapted:
            eng.set_visual_params(self.vis.data)
        img = eng.encode_image(L.STUDENT, image)
        out = eng.logits(img, eng.text_features(runtime.SESSION.ctx_init.to(img.device)))
        eng.set_ln_params(self._ln_init)
        if adapted:
            eng.set_visual_params(self._vis_init)
        return out


class CLIPCLS_TTA_Multiple(nn.Module):
    """TPT/clip/custom_clip.py:500-583 — the zero-shot ensemble: the mean over several CLIPs of their cosine logits.  "It is not used
    for training in this project" (:503): no tunable state, `freeze_parameters` / `reset` / `momentum_update_model` do nothing.
    arch[0] becomes the session's student and arch[1:] its further slots (runtime.SESSION.set_ensemble); `forward` is one
    rlcf_zero_shot_batch call.  At most rlcf_amd._lib.ENS_MAX_MODELS models."""

    def __init__(self, device, classnames, arch=["ViT-B/16", "ViT-L/14"], prompt_prefix=None, **kwargs):
        super().__init__()
        arch = list(arch)
        if len(arch) > L.ENS_MAX_MODELS:
            raise NotImplementedError(f"CLIPCLS_TTA_Multiple: {len(arch)} models; the engine mixes at most {L.ENS_MAX_MODELS} "
                                      "(a student and RLCF_MAX_REWARDS further slots)")
        if not arch:
            raise ValueError("CLIPCLS_TTA_Multiple needs at least one arch")
        self.clip_models = [clip_store.load(ar, device=device)[0] for ar in arch]
        self.resolutions = [c.geometry.image_resolution for c in self.clip_models]                # custom_clip.py:511
        self.n_model = len(self.clip_models)
        self.default_resolutions = kwargs["default_resolutions"] if "default_resolutions" in kwargs.keys() else 224
        runtime.SESSION.set_student(self.clip_models[0])
        runtime.SESSION.set_ensemble(self.clip_models[1:])
        self.device, self.prompt_prefix = device, prompt_prefix
        self.classnames = [name.replace("_", " ") for name in classnames]
        self.n_cls = len(classnames)
        self._class_features = None
        self._set_prompts(classnames)          # the RAW names: custom_clip.py:521 iterates `classnames`, not `self.classnames`

    def _set_prompts(self, names) -> None:
        prompts = [self.prompt_prefix + " " + name + "." for name in names]
        self._publish(clip_store.tokenize(prompts))

    def _publish(self, tokenized_prompts: torch.Tensor) -> None:
        dev = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.tokenized_prompts = tokenized_prompts.to(dev)
        # as CLIPCLS_TTA: the engine's one "learnable" row is the first prompt token, looked up in the student's embedding table, so the
        # student's cached text features are encode_text(tokenized_prompts); the further models read the tokens as they are
        emb = self.clip_models[0].state_dict["token_embedding.weight"]
        ctx = emb[self.tokenized_prompts[0][1:2].to(emb.device)].float()
        runtime.SESSION.set_bank(self.tokenized_prompts, 1, ctx)
        self._class_features = None

    def _engine(self, n_images: int = 1):
        return runtime.SESSION.engine(n_images)

    @property
    def class_features(self) -> List[torch.Tensor]:
        """[C, D_m] per model, L2-normalised (custom_clip.py:523): what the engine cached when it took the class bank"""
        if self._class_features is None:
            eng = self._engine()
            student = eng.text_features(runtime.SESSION.ctx_init.to(eng.device))
            self._class_features = [student] + [eng.reward_class_features(m) for m in range(self.n_model - 1)]
        return self._class_features

    @torch.no_grad()
    def get_class_features(self, tokenized_prompts):       # custom_clip.py:525-534
        """the models' class features of `tokenized_prompts`; prompts other than the current bank are published for the call and the
        bank is put back"""
        current = self.tokenized_prompts
        if tokenized_prompts.shape == current.shape and torch.equal(tokenized_prompts.to(current.device), current):
            return list(self.class_features)
        self._publish(tokenized_prompts)
        out = list(self.class_features)
        self._publish(current)
        return out

    @torch.no_grad()
    def extract_image_features(self, images):              # custom_clip.py:536-549
        """per model the L2-normalised image features [n, D_m] (the reference's docstring says "without normalization"; its code
        normalises, :546); a model whose resolution differs from the images' gets the bicubic align_corners=True resample (:541-544)"""
        eng = self._engine(images.shape[0])
        return [eng.encode_image(w, images) for w in range(self.n_model)]

    @torch.no_grad()
    def freeze_parameters(self):
        pass

    @torch.no_grad()
    def forward(self, image):                              # custom_clip.py:555-566
        eng = self._engine(image.shape[0])
        return eng.zero_shot_batch(image, ensemble=self.n_model > 1, want_top5=False)["logits"]

    @torch.no_grad()
    def reset_classnames_and_state(self, classnames, arch):    # custom_clip.py:568-575
        self.n_cls = len(classnames)
        classnames = [name.replace("_", " ") for name in classnames]
        self.classnames = classnames
        self._set_prompts(classnames)

    @torch.no_grad()
    def reset(self):
        pass

    @torch.no_grad()
    def momentum_update_model(self):
        pass
