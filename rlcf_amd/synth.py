"""Seeded synthetic CLIP weights, views and class-token banks.

Everything here is produced by a counter-based integer hash evaluated with torch
int64 ops, so the same (seed, name, index) gives bit-identical fp32 values on the
CPU (this container, oracle + golden fixtures) and on the GPU box (HIP path) with
no dependence on torch's own generators.  Weight statistics follow
``CLIP.initialize_parameters`` (reference TPT/clip/model.py:299-326); the key
layout is the OpenAI state-dict layout accepted by ``build_model``
(TPT/clip/model.py:399-436, SURVEY.md §8 a-W).
"""
from __future__ import annotations

import math
import zlib
from dataclasses import dataclass
from typing import Dict, Optional, Tuple, Union

import torch

_M32 = 0xFFFFFFFF


@dataclass(frozen=True)
class ClipGeometry:
    """Constructor arguments of the reference ``CLIP`` class, same order
    (TPT/clip/model.py:244-257).  ``vision_layers`` is an int for a VisionTransformer image tower and a 4-tuple of
    block counts for a ModifiedResNet (then ``vision_patch_size`` is None), as in the reference (:262-270)."""
    embed_dim: int
    image_resolution: int
    vision_layers: Union[int, Tuple[int, int, int, int]]
    vision_width: int
    vision_patch_size: Optional[int]
    context_length: int
    vocab_size: int
    transformer_width: int
    transformer_heads: int
    transformer_layers: int

    @property
    def is_resnet(self) -> bool:
        return isinstance(self.vision_layers, (tuple, list))

    @property
    def vision_heads(self) -> int:
        return self.vision_width * 32 // 64 if self.is_resnet else self.vision_width // 64

    @property
    def grid(self) -> int:
        return self.image_resolution // (32 if self.is_resnet else self.vision_patch_size)

    @property
    def vision_tokens(self) -> int:
        return self.grid * self.grid + 1

    def as_tuple(self) -> Tuple[int, ...]:
        return (self.embed_dim, self.image_resolution, self.vision_layers, self.vision_width,
                self.vision_patch_size, self.context_length, self.vocab_size,
                self.transformer_width, self.transformer_heads, self.transformer_layers)


GEOMETRIES: Dict[str, ClipGeometry] = {
    # the OpenAI checkpoints the reference loads (TPT/clip/clip.py:30-40)
    "ViT-B/16": ClipGeometry(512, 224, 12, 768, 16, 77, 49408, 512, 8, 12),
    "ViT-B/32": ClipGeometry(512, 224, 12, 768, 32, 77, 49408, 512, 8, 12),
    "ViT-L/14": ClipGeometry(768, 224, 24, 1024, 14, 77, 49408, 768, 12, 12),
    "ViT-L/14@336px": ClipGeometry(768, 336, 24, 1024, 14, 77, 49408, 768, 12, 12),
    "RN50": ClipGeometry(1024, 224, (3, 4, 6, 3), 64, None, 77, 49408, 512, 8, 12),
    "RN101": ClipGeometry(512, 224, (3, 4, 23, 3), 64, None, 77, 49408, 512, 8, 12),
    "RN50x4": ClipGeometry(640, 288, (4, 6, 10, 6), 80, None, 77, 49408, 640, 10, 12),
    "RN50x16": ClipGeometry(768, 384, (6, 8, 18, 8), 96, None, 77, 49408, 768, 12, 12),
    "RN50x64": ClipGeometry(1024, 448, (3, 15, 36, 10), 128, None, 77, 49408, 1024, 16, 12),
    # reduced geometries for tests (head_dim stays 64 as in every CLIP)
    "tiny": ClipGeometry(128, 32, 2, 128, 8, 77, 1024, 128, 2, 2),
    "tiny-r": ClipGeometry(64, 32, 2, 128, 8, 77, 1024, 64, 1, 2),
    "tiny-r64": ClipGeometry(64, 64, 2, 128, 16, 77, 1024, 64, 1, 2),     # reward model at twice the view resolution (bicubic path)
    "tiny-p6": ClipGeometry(128, 30, 2, 128, 6, 77, 1024, 128, 2, 2),     # 3*6*6 = 108 patch columns: zero-padded to the GEMM's K granule like ViT-L/14's 588
    "small": ClipGeometry(256, 64, 4, 256, 16, 77, 4096, 256, 4, 4),
    # ModifiedResNet image towers (attention-pool width 32*width, head_dim 64): 64x64 input -> 2x2 map -> 5 pooled tokens
    "tiny-rn": ClipGeometry(64, 64, (1, 2, 1, 1), 16, None, 77, 1024, 64, 1, 2),
    "tiny-rn32": ClipGeometry(128, 32, (2, 1, 1, 1), 16, None, 77, 1024, 128, 2, 2),      # as a student: 32x32 views, 1x1 map
}


def _hash32(x: torch.Tensor) -> torch.Tensor:
    """lowbias32-style avalanche on int64 tensors holding 32-bit values."""
    x = x ^ (x >> 16)
    x = (x * 0x7FEB352D) & _M32
    x = x ^ (x >> 15)
    x = (x * 0x846CA68B) & _M32
    x = x ^ (x >> 16)
    return x


def _keys(seed: int, name: str) -> Tuple[int, int]:
    k1 = zlib.crc32(name.encode()) & _M32
    k2 = (zlib.crc32((name + "#").encode()) ^ (seed * 0x9E3779B1)) & _M32
    return k1, k2


def raw_u32(seed: int, name: str, n: int, lane: int, device="cpu") -> torch.Tensor:
    """n 32-bit words of stream (seed, name, lane) as int64."""
    k1, k2 = _keys(seed, name)
    c = torch.arange(n, dtype=torch.int64, device=device) * 4 + lane
    h = _hash32((c + k1 * 0x9E3779B1) & _M32)
    return _hash32(h ^ k2)


_IH_STD = math.sqrt(8.0 * (65536.0 ** 2 - 1.0) / 12.0)


def normal(seed: int, name: str, shape, std: float = 1.0, mean: float = 0.0,
           device="cpu") -> torch.Tensor:
    """Approximately normal fp32 tensor: Irwin-Hall sum of eight 16-bit uniforms,
    exact in integer arithmetic, then one fp64 scale and one fp32 rounding."""
    if str(device) == "meta":            # shapes only (loader tests of the 400-600 M parameter geometries)
        return torch.empty(*shape, dtype=torch.float32, device="meta")
    n = 1
    for s in shape:
        n *= int(s)
    z = _z64(seed, name, n, device)
    return (z * std + mean).to(torch.float32).reshape(*shape)


def _z64(seed: int, name: str, n: int, device="cpu") -> torch.Tensor:
    """the float64 standard scores behind ``normal`` (before its scale and fp32 rounding)"""
    acc = torch.zeros(n, dtype=torch.int64, device=device)
    for lane in range(4):
        w = raw_u32(seed, name, n, lane, device)
        acc += (w & 0xFFFF) + (w >> 16)
    return (acc.to(torch.float64) - 8 * 32767.5) / _IH_STD


def _u64(seed: int, name: str, n: int, lane: int = 0) -> torch.Tensor:
    """float64 uniforms in [0, 1) from the top 32 bits of stream (seed, name, lane), CPU (exact: a 32-bit integer over 2^32)"""
    return raw_u32(seed, name, n, lane).to(torch.float64) / 4294967296.0


def randint(seed: int, name: str, n: int, low: int, high: int, device="cpu") -> torch.Tensor:
    return low + raw_u32(seed, name, n, 0, device) % (high - low)


# --------------------------------------------------------------------------
# weights
# --------------------------------------------------------------------------

def _block(sd, seed, prefix, width, layers, attn_std, proj_std, fc_std, device):
    for i in range(layers):
        p = f"{prefix}.resblocks.{i}."
        sd[p + "attn.in_proj_weight"] = normal(seed, p + "in_w", (3 * width, width), attn_std, device=device)
        sd[p + "attn.in_proj_bias"] = normal(seed, p + "in_b", (3 * width,), 0.02, device=device)
        sd[p + "attn.out_proj.weight"] = normal(seed, p + "out_w", (width, width), proj_std, device=device)
        sd[p + "attn.out_proj.bias"] = normal(seed, p + "out_b", (width,), 0.02, device=device)
        sd[p + "ln_1.weight"] = normal(seed, p + "ln1_w", (width,), 0.1, 1.0, device=device)
        sd[p + "ln_1.bias"] = normal(seed, p + "ln1_b", (width,), 0.05, device=device)
        sd[p + "mlp.c_fc.weight"] = normal(seed, p + "fc_w", (4 * width, width), fc_std, device=device)
        sd[p + "mlp.c_fc.bias"] = normal(seed, p + "fc_b", (4 * width,), 0.02, device=device)
        sd[p + "mlp.c_proj.weight"] = normal(seed, p + "proj_w", (width, 4 * width), proj_std, device=device)
        sd[p + "mlp.c_proj.bias"] = normal(seed, p + "proj_b", (width,), 0.02, device=device)
        sd[p + "ln_2.weight"] = normal(seed, p + "ln2_w", (width,), 0.1, 1.0, device=device)
        sd[p + "ln_2.bias"] = normal(seed, p + "ln2_b", (width,), 0.05, device=device)


def make_state_dict(geo: ClipGeometry, seed: int, device="cpu",
                    logit_scale: float = math.log(100.0), profile: str = "init") -> Dict[str, torch.Tensor]:
    """fp32 state dict in the OpenAI CLIP key layout.  LayerNorm gains/biases and
    linear biases are non-trivial on purpose so every epilogue is exercised.
    ``logit_scale`` defaults to ln(100), the value of the released checkpoints
    (a random-init CLIP has ln(1/0.07)).
    ``profile``: "init" — init-scale Gaussians (every committed fixture depends on these bits); "trained" — the dynamic range of a
    released checkpoint (``_trained``; built on the CPU and then moved to ``device``)."""
    if profile == "trained":
        return {k: v.to(device) for k, v in _trained(geo, seed, logit_scale).items()}
    if profile != "init":
        raise ValueError(f"profile {profile!r}: 'init' or 'trained'")
    sd: Dict[str, torch.Tensor] = {}
    vw, tw = geo.vision_width, geo.transformer_width
    if geo.is_resnet:
        _resnet(sd, seed, geo, device)
        _text(sd, seed, geo, device, logit_scale)
        return sd
    ps = geo.vision_patch_size
    sc = vw ** -0.5
    sd["visual.conv1.weight"] = normal(seed, "v.conv1", (vw, 3, ps, ps), (3 * ps * ps) ** -0.5, device=device)
    sd["visual.class_embedding"] = normal(seed, "v.cls", (vw,), sc, device=device)
    sd["visual.positional_embedding"] = normal(seed, "v.pos", (geo.vision_tokens, vw), sc, device=device)
    sd["visual.ln_pre.weight"] = normal(seed, "v.lnpre_w", (vw,), 0.1, 1.0, device=device)
    sd["visual.ln_pre.bias"] = normal(seed, "v.lnpre_b", (vw,), 0.05, device=device)
    v_proj_std = (vw ** -0.5) * ((2 * geo.vision_layers) ** -0.5)
    _block(sd, seed, "visual.transformer", vw, geo.vision_layers, vw ** -0.5, v_proj_std,
           (2 * vw) ** -0.5, device)
    sd["visual.ln_post.weight"] = normal(seed, "v.lnpost_w", (vw,), 0.1, 1.0, device=device)
    sd["visual.ln_post.bias"] = normal(seed, "v.lnpost_b", (vw,), 0.05, device=device)
    sd["visual.proj"] = normal(seed, "v.proj", (vw, geo.embed_dim), sc, device=device)
    _text(sd, seed, geo, device, logit_scale)
    return sd


# --------------------------------------------------------------------------
# "trained" profile: the dynamic range of released CLIP weights
# --------------------------------------------------------------------------

N_MASSIVE = 3             # residual channels that carry "massive activations" (c_proj bias of +-100..300 in the first half of the blocks)
QUIET_GAIN = 2.0 ** -7    # the last block's ln_2 gains and biases are scaled by this: rows of c_fc's operand below 2^-3
LOUD_QK = 1.5             # the Q and K rows of head 0 of the first and last block are scaled by this: attention logits in the tens


def massive_dims(seed: int, width: int) -> Tuple[int, ...]:
    """the N_MASSIVE fixed residual channels of a tower of this width"""
    out = []
    for v in raw_u32(seed, "tr.massive", 64, 0).tolist():
        if v % width not in out:
            out.append(v % width)
        if len(out) == N_MASSIVE:
            return tuple(out)
    raise AssertionError("unreachable")


def _student_t(seed: int, name: str, shape, std: float) -> torch.Tensor:
    """Student-t with nu = 3 scaled to standard deviation ``std``: z / sqrt(chi2_3 / 3) from four synth normal streams (chi2 gets a
    floor of 0.03 so that a draw of exactly zero cannot divide by zero: |t| <= 49)."""
    n = 1
    for d in shape:
        n *= int(d)
    z = _z64(seed, name + "/t0", n)
    chi = _z64(seed, name + "/t1", n) ** 2 + _z64(seed, name + "/t2", n) ** 2 + _z64(seed, name + "/t3", n) ** 2 + 0.03
    t = z / torch.sqrt(chi / 3.0)
    return (t * (std / math.sqrt(3.0))).to(torch.float32).reshape(*shape)


def _pick(seed: int, name: str, width: int, n: int, avoid) -> list:
    out = []
    for v in raw_u32(seed, name + "/pick", 4 * n + 64, 0).tolist():
        c = v % width
        if c not in out and c not in avoid:
            out.append(c)
        if len(out) == n:
            return out
    raise AssertionError("unreachable")


def _gain(seed: int, name: str, width: int, massive) -> torch.Tensor:
    """LayerNorm gains: power of two times a uniform mantissa in [1, 2).  15 of 16 channels in [0.5, 2), one of 16
    log-uniform over 2^-6 .. 2^5 (clamped to [0.02, 30]); two channels at each end of [0.02, 30] and two exact zeros."""
    r = raw_u32(seed, name + "/e", width, 0)
    tail = (r % 16) == 0
    e = torch.where(tail, (r >> 3) % 11 - 6, (r >> 3) % 2 - 1)
    g = torch.ldexp(1.0 + _u64(seed, name + "/m", width), e).clamp(0.02, 30.0)
    lo1, lo2, hi1, hi2, z1, z2 = _pick(seed, name, width, 6, massive)
    g[lo1], g[lo2], g[hi1], g[hi2], g[z1], g[z2] = 0.02, 0.021, 30.0, 29.0, 0.0, 0.0
    for j, d in enumerate(massive):                        # the blocks' LayerNorms damp the massive channels (ln_pre lifts them)
        g[d] = 0.0625 * (1.0 + float(_u64(seed, name + "/massive", len(massive))[j]))
    return g.to(torch.float32)


def _bias(seed: int, name: str, n: int, std: float, one_in: int) -> torch.Tensor:
    """N(0, std) plus, on one entry in ``one_in``, a uniform offset in (-5, 5)"""
    b = _z64(seed, name + "/b", n) * std
    r = raw_u32(seed, name + "/s", n, 0)
    big = (r % one_in) == 0
    return torch.where(big, b + (_u64(seed, name + "/u", n) * 10.0 - 5.0), b).to(torch.float32)


def _trained_tower(sd, seed, prefix, width, layers, proj_std, massive):
    heads = width // 64
    for i in range(layers):
        p = f"{prefix}.resblocks.{i}."
        w_in = _student_t(seed, p + "in_w", (3 * width, width), width ** -0.5)
        if i in (0, layers - 1):                               # one loud head: q.k / 8 in the tens
            w_in[0:64] *= LOUD_QK
            w_in[width:width + 64] *= LOUD_QK
        sd[p + "attn.in_proj_weight"] = w_in
        sd[p + "attn.in_proj_bias"] = _bias(seed, p + "in_b", 3 * width, 0.02, 32)
        sd[p + "attn.out_proj.weight"] = _student_t(seed, p + "out_w", (width, width), proj_std)
        sd[p + "attn.out_proj.bias"] = _bias(seed, p + "out_b", width, 0.02, 32)
        sd[p + "mlp.c_fc.weight"] = _student_t(seed, p + "fc_w", (4 * width, width), (2 * width) ** -0.5)
        sd[p + "mlp.c_fc.bias"] = _bias(seed, p + "fc_b", 4 * width, 0.02, 32)
        sd[p + "mlp.c_proj.weight"] = _student_t(seed, p + "proj_w", (width, 4 * width), proj_std)
        cb = _bias(seed, p + "proj_b", width, 0.02, 32)
        if i < max(1, layers // 2):                            # massive activations: +-100..300 on fixed residual channels
            u = _u64(seed, p + "proj_b/massive", len(massive))
            for j, d in enumerate(massive):
                cb[d] = (1.0 if j % 2 == 0 else -1.0) * (100.0 + 200.0 * float(u[j]))
        sd[p + "mlp.c_proj.bias"] = cb
        for ln in ("ln_1", "ln_2"):
            g = _gain(seed, p + ln + "_w", width, massive)
            b = _bias(seed, p + ln + "_b", width, 0.05, 16)
            if ln == "ln_2" and i == layers - 1:               # a quiet LayerNorm: its rows leave below 2^-3
                bulk = torch.ldexp(1.0 + _u64(seed, p + "ln2_w/q", width), -(raw_u32(seed, p + "ln2_w/q", width, 1) % 2))
                bulk[list(massive)] *= 0.0625
                g, b = (bulk * QUIET_GAIN).to(torch.float32), (b.double() * QUIET_GAIN).to(torch.float32)
            sd[p + ln + ".weight"], sd[p + ln + ".bias"] = g, b


def _trained(geo: ClipGeometry, seed: int, logit_scale: float) -> Dict[str, torch.Tensor]:
    """The "trained" profile: released CLIP weights are far from init scale, and the kernels' number formats are chosen for O(1) data
    (split-f16 operands, one-pass row statistics, exp / rcp fast forms).  This profile reproduces the dynamic range of a trained
    ViT + text transformer on the seeded generator, deterministic from (seed, name):
      * Linear / in_proj / out_proj / projection / patch-embedding weights: Student-t (nu = 3) at the init standard deviation;
      * LayerNorm gains: power of two times a uniform mantissa, one channel in 16 log-uniform over [0.02, 30], two channels at each
        end of that range, two exact zeros, 0.0625..0.125 on the massive channels (ln_pre: 24..30); biases N(0, 0.05) with one entry in 16 offset by up to +-5
        (ln_post / ln_final: N(0, 0.05) alone); Linear biases likewise (1 in 32);
      * massive activations: the c_proj bias of the first half of every tower's blocks is +-100..300 on ``massive_dims`` (ln_pre gains
        of 24..30 on the same channels);
      * attention: head 0 of the first and last block has its Q and K rows scaled by LOUD_QK (logits in the tens);
      * the last block's ln_2 is quiet (gains and bias times QUIET_GAIN): c_fc operand rows below 2^-3;
      * class / positional / token embeddings at 4x (text positional 5x) the init standard deviation; logit_scale as given (ln 100).
    Built on the CPU in float64 (integer hashes; +, -, *, /, sqrt, exact ldexp) and rounded once to fp32; make_state_dict moves it to
    the device, so CPU and GPU tests see the same bits.  ModifiedResNet image towers are out of scope (their activations already go
    through the device-side dynamic scale of the split-f16 GEMM): such geometries raise."""
    if geo.is_resnet:
        raise ValueError("the trained profile covers VisionTransformer image towers and text towers only")
    sd = make_state_dict(geo, seed, "cpu", logit_scale)
    vw, tw, ps = geo.vision_width, geo.transformer_width, geo.vision_patch_size
    sc = vw ** -0.5
    vm = massive_dims(seed, vw)
    sd["visual.conv1.weight"] = _student_t(seed, "v.conv1", (vw, 3, ps, ps), (3 * ps * ps) ** -0.5)
    sd["visual.class_embedding"] = normal(seed, "v.cls", (vw,), 4 * sc)
    sd["visual.positional_embedding"] = normal(seed, "v.pos", (geo.vision_tokens, vw), 4 * sc)
    g = _gain(seed, "v.lnpre_w", vw, vm)
    for j, d in enumerate(vm):
        g[d] = 24.0 + 6.0 * float(_u64(seed, "v.lnpre_w/massive", len(vm))[j])
    sd["visual.ln_pre.weight"], sd["visual.ln_pre.bias"] = g, _bias(seed, "v.lnpre_b", vw, 0.05, 16)
    _trained_tower(sd, seed, "visual.transformer", vw, geo.vision_layers, sc * (2 * geo.vision_layers) ** -0.5, vm)
    sd["visual.ln_post.weight"] = _gain(seed, "v.lnpost_w", vw, vm)       # (ln_post / ln_final biases keep init scale: a +-5 entry there
    sd["visual.ln_post.bias"] = normal(seed, "v.lnpost_b", (vw,), 0.05)     # would be one constant direction of every feature)
    sd["visual.proj"] = _student_t(seed, "v.proj", (vw, geo.embed_dim), sc)
    tm = massive_dims(seed, tw)
    sd["token_embedding.weight"] = normal(seed, "t.tok", (geo.vocab_size, tw), 0.08)
    sd["positional_embedding"] = normal(seed, "t.pos", (geo.context_length, tw), 0.05)
    _trained_tower(sd, seed, "transformer", tw, geo.transformer_layers, (tw ** -0.5) * (2 * geo.transformer_layers) ** -0.5, tm)
    sd["ln_final.weight"], sd["ln_final.bias"] = _gain(seed, "t.lnf_w", tw, tm), normal(seed, "t.lnf_b", (tw,), 0.05)
    sd["text_projection"] = _student_t(seed, "t.proj", (tw, geo.embed_dim), tw ** -0.5)
    return sd


def to_fp16_grid(sd: Dict[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """The state dict with the tensors a RELEASED CLIP checkpoint stores as fp16 rounded to fp16 values (still float32 tensors): what
    the reference actually holds after `clip.load` — the archives carry the weights of every Conv / Linear / MultiheadAttention and the
    two projections as fp16 (convert_weights, TPT/clip/model.py:375-396, applied before they were saved), and build_model copies them
    into float32 parameters (model.py:399-436, the re-conversion at :435 commented out).  LayerNorm parameters, embeddings and
    logit_scale stay as they are.  The engine recognises such weights at finalize (their split-f16 lo halves are zero) and drops the
    a_hi . w_lo pass of their products — bit for bit the same results in two MFMA passes instead of three."""
    out = {}
    for k, v in sd.items():
        grid = v.is_floating_point() and (
            k.endswith(("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias", "c_fc.weight", "c_fc.bias", "c_proj.weight",
                        "c_proj.bias", "conv1.weight", "conv2.weight", "conv3.weight", "q_proj.weight", "k_proj.weight", "v_proj.weight",
                        "q_proj.bias", "k_proj.bias", "v_proj.bias", "downsample.0.weight"))
            or k in ("visual.proj", "text_projection") or (k.startswith("visual.attnpool.") and k.endswith((".weight", ".bias")) and "positional" not in k))
        out[k] = v.half().float() if grid else v
    return out


def _bn(sd, seed, key, ch, device, gain=1.0):
    """BatchNorm2d buffers and affine in eval form: non-trivial running statistics so that the folding is exercised."""
    sd[key + ".weight"] = normal(seed, key + ".w", (ch,), 0.1, gain, device=device)
    sd[key + ".bias"] = normal(seed, key + ".b", (ch,), 0.05, device=device)
    sd[key + ".running_mean"] = normal(seed, key + ".rm", (ch,), 0.1, device=device)
    sd[key + ".running_var"] = 1.0 + 0.3 * torch.tanh(normal(seed, key + ".rv", (ch,), 1.0, device=device))
    sd[key + ".num_batches_tracked"] = torch.tensor(0, dtype=torch.int64, device=device)


def _conv(sd, seed, key, cout, cin, k, device):
    sd[key + ".weight"] = normal(seed, key, (cout, cin, k, k), (2.0 / (cin * k * k)) ** 0.5, device=device)


def _resnet(sd, seed, geo, device):
    """ModifiedResNet key layout (TPT/clip/model.py:94-154): 3-conv stem, four stages of Bottlenecks (expansion 4, the first
    block of a stage carries the downsample branch), AttentionPool2d."""
    w = geo.vision_width
    _conv(sd, seed, "visual.conv1", w // 2, 3, 3, device);      _bn(sd, seed, "visual.bn1", w // 2, device)
    _conv(sd, seed, "visual.conv2", w // 2, w // 2, 3, device); _bn(sd, seed, "visual.bn2", w // 2, device)
    _conv(sd, seed, "visual.conv3", w, w // 2, 3, device);      _bn(sd, seed, "visual.bn3", w, device)
    inpl = w
    for li, (nb, mult) in enumerate(zip(geo.vision_layers, (1, 2, 4, 8)), start=1):
        planes = w * mult
        for b in range(nb):
            p = f"visual.layer{li}.{b}."
            stride = 2 if (b == 0 and li > 1) else 1
            _conv(sd, seed, p + "conv1", planes, inpl, 1, device);       _bn(sd, seed, p + "bn1", planes, device)
            _conv(sd, seed, p + "conv2", planes, planes, 3, device);     _bn(sd, seed, p + "bn2", planes, device)
            _conv(sd, seed, p + "conv3", planes * 4, planes, 1, device); _bn(sd, seed, p + "bn3", planes * 4, device, gain=0.5)
            if stride > 1 or inpl != planes * 4:
                _conv(sd, seed, p + "downsample.0", planes * 4, inpl, 1, device)
                _bn(sd, seed, p + "downsample.1", planes * 4, device)
            inpl = planes * 4
    e = w * 32
    hw = geo.image_resolution // 32
    sd["visual.attnpool.positional_embedding"] = normal(seed, "v.ap.pos", (hw * hw + 1, e), e ** -0.5, device=device)
    for nm, od in (("q_proj", e), ("k_proj", e), ("v_proj", e), ("c_proj", geo.embed_dim)):
        sd[f"visual.attnpool.{nm}.weight"] = normal(seed, "v.ap." + nm, (od, e), e ** -0.5, device=device)
        sd[f"visual.attnpool.{nm}.bias"] = normal(seed, "v.ap.b." + nm, (od,), 0.02, device=device)


def _text(sd, seed, geo, device, logit_scale):
    tw = geo.transformer_width
    sd["token_embedding.weight"] = normal(seed, "t.tok", (geo.vocab_size, tw), 0.02, device=device)
    sd["positional_embedding"] = normal(seed, "t.pos", (geo.context_length, tw), 0.01, device=device)
    t_proj_std = (tw ** -0.5) * ((2 * geo.transformer_layers) ** -0.5)
    _block(sd, seed, "transformer", tw, geo.transformer_layers, tw ** -0.5, t_proj_std,
           (2 * tw) ** -0.5, device)
    sd["ln_final.weight"] = normal(seed, "t.lnf_w", (tw,), 0.1, 1.0, device=device)
    sd["ln_final.bias"] = normal(seed, "t.lnf_b", (tw,), 0.05, device=device)
    sd["text_projection"] = normal(seed, "t.proj", (tw, geo.embed_dim), tw ** -0.5, device=device)
    sd["logit_scale"] = torch.tensor(logit_scale, dtype=torch.float32, device=device)
    return sd


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------

def make_views(seed: int, n_views: int, resolution: int, device="cpu") -> torch.Tensor:
    """[N,3,R,R] fp32 N(0,1): post-``Normalize`` statistics of the reference loader
    (TPT/tpt_cls_rl.py:132-133).  View 0 plays the clean centre crop."""
    return normal(seed, "views", (n_views, 3, resolution, resolution), device=device)


# name-length pmf chosen to reproduce the ImageNet prompt statistics measured in
# SURVEY.md §0 fact 4 (total length min 8 / mean 9.16 / max 18 with n_ctx = 4)
_NAME_LEN_PMF = ((1, 420), (2, 300), (3, 140), (4, 70), (5, 30), (6, 20), (7, 10), (8, 5), (9, 3), (11, 2))


def make_token_bank(geo: ClipGeometry, n_cls: int, seed: int = 7, n_ctx: int = 4,
                    ctx_token_ids: Optional[Tuple[int, ...]] = None) -> torch.Tensor:
    """int64 [C, context_length] rows ``[SOT, ctx.., name.., '.', EOT, 0..]`` in the
    format ``clip.tokenize`` produces (TPT/clip/clip.py:197-233).  EOT is the
    largest id of the vocabulary, as ``argmax`` EOT lookup requires
    (TPT/clip/custom_clip.py:71)."""
    sot, eot = geo.vocab_size - 2, geo.vocab_size - 1
    if ctx_token_ids is None:
        ctx_token_ids = ctx_token_ids_default(geo, n_ctx)
    assert len(ctx_token_ids) == n_ctx
    dot = 269 % (geo.vocab_size - 2)
    cum, tot = [], 0
    for ln, w in _NAME_LEN_PMF:
        tot += w
        cum.append((tot, ln))
    u = raw_u32(seed, "bank.len", n_cls, 0) % tot
    toks = torch.zeros(n_cls, geo.context_length, dtype=torch.int64)
    ids = raw_u32(seed, "bank.ids", n_cls * 16, 1).reshape(n_cls, 16) % (geo.vocab_size - 2)
    for c in range(n_cls):
        ln = next(l for t, l in cum if int(u[c]) < t)
        if c == n_cls - 1 and n_cls >= 100:
            ln = 11
        row = [sot, *ctx_token_ids, *ids[c, :ln].tolist(), dot, eot]
        toks[c, :len(row)] = torch.tensor(row, dtype=torch.int64)
    return toks


def ctx_token_ids_default(geo: ClipGeometry, n_ctx: int) -> Tuple[int, ...]:
    """ids of the hand-crafted context words; (320,1125,539,320) is
    'a photo of a' under the CLIP BPE."""
    base = (320, 1125, 539, 320)
    out = tuple(base[i % 4] % (geo.vocab_size - 2) for i in range(n_ctx))
    return out


def reward_members(spec: str, seeds, device=None) -> list:
    """'geoA+geoB+...' and '23+29+...' (or a list of ints) -> [(geometry, state dict), ...]: the members of a reward ensemble
    (device: where the weights are generated — the generator is bit-identical on CPU and GPU up to the last bit of BatchNorm statistics)."""
    names = spec.split("+")
    seeds = [int(x) for x in seeds.split("+")] if isinstance(seeds, str) else list(seeds)
    kw = {} if device is None else {"device": device}
    return [(GEOMETRIES[n], make_state_dict(GEOMETRIES[n], seed=s, **kw)) for n, s in zip(names, seeds)]


def make_cocoop_state(geo: ClipGeometry, seed: int, n_ctx: int = 4, shift_std: float = 0.02) -> Dict[str, torch.Tensor]:
    """Seeded stand-in for a trained CoCoOp checkpoint (TPT/clip/cocoop.py:51-56) in the key layout of CoCoOpPromptLearner.state_dict():
    `ctx` [n_ctx, W] and the meta-net Linear(D, D // 16) -> ReLU -> Linear(D // 16, W).  Scaled so that the meta-net matters: linear1
    keeps un-normalised image features (|f| ~ sqrt(D) on these synthetic towers) at O(1) pre-activations of both signs, linear2 turns
    them into a shift of about `shift_std` per element — the size of a token embedding, i.e. of ctx itself."""
    D, W, H = geo.embed_dim, geo.transformer_width, geo.embed_dim // 16
    return {
        "ctx": normal(seed, "cocoop.ctx", (n_ctx, W), 0.02),
        "meta_net.linear1.weight": normal(seed, "cocoop.w1", (H, D), D ** -0.5),
        "meta_net.linear1.bias": normal(seed, "cocoop.b1", (H,), 0.25),
        "meta_net.linear2.weight": normal(seed, "cocoop.w2", (W, H), shift_std * H ** -0.5),
        "meta_net.linear2.bias": normal(seed, "cocoop.b2", (W,), 0.25 * shift_std),
    }
