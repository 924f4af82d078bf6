"""Numpy restatement of the CoCoOp prompt generator for the tests (TPT/clip/cocoop.py:52-56,118-127,179) and the seeded inputs of the
tests/golden/cocoop_ops.npz cases (tests/golden/make_cocoop_golden.py::op_inputs).  Test infrastructure only."""
from __future__ import annotations

import numpy as np

from rlcf_amd import synth
from tpt_ref import load_golden  # noqa: F401


def op_inputs(shape, seed):
    D, H, W, n_ctx, n = shape
    return dict(feats=synth.normal(seed, "op.feats", (n, D), 1.0), ctx=synth.normal(seed, "op.ctx", (n_ctx, W), 0.02),
                w1=synth.normal(seed, "op.w1", (H, D), D ** -0.5), b1=synth.normal(seed, "op.b1", (H,), 0.25),
                w2=synth.normal(seed, "op.w2", (W, H), 0.02 * H ** -0.5), b2=synth.normal(seed, "op.b2", (W,), 0.005))


def case_shape(name):
    """'[strided_]d128_h8_w128_c4_n3' -> (D, H, W, n_ctx, n)"""
    return tuple(int(p[1:]) for p in name.replace("strided_", "").split("_"))


def op_cases():
    """[(name, shape, inputs, fixture arrays)] of cocoop_ops.npz, and its meta"""
    z, meta = load_golden("cocoop_ops")
    out = []
    for c in meta["cases"].split(","):
        shape = case_shape(c)
        out.append((c, shape, op_inputs(shape, int(z[c + "_seed"])), {k: z[f"{c}_{k}"] for k in ("rows64", "mean64", "mean32", "keep")}))
    return out, meta


def meta_net_f64(x, mean=False):
    """ctx + (W2 relu(W1 f + b1) + b2)[:, None, :] in float64 -> [n or 1, n_ctx, W]"""
    a = {k: np.asarray(v, dtype=np.float64) for k, v in x.items()}
    f = a["feats"].mean(axis=0, keepdims=True) if mean else a["feats"]
    h = np.maximum(f @ a["w1"].T + a["b1"], 0.0)
    return a["ctx"][None] + (h @ a["w2"].T + a["b2"])[:, None, :]
