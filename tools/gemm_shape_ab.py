#!/usr/bin/env python
"""Op-level A/B of two (or more) builds of librlcf_hip.so on the split-f16 products of the flagship workload, in ONE process.

    python tools/gemm_shape_ab.py --lib mfma16=rlcf_amd/librlcf_hip.so --lib mfma32=rlcf_amd/librlcf_hip_mfma32.so

Shapes: the four products of a ViT-B/16 layer at M = 403 456 (32 images x 64 views x 197 tokens) and the products of a text layer
at M = 131 040 (width 512), random data, interleaved operand pairs, the epilogue each product has in the tower (pairs out /
residual / QuickGELU -> pairs).  Per shape: >= --settle seconds of back-to-back launches alternating the arms (the chip reaches the
clock it holds under load), then --reps timed launches per arm, alternating A/B/A/B, each timed with its own event pair.
Prints microseconds (median) and TF (2 M N K, the logical product) per shape and arm."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from rlcf_amd import _lib as L, synth  # noqa: E402

LAYER = [("in_proj", 2304, 768, 0, False, True), ("out_proj", 768, 768, 0, True, False), ("c_fc", 3072, 768, 1, False, True),
         ("c_proj", 768, 3072, 0, True, False)]
TEXT = [("t.in_proj", 1536, 512, 0, False, False), ("t.out_proj", 512, 512, 0, True, False), ("t.c_fc", 2048, 512, 1, False, True),
        ("t.c_proj", 512, 2048, 0, True, False)]


def load(path):
    h = C.CDLL(os.path.abspath(path))
    for name in ("rlcf_gemm_f16x3", "rlcf_split_pairs", "rlcf_last_error"):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return h


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", action="append", required=True, help="NAME=PATH, at least two")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--settle", type=float, default=2.0)
    ap.add_argument("--m-layer", type=int, default=403456)
    ap.add_argument("--m-text", type=int, default=131040)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    arms = [(s.split("=", 1)[0], load(s.split("=", 1)[1])) for s in a.lib]
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for M, shapes in ((a.m_layer, LAYER), (a.m_text, TEXT)):
        for name, N, K, epi, res, pair in shapes:
            act = synth.normal(3, f"ab.a.{name}", (M, K), device=dev)
            w = synth.normal(3, f"ab.w.{name}", (N, K), device=dev) * K ** -0.5
            b = synth.normal(3, f"ab.b.{name}", (N,), device=dev) * 0.1
            x = synth.normal(3, f"ab.x.{name}", (M, N), device=dev) if res else None
            a2, w2 = torch.empty_like(act), torch.empty_like(w)
            h0 = arms[0][1]
            assert h0.rlcf_split_pairs(act.data_ptr(), a2.data_ptr(), act.numel(), L.PREC_F16X3, st) == 0
            assert h0.rlcf_split_pairs(w.data_ptr(), w2.data_ptr(), w.numel(), L.PREC_F16X3, st) == 0
            del act, w
            c = None if pair else torch.empty(M, N, device=dev)
            ch = torch.empty(M, N, dtype=torch.float16, device=dev) if pair else None
            cl = torch.empty_like(ch) if pair else None

            def launch(h):
                rc = h.rlcf_gemm_f16x3(a2.data_ptr(), a2.data_ptr() + 64, 2 * K, w2.data_ptr(), w2.data_ptr() + 64, 2 * K, b.data_ptr(),
                                       x.data_ptr() if res else None, N, None, 0, c.data_ptr() if c is not None else None, N,
                                       ch.data_ptr() if pair else None, cl.data_ptr() if pair else None, N, M, N, K, 1.0, epi, st)
                assert rc == 0, h.rlcf_last_error()
            t0 = time.time()
            while time.time() - t0 < a.settle:
                for _, h in arms:
                    launch(h)
                torch.cuda.synchronize()
            ev = {n: [] for n, _ in arms}
            for _ in range(a.reps):
                for n, h in arms:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    launch(h)
                    e1.record()
                    ev[n].append((e0, e1))
            torch.cuda.synchronize()
            rec = {"shape": name, "M": M, "N": N, "K": K}
            for n, _ in arms:
                us = sorted(e0.elapsed_time(e1) * 1e3 for e0, e1 in ev[n])
                med = us[len(us) // 2]
                rec[n] = {"us_median": round(med, 1), "us_min": round(us[0], 1), "us_max": round(us[-1], 1), "tf": round(2.0 * M * N * K / med * 1e-6, 1)}
            rows.append(rec)
            print(json.dumps(rec), flush=True)
            del a2, w2, c, ch, cl, x
            torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
