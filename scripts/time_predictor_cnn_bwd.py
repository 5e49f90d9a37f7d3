#!/usr/bin/env python3
"""Forward + backward of the predictor CNN's two (convolution, ReLU) pairs: `ops.causal_conv_relu_autograd` on C8 activations (the
forward launch of csrc/sea_conv.hip, the backward of csrc/sea_conv_bwd.hip) against the torch modules the layer runs without
`fused_cnn_grad` -- `CausalConv2d(C, C, 3, padding=2, dilation=2, causal=True)` + `ReLU`, twice, on NCHW.  bf16 data.  The HIP
variant is timed with the two re-layouts the layer pays (`ops.to_c8` / `ops.from_c8`, "hip") and without them ("hip_c8").  All
variants run alternately in one process; per variant the script prints min / median / max of the rounds, the device memory held
after the forward and the peak above the inputs, and how far the gradients are from the torch modules'."""
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sea_attention_amd.perlin_attention import ops                                                  # noqa: E402
from sea_attention_amd.perlin_attention.modules import CausalConv2d                                 # noqa: E402

DEV = "cuda:0"
SHAPES = [(8, 64, 4096, 64), (1, 64, 4096, 64)]              # (N, C, T, W)
WARMUP, ROUNDS = 3, 10


def pairs(convs, y8):
    for cv in convs:
        y8 = ops.causal_conv_relu_autograd(y8, cv.weight, cv.bias, 3, cv.dilation, cv.padding[1])
    return y8


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    for N, C, T, W in SHAPES:
        gen = torch.Generator(device=DEV).manual_seed(0)
        rnd = lambda *s: torch.randn(s, generator=gen, device=DEV)
        torch.manual_seed(0)
        convs = [CausalConv2d(C, C, 3, padding=2, dilation=2, causal=True).to(DEV).to(torch.bfloat16) for _ in range(2)]
        net = nn.Sequential(convs[0], nn.ReLU(), convs[1], nn.ReLU())
        x = rnd(N, C, T, W).bfloat16().requires_grad_(True)
        x8 = ops.to_c8(x.detach()).requires_grad_(True)
        g = rnd(N, C, T, W).bfloat16()
        g8 = ops.to_c8(g)
        params = [p for cv in convs for p in (cv.weight, cv.bias)]
        variants = {"hip": (lambda: ops.from_c8(pairs(convs, ops.to_c8(x))), x, g),
                    "hip_c8": (lambda: pairs(convs, x8), x8, g8),
                    "torch": (lambda: net(x), x, g)}
        res = {k: {"ms": []} for k in variants}

        def step(name):
            fn, leaf, go = variants[name]
            for t in (leaf, *params):
                t.grad = None
            fn().backward(go)
        for name, (fn, leaf, go) in variants.items():
            for _ in range(WARMUP):
                step(name)
            torch.cuda.synchronize()
            for t in (leaf, *params):
                t.grad = None
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = fn()
            torch.cuda.synchronize()
            res[name]["held_mb_after_forward"] = round((torch.cuda.memory_allocated() - base) / 2 ** 20, 1)
            out.backward(go)
            torch.cuda.synchronize()
            res[name]["peak_mb_above_inputs"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            dx = leaf.grad if leaf is x else ops.from_c8(leaf.grad)
            res[name]["grads"] = [dx.float().clone()] + [p.grad.float().clone() for p in params]
            del out
        for _ in range(ROUNDS):
            for name in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(name)
                e1.record()
                torch.cuda.synchronize()
                res[name]["ms"].append(e0.elapsed_time(e1))
        out = {"shape": [N, C, T, W], "dtype": "bf16", "dilation": 2, "rounds": ROUNDS, "activation_mb": round(N * C * T * W * 2 / 2 ** 20, 1)}
        for name in variants:
            ms = res[name]["ms"]
            out[name] = {"ms_min": round(min(ms), 3), "ms_median": round(statistics.median(ms), 3), "ms_max": round(max(ms), 3),
                         "held_mb_after_forward": res[name]["held_mb_after_forward"],
                         "peak_mb_above_inputs": res[name]["peak_mb_above_inputs"]}
        names = ("dx", "dW1", "db1", "dW2", "db2")
        for name in ("hip", "hip_c8"):
            out[f"speedup_median_{name}"] = round(statistics.median(res["torch"]["ms"]) / statistics.median(res[name]["ms"]), 2)
        out["max_abs_grad_difference"] = {n: (a - b).abs().max().item() for n, a, b in zip(names, res["hip"]["grads"], res["torch"]["grads"])}
        out["max_abs_grad"] = {n: b.abs().max().item() for n, b in zip(names, res["torch"]["grads"])}
        print(json.dumps(out), flush=True)
        del res, variants, x, x8, g, g8


if __name__ == "__main__":
    main()
