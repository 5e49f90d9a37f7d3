#!/usr/bin/env python3
"""Forward + backward of the predictor's tail: `ops.predictor_tail_autograd` (the forward launch of csrc/sea_predictor.hip, the
backward of csrc/sea_tail_bwd.hip) against the torch modules the layer runs without `fused_tail_grad` -- `UpsampleFP32((1, 4))`,
the 1x1 `CausalConv2d`, the `KeepRes` area resize, `LayerNorm(T_M)` and the softmax.  bf16 data, C = 64 channels, H = 32 heads,
T_M = 256; both outputs carry a gradient.  Both variants run alternately in one process; per variant the script prints min /
median / max of the rounds, the device memory held after the forward and the peak above the inputs, and how far the two sets of
gradients are apart."""
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sea_attention_amd.perlin_attention import ops                                                  # noqa: E402
from sea_attention_amd.perlin_attention.modules import CausalConv2d, KeepRes, UpsampleFP32          # noqa: E402

DEV = "cuda:0"
SHAPES = [(8, 64, 4096, 256), (1, 64, 4096, 256)]            # (N, C, T, T_M); H = C / 2
WARMUP, ROUNDS = 3, 10
NAMES = ("dy", "dW", "dgamma", "dbeta")


def hip_step(keepres, ln2, y):
    conv4 = keepres.net[1]
    return ops.predictor_tail_autograd(y, conv4.weight[:, :, 0, 0], conv4.bias, ln2.weight, ln2.bias, 4, ln2.normalized_shape[0], ln2.eps)


def torch_step(keepres, ln2, y):
    s = ln2(keepres(y))
    return torch.softmax(s.float(), dim=-1).to(s.dtype), s


def step(fn, keepres, ln2, y, leaves, g_p, g_s):
    for t in leaves:
        t.grad = None
    torch.autograd.backward(fn(keepres, ln2, y), [g_p, g_s])


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    for N, C, T, T_M in SHAPES:
        H = C // 2
        gen = torch.Generator(device=DEV).manual_seed(0)
        rnd = lambda *s: torch.randn(s, generator=gen, device=DEV)
        torch.manual_seed(0)
        keepres = KeepRes(UpsampleFP32((1, 4)), CausalConv2d(C, H, 1, padding=1, causal=True), output_width=T_M).to(DEV).to(torch.bfloat16)
        ln2 = nn.LayerNorm(T_M).to(DEV).to(torch.bfloat16)
        y = torch.relu(rnd(N, C, T, T_M // 4)).bfloat16().requires_grad_(True)
        conv4 = keepres.net[1]
        leaves = [y, conv4.weight, ln2.weight, ln2.bias]
        g_p, g_s = rnd(N, H, T, T_M).bfloat16(), rnd(N, H, T, T_M).bfloat16()
        variants = {"hip": hip_step, "torch": torch_step}
        res = {k: {"ms": []} for k in variants}
        for name, fn in variants.items():
            for _ in range(WARMUP):
                step(fn, keepres, ln2, y, leaves, g_p, g_s)
            torch.cuda.synchronize()
            for t in leaves:
                t.grad = None
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = fn(keepres, ln2, y)
            torch.cuda.synchronize()
            res[name]["held_mb_after_forward"] = round((torch.cuda.memory_allocated() - base) / 2 ** 20, 1)
            torch.autograd.backward(out, [g_p, g_s])
            torch.cuda.synchronize()
            res[name]["peak_mb_above_inputs"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            res[name]["grads"] = [y.grad.float().clone(), conv4.weight.grad[:, :, 0, 0].float().clone(), ln2.weight.grad.float().clone(),
                                  ln2.bias.grad.float().clone()]
            del out
        for _ in range(ROUNDS):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(fn, keepres, ln2, y, leaves, g_p, g_s)
                e1.record()
                torch.cuda.synchronize()
                res[name]["ms"].append(e0.elapsed_time(e1))
        out = {"shape": [N, C, T, T_M], "H": H, "dtype": "bf16", "rounds": ROUNDS,
               "map_mb": round(N * H * T * T_M * 2 / 2 ** 20, 1), "y_mb": round(N * C * T * (T_M // 4) * 2 / 2 ** 20, 1)}
        for name in variants:
            ms = res[name]["ms"]
            out[name] = {"ms_min": round(min(ms), 3), "ms_median": round(statistics.median(ms), 3), "ms_max": round(max(ms), 3),
                         "held_mb_after_forward": res[name]["held_mb_after_forward"],
                         "peak_mb_above_inputs": res[name]["peak_mb_above_inputs"]}
        out["speedup_median"] = round(statistics.median(res["torch"]["ms"]) / statistics.median(res["hip"]["ms"]), 2)
        out["max_abs_grad_difference"] = {n: (a - b).abs().max().item() for n, a, b in zip(NAMES, res["hip"]["grads"], res["torch"]["grads"])}
        out["max_abs_grad"] = {n: b.abs().max().item() for n, b in zip(NAMES, res["torch"]["grads"])}
        print(json.dumps(out), flush=True)
        del leaves, y, g_p, g_s, res


if __name__ == "__main__":
    main()
