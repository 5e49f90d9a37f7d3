#!/usr/bin/env python3
"""Forward + backward of the predictor MLP: `ops.predictor_mlp_autograd` (the forward launch of csrc/sea_mlp.hip, the backward of
csrc/sea_mlp_bwd.hip) against the torch module chain the layer runs without `fused_mlp_grad` -- Linear(3d, 2d), LayerNorm, GELU,
Linear(2d, T_M / 2), ChannelSplit(2), LayerNorm(T_M / 4) and the `to_c8` copy in front of the conv op.  d = 64, T_M = 256, bf16 data;
both variants end in the C8 tensor and the encoder output.  The variants run alternately in one process and are timed with device
events; per variant the script prints min / median / max of the rounds, the device memory held after the forward and the peak above
the inputs, and how far the gradients are from the torch chain's."""
import json
import os
import statistics
import sys

import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sea_attention_amd.perlin_attention import ops                                                  # noqa: E402

DEV = "cuda:0"
SHAPES = [(8, 32, 4096), (1, 32, 4096)]                      # (N, H, T)
D, T_M = 64, 256
WARMUP, ROUNDS = 3, 10


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    for N, H, T in SHAPES:
        gen = torch.Generator(device=DEV).manual_seed(0)
        rnd = lambda *s: torch.randn(s, generator=gen, device=DEV)
        torch.manual_seed(0)
        Wd = T_M // 4
        mods = [m.to(DEV).to(torch.bfloat16) for m in (nn.Linear(3 * D, 2 * D), nn.LayerNorm(2 * D), nn.Linear(2 * D, 2 * Wd),
                                                       nn.LayerNorm(Wd), nn.Linear(2 * D, 2))]
        enc_lin, enc_ln, dec_lin, ln1, _sc = mods
        gelu = nn.GELU()
        x = rnd(N, H, T, 3 * D).bfloat16().requires_grad_(True)
        g8, gtp = rnd(N, T, H // 4, Wd, 8).bfloat16(), rnd(N, H, T, 2 * D).bfloat16()
        params = [p for m in mods[:4] for p in (m.weight, m.bias)]

        def torch_chain():
            enc = gelu(enc_ln(enc_lin(x)))
            dec = dec_lin(enc)
            y = ln1(dec.view(N, H, T, 2, Wd).permute(0, 1, 3, 2, 4).reshape(N, 2 * H, T, Wd))
            return ops.to_c8(y), enc
        variants = {"hip": lambda: ops.predictor_mlp_autograd(x, *mods), "torch": torch_chain}
        res = {k: {"ms": []} for k in variants}

        def step(name):
            for t in (x, *params):
                t.grad = None
            torch.autograd.backward(variants[name](), [g8, gtp])
        for name, fn in variants.items():
            for _ in range(WARMUP):
                step(name)
            torch.cuda.synchronize()
            for t in (x, *params):
                t.grad = None
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = fn()
            torch.cuda.synchronize()
            res[name]["held_mb_after_forward"] = round((torch.cuda.memory_allocated() - base) / 2 ** 20, 1)
            torch.autograd.backward(out, [g8, gtp])
            torch.cuda.synchronize()
            res[name]["peak_mb_above_inputs"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            res[name]["grads"] = [t.grad.float().clone() for t in (x, *params)]
            del out
        for _ in range(ROUNDS):
            for name in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(name)
                e1.record()
                torch.cuda.synchronize()
                res[name]["ms"].append(e0.elapsed_time(e1))
        out = {"shape": [N, H, T], "d": D, "T_M": T_M, "dtype": "bf16", "rounds": ROUNDS,
               "input_mb": round(N * H * T * 3 * D * 2 / 2 ** 20, 1), "outputs_mb": round(N * H * T * (2 * Wd + 2 * D) * 2 / 2 ** 20, 1)}
        for name in variants:
            ms = res[name]["ms"]
            out[name] = {"ms_min": round(min(ms), 3), "ms_median": round(statistics.median(ms), 3), "ms_max": round(max(ms), 3),
                         "held_mb_after_forward": res[name]["held_mb_after_forward"],
                         "peak_mb_above_inputs": res[name]["peak_mb_above_inputs"]}
        out["speedup_median_hip"] = round(statistics.median(res["torch"]["ms"]) / statistics.median(res["hip"]["ms"]), 2)
        names = ("dx", "dW1", "db1", "dg1", "dbe1", "dW2", "db2", "dg2", "dbe2")
        out["max_abs_grad_difference"] = {n: (a - b).abs().max().item() for n, a, b in zip(names, res["hip"]["grads"], res["torch"]["grads"])}
        out["max_abs_grad"] = {n: b.abs().max().item() for n, b in zip(names, res["torch"]["grads"])}
        print(json.dumps(out), flush=True)
        del res, variants, x, g8, gtp


if __name__ == "__main__":
    main()
