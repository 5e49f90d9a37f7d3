#!/usr/bin/env python3
"""Forward + backward of the sparse context branch: `ops.sparse_context_autograd` (csrc/sea_context_grad.hip around the attention
launch and its backward) against the path the layer runs without `fused_context_grad` -- `ops.sparse_attention_autograd` plus the
fp32 torch cumulative average, the permute and the cast, as `_forward_sparse` writes them.  bf16 data, fp32 context, the layer's own
kind of CSR (top-k of a random (N,H,T,T_M) map with the module's keep table, T_M = 256, k = 64).  Both variants run alternately in
one process; per variant the script prints min / median / max of the rounds, the device memory held after the forward and the peak
above the inputs, and how far the two sets of gradients are apart.

    --shapes N,H,T,D ...     other shapes than the two of DESIGN 5.15"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sea_attention_amd.perlin_attention import ops                                  # noqa: E402
from sea_attention_amd.perlin_attention.ops import flat_csr                          # noqa: E402

DEV = "cuda:0"
SHAPES = [(8, 32, 4096, 64), (1, 32, 4096, 64)]
T_M, K = 256, 64
WARMUP, ROUNDS = 3, 10
NAMES = ("dq", "dk", "dv", "d row_scale", "d mix")


def hip_step(csr, q, k, v, rs, mix):
    return ops.sparse_context_autograd(q, k, v, csr, rs, mix)


def torch_step(csr, q, k, v, rs, mix):
    N, H, T, D = v.shape
    avg = (v.float().cumsum(-2) / torch.arange(1, T + 1, device=v.device, dtype=torch.float32).view(1, 1, -1, 1)).to(v.dtype)
    p2 = ops.sparse_attention_autograd(q, k, v, csr, row_scale=rs, avg=avg, mix=mix)
    return p2.permute(0, 2, 1, 3).reshape(N, T, H * D).to(torch.float32)


def step(fn, csr, leaves, g):
    for t in leaves:
        t.grad = None
    fn(csr, *leaves).backward(g)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=None)
    args = ap.parse_args()
    shapes = SHAPES if not args.shapes else [tuple(int(x) for x in s.split(",")) for s in args.shapes]
    assert torch.cuda.is_available(), "needs the MI355X"
    for N, H, T, D in shapes:
        gen = torch.Generator(device=DEV).manual_seed(0)
        rnd = lambda *s: torch.randn(s, generator=gen, device=DEV)
        probs = torch.softmax(rnd(N, H, T, T_M), -1)
        csr, _ = ops.topk_to_csr(probs, ops.keep_table_causal(H, T, T_M, K, device=DEV), K, target_width=T)
        del probs
        leaves = [(rnd(N, H, T, D) * s).bfloat16().requires_grad_(True) for s in (D ** -0.5, 1.0, 1.0)]
        leaves += [torch.sigmoid(rnd(N, H, T)).requires_grad_(True) for _ in range(2)]
        g = rnd(N, T, H * D)
        variants = {"hip": hip_step, "torch": torch_step}
        res = {k: {"ms": []} for k in variants}
        for name, fn in variants.items():
            for _ in range(WARMUP):
                step(fn, csr, leaves, g)
            torch.cuda.synchronize()
            for t in leaves:
                t.grad = None
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = fn(csr, *leaves)
            torch.cuda.synchronize()
            res[name]["held_mb_after_forward"] = round((torch.cuda.memory_allocated() - base) / 2 ** 20, 1)
            out.backward(g)
            torch.cuda.synchronize()
            res[name]["peak_mb_above_inputs"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            res[name]["grads"] = [t.grad.float().clone() for t in leaves]
            del out
        for _ in range(ROUNDS):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(fn, csr, leaves, g)
                e1.record()
                torch.cuda.synchronize()
                res[name]["ms"].append(e0.elapsed_time(e1))
        out = {"shape": [N, H, T, D], "T_M": T_M, "k": K, "dtype": "bf16", "rounds": ROUNDS}
        for name in variants:
            ms = res[name]["ms"]
            out[name] = {"ms_min": round(min(ms), 3), "ms_median": round(statistics.median(ms), 3), "ms_max": round(max(ms), 3),
                         "held_mb_after_forward": res[name]["held_mb_after_forward"],
                         "peak_mb_above_inputs": res[name]["peak_mb_above_inputs"]}
        out["speedup_median"] = round(statistics.median(res["torch"]["ms"]) / statistics.median(res["hip"]["ms"]), 2)
        out["max_abs_grad_difference"] = {n: (a - b).abs().max().item() for n, a, b in zip(NAMES, res["hip"]["grads"], res["torch"]["grads"])}
        out["max_abs_grad"] = {n: b.abs().max().item() for n, b in zip(NAMES, res["torch"]["grads"])}
        print(json.dumps(out), flush=True)
        del leaves, g, res, csr
        flat_csr.clear_bwd_workspace()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
