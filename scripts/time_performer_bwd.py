#!/usr/bin/env python3
"""Forward + backward of the estimator's Performer step: `ops.performer_value_autograd` (the forward launch of
csrc/sea_performer.hip, the backward of csrc/sea_performer_bwd.hip) against the torch path the layer runs without
`fused_performer_grad` -- `FastAttention` (perlin_attention/performer.py) plus the two concatenations.  bf16 data, nb = 33.  Both
variants run alternately in one process; per variant the script prints min / median / max of the rounds, the peak device memory
above the inputs, and how far the two sets of gradients are apart."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sea_attention_amd.perlin_attention import ops                                  # noqa: E402
from sea_attention_amd.perlin_attention.performer import FastAttention               # noqa: E402

DEV = "cuda:0"
SHAPES = [(8, 32, 4096, 64), (1, 32, 4096, 64)]
NB = 33
WARMUP, ROUNDS = 3, 10


def hip_step(fa, q, k, v, pos):
    return ops.performer_value_autograd(q, k, v, pos, fa.projection_matrix)


def torch_step(fa, q, k, v, pos):
    vfa = torch.cat([pos.view(1, 1, *pos.shape).expand(v.shape).to(v.dtype), v], dim=-1)
    ctx = fa(q.float(), k.float(), vfa.float()).to(q.dtype)
    return torch.cat([ctx, v], dim=-1)


def step(fn, fa, leaves, g):
    for t in leaves:
        t.grad = None
    fn(fa, *leaves).backward(g)


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    for N, H, T, D in SHAPES:
        gen = torch.Generator(device=DEV).manual_seed(0)
        rnd = lambda *s: torch.randn(s, generator=gen, device=DEV)
        torch.manual_seed(0)
        fa = FastAttention(dim_heads=D, nb_features=NB, causal=True, generalized_attention=True).to(DEV).to(torch.bfloat16)
        leaves = [(rnd(N, H, T, D) * s).bfloat16().requires_grad_(True) for s in (D ** -0.5, 1.0, 1.0)]
        leaves.append(rnd(T, D).bfloat16().requires_grad_(True))
        g = rnd(N, H, T, 3 * D).bfloat16()
        variants = {"hip": hip_step, "torch": torch_step}
        res = {k: {"ms": []} for k in variants}
        for name, fn in variants.items():
            for _ in range(WARMUP):
                step(fn, fa, leaves, g)
            torch.cuda.synchronize()
            for t in leaves:
                t.grad = None
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            out = fn(fa, *leaves)
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
                step(fn, fa, leaves, g)
                e1.record()
                torch.cuda.synchronize()
                res[name]["ms"].append(e0.elapsed_time(e1))
        out = {"shape": [N, H, T, D], "nb": NB, "dtype": "bf16", "rounds": ROUNDS}
        for name in variants:
            ms = res[name]["ms"]
            out[name] = {"ms_min": round(min(ms), 3), "ms_median": round(statistics.median(ms), 3), "ms_max": round(max(ms), 3),
                         "held_mb_after_forward": res[name]["held_mb_after_forward"],
                         "peak_mb_above_inputs": res[name]["peak_mb_above_inputs"]}
        out["speedup_median"] = round(statistics.median(res["torch"]["ms"]) / statistics.median(res["hip"]["ms"]), 2)
        out["max_abs_grad_difference"] = {n: (a - b).abs().max().item() for n, a, b in
                                          zip(("dq", "dk", "dv", "dpos"), res["hip"]["grads"], res["torch"]["grads"])}
        out["max_abs_grad"] = {n: b.abs().max().item() for n, b in zip(("dq", "dk", "dv", "dpos"), res["torch"]["grads"])}
        print(json.dumps(out), flush=True)
        del leaves, g, res


if __name__ == "__main__":
    main()
