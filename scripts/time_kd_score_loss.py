#!/usr/bin/env python3
"""Forward + backward of the student-score KD term: `ops.kd_score_loss` (csrc/sea_kd_score_loss.hip) against the torch
expression the layer runs without `fused_kd_score_loss` -- `_kl_and_mse` over `q_for_score @ k_for_score^T`, in head chunks of
4 (`dense_head_chunk = 4`).  bf16 q, k and truth.  Both variants run alternately in one process; per variant the script prints
min / median / max of the rounds, the peak device memory above the inputs, and how far the two results are apart (the torch
form rounds q k^T to bf16 before the softmaxes, the kernels do not: DESIGN 5.8)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sea_attention_amd.perlin_attention import ops                                  # noqa: E402
from sea_attention_amd.perlin_attention.attention import _kl_and_mse                 # noqa: E402

DEV = "cuda:0"
FP_MIN = torch.finfo(torch.float16).min / 2
SHAPES = [(1, 32, 2048, 64), (1, 32, 4096, 64)]
WARMUP, ROUNDS, CHUNK = 3, 10, 4
HBM_GB_PER_S = 8000.0


def hip_term(q, k, truth, mask):
    return ops.kd_score_loss(q, k, truth)


def torch_term(q, k, truth, mask):
    H = q.shape[1]
    loss = 0
    for h0 in range(0, H, CHUNK):
        h1 = min(H, h0 + CHUNK)
        scores = torch.matmul(q[:, h0:h1], k[:, h0:h1].transpose(-1, -2))
        loss = loss + _kl_and_mse(scores, truth[:, h0:h1], mask, FP_MIN) * ((h1 - h0) / H)
        del scores
    return loss


def step(fn, q, k, truth, mask):
    q.grad = k.grad = None
    loss = fn(q, k, truth, mask)
    loss.backward()
    return loss.detach()


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    for N, H, T, D in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(0)
        q = (torch.randn((N, H, T, D), generator=g, device=DEV) * 0.6).bfloat16().requires_grad_(True)
        k = (torch.randn((N, H, T, D), generator=g, device=DEV) * 0.6).bfloat16().requires_grad_(True)
        truth = (torch.randn((N, H, T, T), generator=g, device=DEV) * 3.0).bfloat16()
        idx = torch.arange(T, device=DEV)
        mask = ((idx.view(1, T) > idx.view(T, 1)) * FP_MIN).view(1, 1, T, T).expand(N, 1, T, T).contiguous()
        variants = {"hip": hip_term, "torch_chunk4": torch_term}
        res = {name: {"ms": []} for name in variants}
        for name, fn in variants.items():
            for _ in range(WARMUP):
                step(fn, q, k, truth, mask)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            res[name]["loss"] = float(step(fn, q, k, truth, mask))
            torch.cuda.synchronize()
            res[name]["peak_mb_above_inputs"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            res[name]["grads"] = (q.grad.float().clone(), k.grad.float().clone())
        for _ in range(ROUNDS):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(fn, q, k, truth, mask)
                e1.record()
                torch.cuda.synchronize()
                res[name]["ms"].append(e0.elapsed_time(e1))
        # the forward launch alone, against its compulsory traffic: the causal half of truth once per sweep (two sweeps), q, k
        # and the fp32 row outputs
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fwd = []
        for _ in range(ROUNDS):
            e0.record()
            ops.kd_score_loss_parts(q.detach(), k.detach(), truth)
            e1.record()
            torch.cuda.synchronize()
            fwd.append(e0.elapsed_time(e1))
        half = N * H * (T * (T + 1) // 2) * 2
        bytes_fwd = 2 * half + N * H * T * (2 * D * 2 + 7 * 4)
        out = {"shape": [N, H, T, D], "dtype": "bf16", "rounds": ROUNDS}
        for name in variants:
            ms = res[name]["ms"]
            out[name] = {"ms_min": round(min(ms), 3), "ms_median": round(statistics.median(ms), 3), "ms_max": round(max(ms), 3),
                         "peak_mb_above_inputs": res[name]["peak_mb_above_inputs"], "loss": res[name]["loss"]}
        out["speedup_median"] = round(statistics.median(res["torch_chunk4"]["ms"]) / statistics.median(res["hip"]["ms"]), 2)
        gbs = bytes_fwd / statistics.median(fwd) / 1e6
        out["hip_forward_only"] = {"ms_min": round(min(fwd), 3), "ms_median": round(statistics.median(fwd), 3), "ms_max": round(max(fwd), 3),
                                   "causal_half_of_truth_gb": round(half / 1e9, 3), "traffic_gb": round(bytes_fwd / 1e9, 3),
                                   "gb_per_s_median": round(gbs, 1), "fraction_of_8_tb_per_s": round(gbs / HBM_GB_PER_S, 3)}
        for i, nm in enumerate(("q", "k")):
            out[f"max_abs_d_{nm}_difference"] = (res["hip"]["grads"][i] - res["torch_chunk4"]["grads"][i]).abs().max().item()
            out[f"max_abs_d_{nm}"] = res["torch_chunk4"]["grads"][i].abs().max().item()
        print(json.dumps(out), flush=True)
        del q, k, truth, mask, res


if __name__ == "__main__":
    main()
