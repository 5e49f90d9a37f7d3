#!/usr/bin/env python3
"""Forward + backward of the estimator's KD term: `ops.kd_estimator_loss` (csrc/sea_kd_loss.hip) against the torch expression
the layer runs without `fused_kd_loss` -- `_kl_and_mse` over `resize_from_m_to_t`, in head chunks of 4 (`dense_head_chunk = 4`),
eval mode (no rank jitter).  bf16 est and truth.  Both variants run alternately in one process; per variant the script
prints min / median / max of the rounds, the peak device memory above the inputs, and how far the two results are apart."""
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
SHAPES = [(1, 32, 4096, 256), (1, 32, 2048, 256)]
WARMUP, ROUNDS, CHUNK = 3, 10, 4


def hip_term(est, truth, mask):
    return ops.kd_estimator_loss(est, truth)


def torch_term(est, truth, mask):
    H = est.shape[1]
    loss = 0
    for h0 in range(0, H, CHUNK):
        h1 = min(H, h0 + CHUNK)
        sc = ops.resize_from_m_to_t(x=est[:, h0:h1], masked_fill_value=FP_MIN, attention_mask=mask, target_width=est.shape[2],
                                    training=False, is_causal=True, k=64, oversampled=1.0).float()
        loss = loss + _kl_and_mse(sc, truth[:, h0:h1], mask, FP_MIN) * ((h1 - h0) / H)
        del sc
    return loss


def step(fn, est, truth, mask):
    est.grad = None
    loss = fn(est, truth, mask)
    loss.backward()
    return loss.detach()


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    for N, H, T, T_M in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(0)
        est = (torch.randn((N, H, T, T_M), generator=g, device=DEV) * 2.0).bfloat16().requires_grad_(True)
        truth = (torch.randn((N, H, T, T), generator=g, device=DEV) * 3.0).bfloat16()
        idx = torch.arange(T, device=DEV)
        mask = ((idx.view(1, T) > idx.view(T, 1)) * FP_MIN).view(1, 1, T, T).expand(N, 1, T, T).contiguous()
        variants = {"hip": hip_term, "torch_chunk4": torch_term}
        res = {k: {"ms": []} for k in variants}
        for name, fn in variants.items():
            for _ in range(WARMUP):
                step(fn, est, truth, mask)
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            res[name]["loss"] = float(step(fn, est, truth, mask))
            torch.cuda.synchronize()
            res[name]["peak_mb_above_inputs"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            res[name]["grad"] = est.grad.float().clone()
        for _ in range(ROUNDS):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                step(fn, est, truth, mask)
                e1.record()
                torch.cuda.synchronize()
                res[name]["ms"].append(e0.elapsed_time(e1))
        # the forward launch alone, against its compulsory traffic (the causal half of truth, est, the fp32 outputs)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        fwd = []
        for _ in range(ROUNDS):
            e0.record()
            ops.kd_estimator_loss_parts(est.detach(), truth)
            e1.record()
            torch.cuda.synchronize()
            fwd.append(e0.elapsed_time(e1))
        bytes_fwd = N * H * (T * (T + 1) // 2 * 2 + T * T_M * 2 + T * T_M * 4 + T * 16)
        gd = (res["hip"]["grad"] - res["torch_chunk4"]["grad"]).abs().max().item()
        out = {"shape": [N, H, T, T_M], "dtype": "bf16", "rounds": ROUNDS}
        for name in variants:
            ms = res[name]["ms"]
            out[name] = {"ms_min": round(min(ms), 3), "ms_median": round(statistics.median(ms), 3), "ms_max": round(max(ms), 3),
                         "peak_mb_above_inputs": res[name]["peak_mb_above_inputs"], "loss": res[name]["loss"]}
        out["speedup_median"] = round(statistics.median(res["torch_chunk4"]["ms"]) / statistics.median(res["hip"]["ms"]), 2)
        out["hip_forward_only"] = {"ms_min": round(min(fwd), 3), "ms_median": round(statistics.median(fwd), 3), "ms_max": round(max(fwd), 3),
                                   "compulsory_gb": round(bytes_fwd / 1e9, 3),
                                   "gb_per_s_median": round(bytes_fwd / statistics.median(fwd) / 1e6, 1)}
        out["max_abs_grad_difference"] = gd
        out["max_abs_grad"] = res["torch_chunk4"]["grad"].abs().max().item()
        print(json.dumps(out), flush=True)
        del est, truth, mask, res


if __name__ == "__main__":
    main()
