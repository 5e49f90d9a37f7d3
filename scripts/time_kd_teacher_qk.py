#!/usr/bin/env python3
"""Forward + backward of the two KD terms with the teacher factored (`ops.TeacherScores(q_t, k_t)`: include/sea_hip_train.h
"the teacher") against the same ops on the teacher's (N,H,T,T) score tensor.  Per term three variants, alternating in one process:

    factored      the op on TeacherScores(q_t, k_t)
    tensor        the op on a pre-made score tensor
    tensor+bmm    the op on the tensor plus the q_t @ k_t^T bmm that makes it (what the factored op replaces)

bf16, T_M = 256.  3 warm-up steps per variant, then 10 rounds, device events; per variant min / median / max, the peak device
memory above the inputs, and whether the factored median stays within `tensor+bmm`'s (by at most the larger
(max - min) / median spread of the two)."""
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sea_attention_amd.perlin_attention import ops                                  # noqa: E402

DEV = "cuda:0"
SHAPES = [(1, 32, 2048, 64), (1, 32, 4096, 64)]
T_M = 256
WARMUP, ROUNDS = 3, 10


def main():
    assert torch.cuda.is_available(), "needs the MI355X"
    for N, H, T, D in SHAPES:
        g = torch.Generator(device=DEV).manual_seed(0)
        q, k, qt, kt = ((torch.randn((N, H, T, D), generator=g, device=DEV) * 0.6).bfloat16() for _ in range(4))
        est = (torch.randn((N, H, T, T_M), generator=g, device=DEV) * 2.0).bfloat16().requires_grad_(True)
        q.requires_grad_(True)
        k.requires_grad_(True)
        ts = ops.TeacherScores(qt, kt)
        premade = ts.dense()
        terms = {
            "score": {"factored": lambda: ops.kd_score_loss(q, k, ts),
                      "tensor": lambda: ops.kd_score_loss(q, k, premade),
                      "tensor+bmm": lambda: ops.kd_score_loss(q, k, torch.matmul(qt, kt.transpose(-1, -2)))},
            "estimator": {"factored": lambda: ops.kd_estimator_loss(est, ts),
                          "tensor": lambda: ops.kd_estimator_loss(est, premade),
                          "tensor+bmm": lambda: ops.kd_estimator_loss(est, torch.matmul(qt, kt.transpose(-1, -2)))},
        }

        def step(fn):
            q.grad = k.grad = est.grad = None
            loss = fn()
            loss.backward()
            return loss.detach()

        for term, variants in terms.items():
            res = {name: {"ms": []} for name in variants}
            for name, fn in variants.items():
                for _ in range(WARMUP):
                    step(fn)
                q.grad = k.grad = est.grad = None
                torch.cuda.synchronize()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                res[name]["loss"] = float(step(fn))
                torch.cuda.synchronize()
                res[name]["peak_mb_above_inputs"] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            for _ in range(ROUNDS):
                for name, fn in variants.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step(fn)
                    e1.record()
                    torch.cuda.synchronize()
                    res[name]["ms"].append(e0.elapsed_time(e1))
            out = {"term": term, "shape": [N, H, T, D], "T_M": T_M, "dtype": "bf16", "rounds": ROUNDS,
                   "score_tensor_mb": round(N * H * T * T * 2 / 2 ** 20, 1)}
            for name in variants:
                ms = res[name]["ms"]
                med = statistics.median(ms)
                out[name] = {"ms_min": round(min(ms), 3), "ms_median": round(med, 3), "ms_max": round(max(ms), 3),
                             "spread": round((max(ms) - min(ms)) / med, 3),
                             "peak_mb_above_inputs": res[name]["peak_mb_above_inputs"], "loss": res[name]["loss"]}
            ratio = out["factored"]["ms_median"] / out["tensor+bmm"]["ms_median"]
            allowed = 1.0 + max(out["factored"]["spread"], out["tensor+bmm"]["spread"])
            out["factored_over_tensor_plus_bmm"] = round(ratio, 3)
            out["requirement_met"] = bool(ratio <= allowed)
            print(json.dumps(out), flush=True)
        del q, k, qt, kt, est, ts, premade, terms


if __name__ == "__main__":
    main()
