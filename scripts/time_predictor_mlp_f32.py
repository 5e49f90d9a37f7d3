#!/usr/bin/env python3
"""The predictor MLP on fp32 data: `ops.predictor_mlp_f32` (one launch of csrc/sea_mlp_f32.hip) against the launches the layer runs
with `fused_mlp_fp32` off -- Linear(3d, 2d), `split_layernorm` with GELU, Linear(2d, T_M / 2), `split_layernorm`, the `to_c8` copy and
the gates' Linear + sigmoid -- and the whole fp32 layer step (bench.py's LayerBench, sparse mode) with the switch on and off.
d = 64, T_M = 256; shapes: BASELINE config 2 (8 x 12 x 2048) and the headline shape in fp32 (8 x 32 x 4096).  The variants run
alternately in one process, timed with device events over rounds of STEPS calls after a warm-up; per variant the script prints
min / median / max of the rounds' per-call times and how far the fused outputs are from the unfused ones."""
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
SHAPES = [(8, 12, 2048), (8, 32, 4096)]                      # (N, H, T)
D, T_M = 64, 256
WARMUP, ROUNDS, STEPS = 5, 5, 20


def timed(variants):
    """{name: [ms per call of each round]}: rounds of STEPS calls between two events, the variants alternating round by round"""
    for fn in variants.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(ROUNDS):
        for name, fn in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _s in range(STEPS):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / STEPS)
    return ms


def summary(ms):
    return {"ms_min": round(min(ms), 4), "ms_median": round(statistics.median(ms), 4), "ms_max": round(max(ms), 4)}


def stage(N, H, T):
    gen = torch.Generator(device=DEV).manual_seed(0)
    torch.manual_seed(0)
    Wd = T_M // 4
    mods = [m.to(DEV) for m in (nn.Linear(3 * D, 2 * D), nn.LayerNorm(2 * D), nn.Linear(2 * D, 2 * Wd), nn.LayerNorm(Wd), nn.Linear(2 * D, 2))]
    enc_lin, enc_ln, dec_lin, ln1, sc = mods
    x = torch.randn((N, H, T, 3 * D), generator=gen, device=DEV)

    def unfused():
        tp = ops.split_layernorm(enc_lin(x), 1, enc_ln.weight, enc_ln.bias, enc_ln.eps, gelu=True)
        y = ops.to_c8(ops.split_layernorm(dec_lin(tp), 2, ln1.weight, ln1.bias, ln1.eps))
        g = torch.sigmoid(sc(tp))
        return y, tp, g[..., 0], g[..., 1]
    with torch.no_grad():
        ms = timed({"fused": lambda: ops.predictor_mlp_f32(x, *mods), "fused_with_tpred": lambda: ops.predictor_mlp_f32(x, *mods, want_tpred=True),
                    "unfused": unfused})
        a, b = ops.predictor_mlp_f32(x, *mods, want_tpred=True), unfused()
    rows = N * H * T
    out = {"what": "stage", "shape": [N, H, T], "d": D, "T_M": T_M, "rounds": ROUNDS, "steps_per_round": STEPS,
           "gflop": round(rows * 2 * (3 * D * 2 * D + 2 * D * (2 * Wd + 2)) / 1e9, 2),
           "min_hbm_mb": round(rows * 4 * (3 * D + 2 * Wd + 2) / 2 ** 20, 1)}
    out.update({k: summary(v) for k, v in ms.items()})
    out["speedup_median"] = round(statistics.median(ms["unfused"]) / statistics.median(ms["fused"]), 3)
    out["max_abs_difference"] = {n: (p - q).abs().max().item() for n, p, q in zip(("x_c8", "tpred", "row_scale", "avg_scale"), a, b)}
    print(json.dumps(out), flush=True)


def layer_step(workload, NB):
    import bench
    lb = bench.LayerBench(workload, NB, "fp32", DEV)                      # ONE layer and batch, the switch set around each call

    def step(sw):
        lb.layer.attention.fused_mlp_fp32 = sw
        try:
            return lb.forward()
        finally:
            lb.layer.attention.fused_mlp_fp32 = False
    ms = timed({"switch_on": lambda: step(True), "switch_off": lambda: step(False)})
    out = {"what": "layer step (eager, sparse mode, fp32 data)", "workload": workload, "batch": NB, "rounds": ROUNDS, "steps_per_round": STEPS}
    out.update({k: summary(v) for k, v in ms.items()})
    ctx = [(o.context_layer if hasattr(o, "context_layer") else o[0]).float() for o in (step(True), step(False))]
    d = (ctx[0] - ctx[1]).abs()
    # a near-tie of the top-k selection that the two maps (a few 1e-7 apart) resolve differently changes a whole context row
    out["context_max_abs_difference"] = d.max().item()
    out["context_rows_differing_above_1e-4"] = int((d.amax(-1) > 1e-4).sum().item())
    out["context_rows"] = int(d[..., 0].numel())
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    assert torch.cuda.is_available(), "needs the MI355X"
    for shape in SHAPES:
        stage(*shape)
    layer_step("opt-125m", 8)
    layer_step("opt-1.3b", 8)
