#!/usr/bin/env python3
"""The key-range form of the attention launch (`ops.sparse_attention(path="keyrange")`, csrc/sea_attn_keyrange.hip) against the
fused gather form, on the layer's own selection: the estimator runs once per shape, its (bits, crow, head_off) are kept, and the
variants are timed interleaved in one process -- HIP-event medians of REPS single launches each after a warm-up.  The gather
form's own min / max stand beside its median: the spread a difference has to exceed.

    python scripts/time_attn_keyrange.py [--out profiles/time_attn_keyrange.json] [--reps 30] [--shapes name,name]

One JSON document: per shape the gather form, and per range_keys the key-range form with its workspace bytes and its max
difference from the gather form's context."""
import argparse, json, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import sea_attention_amd as S
from bench import _Cfg
from sea_attention_amd.perlin_attention import ops, PerlinAttentionConfig, PerlinSelfAttention
from sea_attention_amd.perlin_attention import attention as A
from sea_attention_amd.perlin_attention.ops import flat_csr

SHAPES = {                       # (H, d, N, T): T_M = 256, k = 64 as in bench.py
    "opt-125m_x1_T32768": (12, 64, 1, 32768),
    "opt-125m_x1_T16384": (12, 64, 1, 16384),
    "llama-13b_x1_T16384": (40, 128, 1, 16384),
    "opt-1.3b_x8_T4096": (32, 64, 8, 4096),          # the headline: K + V per head fit the L2, not expected to pay
}
RANGES = (2048, 4096, 8192, 16384)
T_M, K, DEV, DT = 256, 64, "cuda:0", torch.bfloat16


def selection(H, d, N, T):
    """One forward of the layer; the attention launch's own arguments (q, k, v, the CSR handle with pending columns, gates)."""
    S.seed(42)
    pc = PerlinAttentionConfig(k=K, attention_predictor_length=T_M, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix')
    layer = PerlinSelfAttention(_Cfg(H * d, H, T), pc).to(DEV).to(DT).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = True
    layer.attention.context_layer_dtype = DT
    layer.attention.assume_not_padded = True
    S.seed(7)
    x = torch.randn((N, H, T, d), device=DEV)
    q, kk, v = (x * d ** -0.5).to(DT), torch.randn_like(x).to(DT), torch.randn_like(x).to(DT)
    del x
    fp_min = torch.finfo(torch.float16).min / 2
    ar = torch.arange(T, device=DEV)
    mask = ((ar.view(1, T) > ar.view(T, 1)).to(DT) * fp_min).view(1, 1, T, T).expand(N, 1, T, T)
    seen = {}
    real = A.ops.sparse_attention

    def spy(q_, k_, v_, csr, **kw):
        seen.update(q=q_, k=k_, v=v_, csr=csr, kw=dict(kw), pending=csr._pending)
        return real(q_, k_, v_, csr, **kw)
    A.ops.sparse_attention = spy
    try:
        with torch.no_grad():
            layer(None, None, None, query_layer=q, key_layer=kk, value_layer=v, attention_mask=mask)
    finally:
        A.ops.sparse_attention = real
    torch.cuda.synchronize()
    del mask, layer
    torch.cuda.empty_cache()
    assert seen["pending"] is not None, "the layer's handle keeps its columns pending"
    return seen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    a = ap.parse_args()
    assert a.reps >= 20
    res = {"device": torch.cuda.get_device_name(0), "dtype": "bf16", "T_M": T_M, "k": K, "reps": a.reps, "shapes": {}}
    for name in a.shapes.split(","):
        H, d, N, T = SHAPES[name]
        seen = selection(H, d, N, T)
        csr = seen["csr"]
        epi = {k_: seen["kw"][k_] for k_ in ("row_scale", "avg", "mix")}
        outs = {}

        def launch(rk):
            csr._pending = seen["pending"]                                       # (the handle stays pending either way)
            out = outs.setdefault(rk, torch.empty((N, T, H * d), dtype=DT, device=DEV))
            kw = dict(path="keyrange", range_keys=rk) if rk else dict(path="gather", keep_columns_pending=True)
            ops.sparse_attention(seen["q"], seen["k"], seen["v"], csr, out=out.view(N, T, H, d).permute(0, 2, 1, 3), **epi, **kw)
            return out
        variants = [0] + [rk for rk in RANGES if rk < T and -(-T // rk) <= 64]
        for _ in range(a.warmup):
            for rk in variants:
                launch(rk)
        torch.cuda.synchronize()
        times = {rk: [] for rk in variants}
        for _ in range(a.reps):                                                   # interleaved: drift hits every variant alike
            for rk in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); launch(rk); e1.record()
                torch.cuda.synchronize()
                times[rk].append(e0.elapsed_time(e1))
        ref = outs[0].float()
        g = times[0]
        row = {"H": H, "d": d, "N": N, "T": T, "nnz": int(csr.crow[:, -1].sum()), "kv_bytes_per_head": 2 * T * d * 2,
               "gather_ms": {"median": round(statistics.median(g), 4), "min": round(min(g), 4), "max": round(max(g), 4)},
               "keyrange": {}}
        for rk in variants[1:]:
            R = -(-T // rk)
            ws = ((ops.keyrange_workspace_floats(1, H, T, d, R) + 3) & ~3) * N * 4
            t = times[rk]
            row["keyrange"][str(rk)] = {"ranges": R, "median_ms": round(statistics.median(t), 4), "min_ms": round(min(t), 4),
                                        "max_ms": round(max(t), 4), "workspace_bytes": ws,
                                        "vs_gather": round(statistics.median(t) / statistics.median(g), 3),
                                        "max_abs_diff_from_gather": float((outs[rk].float() - ref).abs().max())}
        res["shapes"][name] = row
        print(json.dumps({name: row}), flush=True)
        del seen, csr, outs, epi
        flat_csr.clear_bwd_workspace()
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
