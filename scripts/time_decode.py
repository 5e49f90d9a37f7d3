#!/usr/bin/env python3
"""KV-cache decoding latency of one SEA layer: prefill T0 tokens, then single-token steps.
Reports ms per decoded token (all sequences of the batch advance together) at OPT-1.3B shape.

    python scripts/time_decode.py [--batch 8] [--prefill 4000] [--predictor-length 256] [--k 64] [--steps 32] [--repeats 1]
                                  [--no-cached-forward]

--predictor-length: T_M of the layer (a decode session runs at 64 / 96 / 128 / 256).  --repeats R: the session legs time R
consecutive windows of (steps - 4) positions each and report min / median / max over them (one window: the single figure, as
before).  NB / T0 in the environment are the older spelling of --batch / --prefill."""
import argparse, os, sys, json, statistics, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=int(os.environ.get("NB", 8)))
ap.add_argument("--prefill", type=int, default=int(os.environ.get("T0", 4000)))
ap.add_argument("--predictor-length", type=int, default=256)
ap.add_argument("--k", type=int, default=64)
ap.add_argument("--steps", type=int, default=32, help="positions per window, the first 4 of the first window are warm-up")
ap.add_argument("--repeats", type=int, default=1)
ap.add_argument("--no-cached-forward", action="store_true", help="skip the eager cached-forward leg (one module call per token)")
args = ap.parse_args()
N, H, d, T0, steps, T_M, k, R = args.batch, 32, 64, args.prefill, args.steps, args.predictor_length, args.k, args.repeats
assert steps > 4 and R >= 1
W = steps - 4                                          # timed positions per window
T_all = T0 + 4 + R * W
dev, dt = "cuda:0", torch.bfloat16
class Cfg:
    hidden_size, num_attention_heads, max_position_embeddings = H * d, H, T_all
S.seed(42)
pc = PerlinAttentionConfig(k=k, attention_predictor_length=T_M, performer_nb_factor=8, causal=True, k_flatten=True,
                           k_flatten_dim='causal_batch', context_output_method='mix', use_cache=True)
layer = PerlinSelfAttention(Cfg(), pc).to(dev).to(dt).eval()
for m in layer.modules():
    if hasattr(m, 'benchmarking'): m.benchmarking = True
layer.attention.context_layer_dtype = dt
x = torch.randn((N, H, T_all, d), device=dev).to(dt); q = (x.float() * d ** -0.5).to(dt)
fp_min = torch.finfo(torch.float16).min / 2
def mask(T_dst, T_src):
    rows = torch.arange(T_src - T_dst, T_src, device=dev).view(T_dst, 1)
    return ((torch.arange(T_src, device=dev).view(1, T_src) > rows) * fp_min).view(1, 1, T_dst, T_src).expand(N, 1, T_dst, T_src).to(dt)
res = {}
with torch.no_grad():
    t0 = time.perf_counter()
    out = layer(None, None, None, query_layer=q[:, :, :T0], key_layer=x[:, :, :T0], value_layer=x[:, :, :T0], attention_mask=mask(T0, T0))
    torch.cuda.synchronize(); t_prefill = time.perf_counter() - t0
    if not args.no_cached_forward:
        st = out.state
        for i in range(4):    # warm-up decode steps
            hi = T0 + i + 1
            st = layer(None, None, None, query_layer=q[:, :, hi - 1:hi], key_layer=x[:, :, :hi], value_layer=x[:, :, :hi], attention_mask=mask(1, hi), last_state=st).state
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(4, min(steps, 32)):
            hi = T0 + i + 1
            st = layer(None, None, None, query_layer=q[:, :, hi - 1:hi], key_layer=x[:, :, :hi], value_layer=x[:, :, :hi], attention_mask=mask(1, hi), last_state=st).state
        torch.cuda.synchronize(); t_dec = (time.perf_counter() - t0) / (min(steps, 32) - 4)
        res.update(decode_ms_per_token_step=round(t_dec * 1e3, 3), decode_tokens_per_s=round(N / t_dec, 1))
    # the same positions through the graph-replayed session (perlin_attention/decode.py)
    from sea_attention_amd.perlin_attention.decode import DecodeSession
    for label, use_graph in (("session_eager", False), ("session_graph", True)):
        sess = DecodeSession(layer.attention, out.state, x[:, :, :T0], x[:, :, :T0], capacity=T_all, use_graph=use_graph)
        assert sess.fused_cnn                         # (the one-launch CNN + tail + selection: what these figures are about)
        for i in range(4):
            hi = T0 + i + 1
            sess.step(q[:, :, hi - 1:hi], x[:, :, hi - 1:hi], x[:, :, hi - 1:hi])
        per = []
        for r in range(R):
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(4 + r * W, 4 + (r + 1) * W):
                hi = T0 + i + 1
                sess.step(q[:, :, hi - 1:hi], x[:, :, hi - 1:hi], x[:, :, hi - 1:hi])
            torch.cuda.synchronize()
            per.append((time.perf_counter() - t0) / W * 1e3)
        res[label + "_ms_per_step"] = round(statistics.median(per), 4 if R > 1 else 3)
        if R > 1:
            res[label + "_ms_min_max"] = [round(min(per), 4), round(max(per), 4)]
print(json.dumps({**res, "batch": N, "prefill_tokens": T0, "predictor_length": T_M, "k": k, "window_steps": W, "repeats": R,
                  "prefill_ms": round(t_prefill * 1e3, 2), "lib": os.environ.get("SEA_HIP_LIB", "tree")}))
