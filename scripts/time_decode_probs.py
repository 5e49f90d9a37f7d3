#!/usr/bin/env python3
"""What the attention probabilities of a graph-replayed decode step cost (`DecodeSession(..., attention_probs=True)`), one SEA
layer at OPT-1.3B shape: prefill T0 tokens, then single-token steps.  Legs, ms per position (all sequences advance together):

    session_graph               the replayed session as it always was (probabilities off)
    session_graph_probs         the same with attention_probs=True: the attention launch also stores one fp32 per CSR entry
    cached_forward              the regular cached forward, one module call per token
    cached_forward_probs        ... with attention.return_attention_probs = True: where the probabilities came from before

    python scripts/time_decode_probs.py [--batch 8] [--prefill 4000] [--predictor-length 256] [--k 64] [--steps 32] [--repeats 5]
                                        [--no-cached-forward]

Every leg times --repeats consecutive windows of (steps - 4) positions and reports median and [min, max] over them.  On a tree
without the feature only the legs that exist there run (the figure to compare `session_graph` with)."""
import argparse, inspect, os, sys, json, statistics, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
from sea_attention_amd.perlin_attention.decode import DecodeSession
ap = argparse.ArgumentParser()
ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--prefill", type=int, default=4000)
ap.add_argument("--predictor-length", type=int, default=256)
ap.add_argument("--k", type=int, default=64)
ap.add_argument("--steps", type=int, default=32, help="positions per window, the first 4 of the first window are warm-up")
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--no-cached-forward", action="store_true", help="skip the two cached-forward legs")
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
def windows(step):
    """`step(i)` for positions 0 .. 4 + R * W - 1: four warm-up positions, then R timed windows; ms per position of each."""
    for i in range(4):
        step(i)
    per = []
    for r in range(R):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(4 + r * W, 4 + (r + 1) * W):
            step(i)
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) / W * 1e3)
    return per
res = {}
def report(label, per):
    res[label + "_ms_per_step"] = round(statistics.median(per), 4)
    res[label + "_ms_min_max"] = [round(min(per), 4), round(max(per), 4)]
has_probs = "attention_probs" in inspect.signature(DecodeSession.__init__).parameters
with torch.no_grad():
    out = layer(None, None, None, query_layer=q[:, :, :T0], key_layer=x[:, :, :T0], value_layer=x[:, :, :T0], attention_mask=mask(T0, T0))
    torch.cuda.synchronize()
    for label, on in (("session_graph", False), ("session_graph_probs", True)):
        if on and not has_probs:
            continue
        sess = DecodeSession(layer.attention, out.state, x[:, :, :T0], x[:, :, :T0], capacity=T_all, **(dict(attention_probs=True) if on else {}))
        assert sess.fused_cnn and sess.graph is not None
        def step(i):
            hi = T0 + i + 1
            sess.step(q[:, :, hi - 1:hi], x[:, :, hi - 1:hi], x[:, :, hi - 1:hi])
        report(label, windows(step))
        if on:
            assert sess.attention_probs.col_is_pending and sess.captures == 1
            res["probs_entries_per_sequence"] = int(sess.csr.crow[:, 1].max().item())
        del sess
    if not args.no_cached_forward:
        for label, on in (("cached_forward", False), ("cached_forward_probs", True)):
            state = {"st": out.state}
            layer.attention.return_attention_probs = on
            def step(i):
                hi = T0 + i + 1
                o = layer(None, None, None, query_layer=q[:, :, hi - 1:hi], key_layer=x[:, :, :hi], value_layer=x[:, :, :hi],
                          attention_mask=mask(1, hi), last_state=state["st"])
                assert (o.partial_attention_probs is not None) == on
                state["st"] = o.state
            try:
                report(label, windows(step))
            finally:
                layer.attention.return_attention_probs = False
print(json.dumps({**res, "batch": N, "prefill_tokens": T0, "predictor_length": T_M, "k": k, "window_steps": W, "repeats": R,
                  "attention_probs_supported": has_probs, "lib": os.environ.get("SEA_HIP_LIB", "tree")}))
