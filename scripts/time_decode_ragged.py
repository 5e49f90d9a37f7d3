#!/usr/bin/env python3
"""Graph-replayed decoding of sequences at DIFFERENT positions (DecodeSession.from_sequences) at OPT-1.3B shape
(H = 32, d = 64, T_M = 256, k = 64, bf16).  In one process, after a warm-up, alternates three setups and reports the
median ms per position (all eight sequences advance one token) of several repeats as one JSON line:
  (a) a uniform batch-8 session, every sequence at T0 = 4000;
  (b) a ragged batch-8 session, lengths spread over 1000 .. 4000;
  (c) eight N = 1 sessions at the lengths of (b), stepped in turn."""
import json, os, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
from sea_attention_amd.perlin_attention.decode import DecodeSession
N, H, d, T0, T_M, k = 8, 32, 64, 4000, 256, 64
WARM, STEPS, REPEATS = 4, int(os.environ.get("STEPS", 16)), int(os.environ.get("REPEATS", 5))
CAP = T0 + WARM + STEPS * REPEATS + 1
LENGTHS = [1000 + (T0 - 1000) * i // (N - 1) for i in range(N)]             # 1000 ... 4000
dev, dt = "cuda:0", torch.bfloat16
class Cfg:
    hidden_size, num_attention_heads, max_position_embeddings = H * d, H, CAP
S.seed(42)
pc = PerlinAttentionConfig(k=k, attention_predictor_length=T_M, performer_nb_factor=8, causal=True, k_flatten=True,
                           k_flatten_dim='causal_batch', context_output_method='mix', use_cache=True)
layer = PerlinSelfAttention(Cfg(), pc).to(dev).to(dt).eval()
for m in layer.modules():
    if hasattr(m, 'benchmarking'): m.benchmarking = True
layer.attention.context_layer_dtype = dt
x = torch.randn((N, H, T0, d), device=dev).to(dt); q = (x.float() * d ** -0.5).to(dt)
rows = torch.randn((N, H, WARM + STEPS * REPEATS, d), device=dev).to(dt); qrows = (rows.float() * d ** -0.5).to(dt)
fp_min = torch.finfo(torch.float16).min / 2
def mask(n, T):
    r = torch.arange(T, device=dev)
    return ((r.view(1, T) > r.view(T, 1)) * fp_min).view(1, 1, T, T).expand(n, 1, T, T).to(dt)
def prefill(xs, qs, L):
    out = layer(None, None, None, query_layer=qs[:, :, :L], key_layer=xs[:, :, :L], value_layer=xs[:, :, :L], attention_mask=mask(xs.shape[0], L))
    return out.state, xs[:, :, :L], xs[:, :, :L]
with torch.no_grad():
    uniform = DecodeSession(layer.attention, *prefill(x, q, T0), capacity=CAP)
    seqs = [prefill(x[n:n + 1], q[n:n + 1], L) for n, L in enumerate(LENGTHS)]
    ragged = DecodeSession.from_sequences(layer.attention, seqs, CAP)
    singles = [DecodeSession(layer.attention, *s, capacity=CAP) for s in seqs]
    del seqs
    def step_batch(sess, i):
        sess.step(qrows[:, :, i:i + 1], rows[:, :, i:i + 1], rows[:, :, i:i + 1])
    def step_singles(_, i):
        for n, s in enumerate(singles):
            s.step(qrows[n:n + 1, :, i:i + 1], rows[n:n + 1, :, i:i + 1], rows[n:n + 1, :, i:i + 1])
    setups = {"uniform_b8": (uniform, step_batch), "ragged_b8": (ragged, step_batch), "single_x8": (None, step_singles)}
    for sess, fn in setups.values():
        for i in range(WARM):
            fn(sess, i)
    torch.cuda.synchronize()
    times = {name: [] for name in setups}
    for r in range(REPEATS):
        base = WARM + r * STEPS
        for name, (sess, fn) in setups.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(base, base + STEPS):
                fn(sess, i)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / STEPS * 1e3)
med = {name: round(statistics.median(v), 4) for name, v in times.items()}
print(json.dumps({**{f"{n}_ms_per_position": v for n, v in med.items()},
                  "ragged_over_uniform": round(med["ragged_b8"] / med["uniform_b8"], 3),
                  "single_over_ragged": round(med["single_x8"] / med["ragged_b8"], 2),
                  "lengths": LENGTHS, "uniform_length": T0, "steps": STEPS, "repeats": REPEATS,
                  "all_ms": {n: [round(t, 4) for t in v] for n, v in times.items()}}))
