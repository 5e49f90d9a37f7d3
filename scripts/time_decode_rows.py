#!/usr/bin/env python3
"""Multi-token steps of a graph-replayed ragged session (DecodeSession.from_sequences(..., max_step_rows=8)) against the plain
one-row step at OPT-1.3B shape (H = 32, d = 64, T_M = 256, k = 64, bf16, N = 8, lengths 1000 .. 4000).  In one process,
after a warm-up, alternates: the plain session's one-row step, then for s in {1, 2, 4, 8} an s-row step of the S = 8 session
followed by a seeded random rewind -- timed with the rewind and without it (the step alone) -- and reports the median ms per
step of several repeats as one JSON line, with each s-row step's cost over the plain step."""
import json, os, random, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
from sea_attention_amd.perlin_attention.decode import DecodeSession
N, H, d, T0, T_M, k, SMAX = 8, 32, 64, 4000, 256, 64, 8
SV = [int(v) for v in os.environ.get("ROWS", "1,2,4,8").split(",")]                 # (ROWS=4: one s, e.g. under a profiler)
WARM, STEPS, REPEATS = 2, int(os.environ.get("STEPS", 16)), int(os.environ.get("REPEATS", 5))
CAP = T0 + 2 * (WARM + STEPS * REPEATS) * sum(SV) + 64                          # (rows past the rewinds, with room)
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
rows = torch.randn((N, H, SMAX, d), device=dev).to(dt); qrows = (rows.float() * d ** -0.5).to(dt)
fp_min = torch.finfo(torch.float16).min / 2
def mask(n, T):
    r = torch.arange(T, device=dev)
    return ((r.view(1, T) > r.view(T, 1)) * fp_min).view(1, 1, T, T).expand(n, 1, T, T).to(dt)
def prefill(xs, qs, L):
    out = layer(None, None, None, query_layer=qs[:, :, :L], key_layer=xs[:, :, :L], value_layer=xs[:, :, :L], attention_mask=mask(xs.shape[0], L))
    return out.state, xs[:, :, :L], xs[:, :, :L]
rng = random.Random(int(os.environ.get("SEED", 3)))
with torch.no_grad():
    seqs = [prefill(x[n:n + 1], q[n:n + 1], L) for n, L in enumerate(LENGTHS)]
    plain = DecodeSession.from_sequences(layer.attention, seqs, CAP)
    multi = DecodeSession.from_sequences(layer.attention, seqs, CAP, max_step_rows=SMAX)
    del seqs
    def one(i):
        return plain.step(qrows[:, :, :1], rows[:, :, :1], rows[:, :, :1])
    def rows_step(s, rewind):
        multi.step(qrows[:, :, :s], rows[:, :, :s], rows[:, :, :s])
        if rewind:
            multi.rewind([rng.randint(0, s) for _ in range(N)])
    for i in range(WARM):                                                   # (captures every s-graph)
        one(i)
        for s in SV:
            rows_step(s, True)
    torch.cuda.synchronize()
    times = {"plain_1": []}
    for s in SV:
        times[f"rows_{s}"] = []
        times[f"rows_{s}_rewind"] = []
    def timed(name, fn):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(STEPS):
            fn()
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / STEPS * 1e3)
    for r in range(REPEATS):
        timed("plain_1", lambda: one(0))
        for s in SV:
            timed(f"rows_{s}", lambda: rows_step(s, False))
            timed(f"rows_{s}_rewind", lambda: rows_step(s, True))
    captures = multi.captures
med = {name: round(statistics.median(v), 4) for name, v in times.items()}
print(json.dumps({**{f"{n}_ms_per_step": v for n, v in med.items()},
                  **{f"rows_{s}_over_plain": round(med[f"rows_{s}"] / med["plain_1"], 3) for s in SV},
                  **{f"rows_{s}_rewind_over_plain": round(med[f"rows_{s}_rewind"] / med["plain_1"], 3) for s in SV},
                  "captures": captures, "capacity": CAP, "lengths": LENGTHS, "steps": STEPS, "repeats": REPEATS,
                  "all_ms": {n: [round(t, 4) for t in v] for n, v in times.items()}}))
