#!/usr/bin/env python3
"""Paged K / V against contiguous caches for graph-replayed decoding of sequences at different positions
(DecodeSession.from_sequences with and without page_rows) at OPT-1.3B shape (H = 32, d = 64, T_M = 256, k = 64, bf16, N = 8,
lengths 1000 .. 4000).  In one process, after a warm-up, alternates the two sessions and reports the median ms per position
(all eight sequences advance one token) of several repeats as one JSON line, with the K / V bytes each session holds: the
paged pool is sized for the sequences' own lengths (+ one page per slot of headroom), the contiguous caches for N x capacity."""
import json, os, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
from sea_attention_amd.perlin_attention.decode import DecodeSession
N, H, d, T0, T_M, k, PAGE = 8, 32, 64, 4000, 256, 64, 64
WARM, STEPS, REPEATS = 4, int(os.environ.get("STEPS", 16)), int(os.environ.get("REPEATS", 5))
CAP = 4096 if T0 + WARM + STEPS * REPEATS < 4096 else T0 + WARM + STEPS * REPEATS + 1
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
total = WARM + STEPS * REPEATS
POOL = sum(-(-(L + total + 1) // PAGE) for L in LENGTHS) + N
with torch.no_grad():
    seqs = [prefill(x[n:n + 1], q[n:n + 1], L) for n, L in enumerate(LENGTHS)]
    contiguous = DecodeSession.from_sequences(layer.attention, seqs, CAP)
    paged = DecodeSession.from_sequences(layer.attention, seqs, CAP, page_rows=PAGE, pool_pages=POOL)
    del seqs
    def step(sess, i):
        return sess.step(qrows[:, :, i:i + 1], rows[:, :, i:i + 1], rows[:, :, i:i + 1])
    for i in range(WARM):
        a = step(contiguous, i).clone()
        b = step(paged, i)
        assert torch.equal(a, b), i                                          # the same bits, every step
    torch.cuda.synchronize()
    times = {"contiguous_b8": [], "paged_b8": []}
    setups = {"contiguous_b8": contiguous, "paged_b8": paged}
    for r in range(REPEATS):
        base = WARM + r * STEPS
        for name, sess in setups.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(base, base + STEPS):
                step(sess, i)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / STEPS * 1e3)
    assert torch.equal(contiguous.ctx, paged.ctx) and contiguous.lengths == paged.lengths
med = {name: round(statistics.median(v), 4) for name, v in times.items()}
kv_bytes = lambda s: s.kv_cache.numel() * s.kv_cache.element_size()
print(json.dumps({**{f"{n}_ms_per_position": v for n, v in med.items()},
                  "paged_over_contiguous": round(med["paged_b8"] / med["contiguous_b8"], 3),
                  "contiguous_kv_mb": round(kv_bytes(contiguous) / 2 ** 20, 1), "paged_pool_mb": round(kv_bytes(paged) / 2 ** 20, 1),
                  "pool_pages": POOL, "page_rows": PAGE, "pages_in_use": POOL - paged.free_pages, "capacity": CAP,
                  "lengths": LENGTHS, "steps": STEPS, "repeats": REPEATS,
                  "all_ms": {n: [round(t, 4) for t in v] for n, v in times.items()}}))
