#!/usr/bin/env python3
"""Fork and beam reorder of a paged decode session (DecodeSession.fork / reorder) at OPT-1.3B shape (H = 32, d = 64, T_M = 256,
k = 64, bf16), eight slots, one 4000-token prompt, 64-row pages.  In one process it reports as one JSON line:
  * the pages in use after forking the prompt's slot into the seven others, against eight independently admitted copies;
  * the median ms per position (all eight slots advance one token) of the forked session against the independent one --
    the same kernels, alternated;
  * the median ms per `reorder` with beam-search-like parent maps: the HIP entry (sea_decode_fork) against a torch-ops
    restatement of the same moves (index_select / index_copy_ per buffer) behind the same host bookkeeping, alternated.
Both reorder forms are first checked to leave the same sequences behind."""
import contextlib, json, os, statistics, sys, time, torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
from sea_attention_amd.perlin_attention import ops
from sea_attention_amd.perlin_attention.decode import DecodeSession
N, H, d, T0, T_M, k, PAGE = 8, 32, 64, 4000, 256, 64, 64
WARM, STEPS, REPEATS = 4, int(os.environ.get("STEPS", 16)), int(os.environ.get("REPEATS", 5))
REORDERS = int(os.environ.get("REORDERS", 50))
total = WARM + STEPS * REPEATS + 1
CAP = T0 + total + 8
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
g = torch.Generator(device=dev).manual_seed(0)
x = torch.randn((1, H, T0, d), device=dev, generator=g).to(dt); q = (x.float() * d ** -0.5).to(dt)
rows = torch.randn((N, H, total, d), device=dev, generator=g).to(dt); qrows = (rows.float() * d ** -0.5).to(dt)
fp_min = torch.finfo(torch.float16).min / 2
def prefill(L):
    r = torch.arange(L, device=dev)
    mask = ((r.view(1, L) > r.view(L, 1)) * fp_min).view(1, 1, L, L).to(dt)
    out = layer(None, None, None, query_layer=q[:, :, :L], key_layer=x[:, :, :L], value_layer=x[:, :, :L], attention_mask=mask)
    return out.state, x[:, :, :L], x[:, :, :L]


def torch_fork(moves, n_staged, image, x_ring, y1_ring, counters, block_table, capacity, kv_pool, nb, staging):
    """ops.decode_fork restated in torch ops: every source is gathered (a copy) before any destination is written, so the
    moves have the same snapshot semantics.  Every move must have a source open page (the script checks the lengths)."""
    src, dst = moves[:, 0].long(), moves[:, 1].long()
    n = x_ring.shape[0]
    img = image.view(n, -1)
    ctr, tab = counters.index_select(0, src), block_table.index_select(0, src)
    j = torch.arange(block_table.shape[1], device=tab.device).view(1, -1)
    o = (ctr[:, :1] // kv_pool.shape[3])
    tab = torch.where(j < o, tab, torch.where(j == o, moves[:, 3:4], torch.full_like(tab, -1)))
    img.index_copy_(0, dst, img.index_select(0, src))
    x_ring.index_copy_(0, dst, x_ring.index_select(0, src))
    y1_ring.index_copy_(0, dst, y1_ring.index_select(0, src))
    counters.index_copy_(0, dst, ctr)
    block_table.index_copy_(0, dst, tab)
    kv_pool.index_copy_(1, moves[:, 3].long(), kv_pool.index_select(1, moves[:, 2].long()))


@contextlib.contextmanager
def torch_moves():
    hip = ops.decode_fork
    ops.decode_fork = torch_fork
    try:
        yield
    finally:
        ops.decode_fork = hip


with torch.no_grad():
    A, B = prefill(T0), prefill(16)
    grow = N * 3
    indep = DecodeSession.from_sequences(layer.attention, [A] * N, CAP, page_rows=PAGE, pool_pages=N * -(-(T0 + 1) // PAGE) + grow + 16)
    pages_independent = indep.allocator.pool_pages - indep.free_pages
    forked = DecodeSession.from_sequences(layer.attention, [A] + [B] * (N - 1), CAP, page_rows=PAGE,
                                          pool_pages=-(-(T0 + 1) // PAGE) + (N - 1) + grow + 16)
    forked.fork(0, list(range(1, N)))
    pages_forked = forked.allocator.pool_pages - forked.free_pages
    shared_forked = len(forked.shared_pages)
    del A, B
    def step(sess, i):
        return sess.step(qrows[:, :, i:i + 1], rows[:, :, i:i + 1], rows[:, :, i:i + 1])
    for i in range(WARM):
        a = step(indep, i).clone()
        b = step(forked, i)
        assert torch.equal(a, b), i                                          # the same bits, every step
    torch.cuda.synchronize()
    times = {"independent_b8": [], "forked_b8": []}
    setups = {"independent_b8": indep, "forked_b8": forked}
    for r in range(REPEATS):
        base = WARM + r * STEPS
        for name, sess in setups.items():
            torch.cuda.synchronize(); t0 = time.perf_counter()
            for i in range(base, base + STEPS):
                step(sess, i)
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / STEPS * 1e3)
    assert torch.equal(indep.ctx, forked.ctx) and indep.lengths == forked.lengths
    # reorder: beam-search-like parent maps (ascending parents of a top-k, some slots kept, some parents taken twice)
    gm = torch.Generator().manual_seed(3)
    maps = [torch.randint(0, N, (N,), generator=gm).sort().values.tolist() for _ in range(16)]
    assert all(L % PAGE for L in forked.lengths), "every source has an open page (torch_fork copies pages unconditionally)"
    # the two forms leave the same sequences behind: HIP on one session, torch ops on the other, the same maps
    for parents in maps[:4]:
        forked.reorder(parents)
        with torch_moves():
            indep.reorder(parents)
    for n in range(N):
        assert torch.equal(forked.image.view(N, -1)[n], indep.image.view(N, -1)[n]), n
        assert torch.equal(forked.win[n], indep.win[n]) and all(torch.equal(a, b) for a, b in zip(forked.sequence_kv(n), indep.sequence_kv(n)))
    assert torch.equal(step(forked, total - 1).clone(), step(indep, total - 1)), "one step after the reorders"
    assert all(L % PAGE for L in forked.lengths)
    reorder_ms = {"hip": [], "torch_ops": []}
    for r in range(REPEATS + 1):                                             # (the first round warms both up, not reported)
        for name in reorder_ms:
            ctx = torch_moves() if name == "torch_ops" else contextlib.nullcontext()
            with ctx:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for i in range(REORDERS):
                    forked.reorder(maps[i % len(maps)])
                torch.cuda.synchronize()
            if r:
                reorder_ms[name].append((time.perf_counter() - t0) / REORDERS * 1e3)
med = {name: round(statistics.median(v), 4) for name, v in times.items()}
rmed = {name: round(statistics.median(v), 4) for name, v in reorder_ms.items()}
print(json.dumps({"pages_in_use_forked": pages_forked, "pages_in_use_independent": pages_independent,
                  "shared_pages_forked": shared_forked,
                  **{f"{n}_ms_per_position": v for n, v in med.items()},
                  "forked_over_independent": round(med["forked_b8"] / med["independent_b8"], 3),
                  **{f"reorder_{n}_ms": v for n, v in rmed.items()},
                  "reorder_hip_over_torch_ops": round(rmed["hip"] / rmed["torch_ops"], 3),
                  "moved_slots_per_reorder": round(sum(sum(1 for i, p in enumerate(m) if p != i) for m in maps) / len(maps), 2),
                  "page_rows": PAGE, "prompt": T0, "capacity": CAP, "steps": STEPS, "repeats": REPEATS, "reorders": REORDERS,
                  "all_ms": {n: [round(t, 4) for t in v] for n, v in {**times, **{f"reorder_{k}": v for k, v in reorder_ms.items()}}.items()}}))
