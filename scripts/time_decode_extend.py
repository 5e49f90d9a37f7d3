#!/usr/bin/env python3
"""Extending a forked decode slot by a suffix (DecodeSession.extend) at OPT-1.3B shape (H = 32, d = 64, T_M = 256, k = 64,
bf16): eight slots, one parked 4000-token prompt, 64-row pages, suffixes of 16, 64 and 256 rows.  One JSON line:
  * ms per call of `extend` against the route that exists without it -- export_state + sequence_kv + the cached forward +
    admit -- alternated in this process, the slot reset by a `fork` from the parked prompt before every call (not timed);
    both are first checked to leave the same sequence behind.  A tree without `extend` reports the existing route alone;
  * the 64-row suffix as 64 one-row replayed steps of the forked slot (the other slots paused): ms per row, beside ms per row
    of the two routes above;
  * pages in use after seven copies took a 200-row suffix each through `extend`, against seven admitted copies;
  * ms per all-active one-row step, contiguous and paged, and per 4-row step of a `max_step_rows` session (no kernel of
    theirs belongs to `extend`: the figures are there to be compared with another tree's).
`--compare PARENT.jsonl NEW.jsonl` pools the lines two trees printed in alternated runs of one job into the summary line
(min / median / max of all repeats, ratios of medians) kept in profiles/time_decode_extend.json."""
import json, os, statistics, sys, time


def _mmm(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4), "repeats": len(v)}


def compare(parent_path, new_path):
    load = lambda p: [json.loads(ln) for ln in open(p) if ln.strip().startswith("{")]
    par, new = load(parent_path), load(new_path)
    pool = lambda runs, *keys: [t for r in runs for t in _dig(r["all_ms"], keys)]
    out = {"runs": {"parent": len(par), "new": len(new)}, "suffix": {}, "steps": {}}
    for s in new[0]["suffixes"]:
        a, b, c = pool(new, "extend", str(s)), pool(par, "existing", str(s)), pool(new, "existing", str(s))
        out["suffix"][str(s)] = {"extend_ms": _mmm(a), "parent_existing_route_ms": _mmm(b), "existing_route_same_process_ms": _mmm(c),
                                 "extend_over_parent_route": round(statistics.median(a) / statistics.median(b), 3)}
    for name in ("step_contiguous", "step_paged", "step_rows4"):
        a, b = pool(new, name), pool(par, name)
        lo, hi = min(b) - 0.0008, max(b) + 0.0008                            # the parent's own min - max, widened by 0.8 us
        out["steps"][name] = {"new_ms": _mmm(a), "parent_ms": _mmm(b), "new_median_inside_parent_range": lo <= statistics.median(a) <= hi}
    s64 = out["suffix"]["64"]
    out["per_row_ms_at_64"] = {"extend": round(s64["extend_ms"]["median"] / 64, 5),
                               "parent_existing_route": round(s64["parent_existing_route_ms"]["median"] / 64, 5),
                               "parent_one_row_steps": round(statistics.median(pool(par, "suffix_as_steps_per_row")), 5),
                               "one_row_steps": round(statistics.median(pool(new, "suffix_as_steps_per_row")), 5)}
    out["pages"] = new[0]["pages"]
    print(json.dumps(out))


def _dig(d, keys):
    for k in keys:
        d = d[k]
    return d


if len(sys.argv) > 1 and sys.argv[1] == "--compare":
    compare(sys.argv[2], sys.argv[3])
    sys.exit(0)

import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
from sea_attention_amd.perlin_attention.decode import DecodeSession
N, H, d, T0, T_M, k, PAGE = 8, 32, 64, 4000, 256, 64, 64
SUFFIXES = (16, 64, 256)
WARM, STEPS, REPEATS, CALLS = 4, int(os.environ.get("STEPS", 32)), int(os.environ.get("REPEATS", 5)), int(os.environ.get("CALLS", 4))
CAP = T0 + max(4 * (WARM + STEPS * REPEATS), max(SUFFIXES) + 64) + 8
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
rows = torch.randn((N, H, CAP - T0, d), device=dev, generator=g).to(dt); qrows = (rows.float() * d ** -0.5).to(dt)
fp_min = torch.finfo(torch.float16).min / 2
has_extend = hasattr(DecodeSession, "extend")


def tail_mask(s, T):
    return torch.triu(torch.full((s, T), fp_min, dtype=dt, device=dev), diagonal=T - s + 1).view(1, 1, s, T)


def existing_route(sess, slot, qs, ks):
    """What reaches the state of `extend` without it: export, gather, the cached forward over the suffix, admit."""
    st = sess.export_state(slot)
    kp, vp = sess.sequence_kv(slot)
    k_all, v_all = torch.cat([kp, ks], 2), torch.cat([vp, ks], 2)
    out = layer(None, None, None, query_layer=qs, key_layer=k_all, value_layer=v_all,
                attention_mask=tail_mask(qs.shape[2], k_all.shape[2]), last_state=st)
    sess.admit(slot, out.state, k_all, v_all)
    return out.context_layer


def timed(fn):
    torch.cuda.synchronize(); t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


with torch.no_grad():
    mask = tail_mask(T0, T0)
    A = layer(None, None, None, query_layer=q, key_layer=x, value_layer=x, attention_mask=mask)
    A = (A.state, x, x)
    del mask
    copies = N - 1
    pool = -(-(T0 + 1) // PAGE) + copies * (-(-(T0 + 200 + 1) // PAGE) + 1) + 16
    park = DecodeSession.from_sequences(layer.attention, [A] + [None] * copies, CAP, page_rows=PAGE, pool_pages=pool)
    park.pause(0)
    routes = {"existing": existing_route}
    if has_extend:
        routes["extend"] = lambda sess, slot, qs, ks: sess.extend(slot, qs, ks, ks)
    # pages: seven copies of the prompt, each with a 200-row suffix of its own
    pages = {}
    for name, route in routes.items():
        park.fork(0, list(range(1, N)))
        for n in range(1, N):
            route(park, n, qrows[n:n + 1, :, :200], rows[n:n + 1, :, :200])
        pages[f"in_use_{name}"] = park.allocator.pool_pages - park.free_pages
        pages[f"shared_{name}"] = len(park.shared_pages)
    # the two routes leave the same sequence behind
    if has_extend:
        park.fork(0, [1, 2])
        a = park.extend(1, qrows[:1, :, :64], rows[:1, :, :64], rows[:1, :, :64])
        b = existing_route(park, 2, qrows[:1, :, :64], rows[:1, :, :64])
        assert torch.equal(a, b) and park.lengths[1] == park.lengths[2] == T0 + 64
        assert torch.equal(park.image.view(N, -1)[1], park.image.view(N, -1)[2]) and torch.equal(park.win[1], park.win[2])
        assert all(torch.equal(u, v) for u, v in zip(park.sequence_kv(1), park.sequence_kv(2)))
    all_ms = {name: {str(s): [] for s in SUFFIXES} for name in routes}
    for r in range(REPEATS + 1):                                             # (the first round warms every shape up, not reported)
        for s in SUFFIXES:
            for name, route in routes.items():
                ts = []
                for c in range(CALLS):
                    park.fork(0, [1])
                    ts.append(timed(lambda: route(park, 1, qrows[:1, :, :s], rows[:1, :, :s])))
                if r:
                    all_ms[name][str(s)].append(statistics.mean(ts))
    # the 64-row suffix as one-row replayed steps of the forked slot
    all_ms["suffix_as_steps_per_row"] = []
    nan = torch.full_like(rows[:, :, :1], float("nan"))
    for r in range(REPEATS + 1):
        park.release(list(range(1, N)))
        park.fork(0, [1])
        park.resume([1])
        fed = []
        for i in range(64):                                                   # (the paused slots are fed NaN: nothing reads it)
            qi, ki = nan.clone(), nan.clone()
            qi[1], ki[1] = qrows[0, :, i:i + 1], rows[0, :, i:i + 1]
            fed.append((qi, ki))
        def steps():
            for qi, ki in fed:
                park.step(qi, ki, ki)
        t = timed(steps)
        if r:
            all_ms["suffix_as_steps_per_row"].append(t / 64)
    del park
    # all-active steps: contiguous, paged, and four rows at a time
    sessions = {"step_contiguous": (DecodeSession.from_sequences(layer.attention, [A] * N, CAP), 1),
                "step_paged": (DecodeSession.from_sequences(layer.attention, [A] * N, CAP, page_rows=PAGE), 1),
                "step_rows4": (DecodeSession.from_sequences(layer.attention, [A] * N, CAP, max_step_rows=8), 4)}
    def run(sess, s, i0, count):
        for i in range(i0, i0 + count):
            sess.step(qrows[:, :, i * s:(i + 1) * s], rows[:, :, i * s:(i + 1) * s], rows[:, :, i * s:(i + 1) * s])
    for name, (sess, s) in sessions.items():
        run(sess, s, 0, WARM)
        all_ms[name] = []
    for r in range(REPEATS):
        for name, (sess, s) in sessions.items():
            all_ms[name].append(timed(lambda: run(sess, s, WARM + r * STEPS, STEPS)) / STEPS)

med = lambda v: round(statistics.median(v), 4)
out = {"has_extend": has_extend, "suffixes": list(SUFFIXES), "prompt": T0, "page_rows": PAGE, "capacity": CAP, "slots": N,
       "repeats": REPEATS, "calls_per_repeat": CALLS, "steps": STEPS, "pages": pages}
for name in routes:
    out[f"{name}_ms"] = {s: _mmm(v) for s, v in all_ms[name].items()}
if has_extend:
    out["extend_over_existing"] = {str(s): round(med(all_ms["extend"][str(s)]) / med(all_ms["existing"][str(s)]), 3) for s in SUFFIXES}
    out["extend_ms_per_row_at_64"] = round(med(all_ms["extend"]["64"]) / 64, 5)
out["existing_ms_per_row_at_64"] = round(med(all_ms["existing"]["64"]) / 64, 5)
out["one_row_steps_ms_per_row"] = _mmm(all_ms["suffix_as_steps_per_row"])
for name in ("step_contiguous", "step_paged", "step_rows4"):
    out[f"{name}_ms"] = _mmm(all_ms[name])
out["all_ms"] = {n: ({s: [round(t, 4) for t in v] for s, v in vals.items()} if isinstance(vals, dict) else [round(t, 4) for t in vals])
                 for n, vals in all_ms.items()}
print(json.dumps(out))
