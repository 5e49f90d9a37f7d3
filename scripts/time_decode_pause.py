#!/usr/bin/env python3
"""What sitting-out slots cost and save (DecodeSession.pause / resume) at OPT-1.3B shape (H = 32, d = 64, T_M = 256, k = 64,
bf16, N = 8, lengths spread over 1000 .. 4000: the shape of time_decode_ragged.py), contiguous and paged K / V.

    python scripts/time_decode_pause.py [--parent-lib /path/to/the/parent/commit's/libsea_hip.so] [--this-first]

One child process per measurement.  (a) runs the SAME procedure -- all eight slots active, nothing paused or resumed in
between -- once per build: this tree's library and, with --parent-lib, that one loaded through SEA_HIP_LIB (the all-active
step needs nothing of this change).  (b) and (c) run in a third process on this tree's library.  In each process, after a
warm-up, the setups alternate inside every repeat; ms per position as min / median / max over the repeats, one JSON line:
  (a) all eight slots active, per build: the common path must cost what it cost;
  (b) 4 of 8 and 7 of 8 slots paused, against all-active in the same process, and an N = 1 session at the longest length
      for scale;
  (c) one pause + resume pair between steps: host time of the two calls and stream time (events around them)."""
import json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
N, H, d, T0, T_M, k, PAGE = 8, 32, 64, 4000, 256, 64, 64
WARM, STEPS, REPEATS = 4, int(os.environ.get("STEPS", 16)), int(os.environ.get("REPEATS", 5))
LENGTHS = [1000 + (T0 - 1000) * i // (N - 1) for i in range(N)]             # 1000 ... 4000


def spread(v):
    return {"min": round(min(v), 4), "median": round(statistics.median(v), 4), "max": round(max(v), 4)}


def child(with_pauses):
    import torch
    import sea_attention_amd as S
    from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
    from sea_attention_amd.perlin_attention.decode import DecodeSession
    kinds = ["contiguous", "paged"]
    paused_sets = {"all_active": [], "paused_4_of_8": [1, 3, 5, 7], "paused_7_of_8": list(range(7))} if with_pauses else {"all_active": []}
    total = WARM + STEPS * REPEATS
    CAP = T0 + WARM + 3 * STEPS * REPEATS + 1                    # (the same in both builds: a session steps up to three setups per repeat)
    dev, dt = "cuda:0", torch.bfloat16

    class Cfg:
        hidden_size, num_attention_heads, max_position_embeddings = H * d, H, CAP
    S.seed(42)
    pc = PerlinAttentionConfig(k=k, attention_predictor_length=T_M, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix', use_cache=True)
    layer = PerlinSelfAttention(Cfg(), pc).to(dev).to(dt).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = True
    layer.attention.context_layer_dtype = dt
    x = torch.randn((N, H, T0, d), device=dev).to(dt)
    q = (x.float() * d ** -0.5).to(dt)
    rows = torch.randn((N, H, total, d), device=dev).to(dt)
    qrows = (rows.float() * d ** -0.5).to(dt)
    fp_min = torch.finfo(torch.float16).min / 2

    def mask(T):
        r = torch.arange(T, device=dev)
        return ((r.view(1, T) > r.view(T, 1)) * fp_min).view(1, 1, T, T).to(dt)

    def prefill(xs, qs, L):
        out = layer(None, None, None, query_layer=qs[:, :, :L], key_layer=xs[:, :, :L], value_layer=xs[:, :, :L], attention_mask=mask(L))
        return out.state, xs[:, :, :L], xs[:, :, :L]

    with torch.no_grad():
        seqs = [prefill(x[n:n + 1], q[n:n + 1], L) for n, L in enumerate(LENGTHS)]
        sessions = {"contiguous": DecodeSession.from_sequences(layer.attention, seqs, CAP),
                    "paged": DecodeSession.from_sequences(layer.attention, seqs, CAP, page_rows=PAGE)}
        single = DecodeSession.from_sequences(layer.attention, seqs[-1:], CAP)
        del seqs

        def run(sess, lo, hi):
            n = sess.N
            for i in range(lo, hi):
                sess.step(qrows[:n, :, i:i + 1], rows[:n, :, i:i + 1], rows[:n, :, i:i + 1])

        def timed(sess, lo, hi):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run(sess, lo, hi)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) / (hi - lo) * 1e3

        for sess in list(sessions.values()) + [single]:
            run(sess, 0, WARM)
        times = {}
        for r in range(REPEATS):
            lo = WARM + r * STEPS
            for kind in kinds:
                sess = sessions[kind]
                for name, out in paused_sets.items():
                    if out:
                        sess.pause(out)
                    times.setdefault(f"{kind}_{name}", []).append(timed(sess, lo, lo + STEPS))
                    if out:
                        sess.resume(out)
            times.setdefault("single_longest", []).append(timed(single, lo, lo + STEPS))
        result = {"ms_per_position": {name: spread(v) for name, v in times.items()},
                  "all_ms": {name: [round(t, 4) for t in v] for name, v in times.items()}}
        if with_pauses:                                            # (c) a pause + resume pair between steps
            sess = sessions["contiguous"]
            host, stream = [], []
            for _ in range(20):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                t0 = time.perf_counter()
                sess.pause([3])
                sess.resume([3])
                host.append((time.perf_counter() - t0) * 1e3)
                e1.record()
                torch.cuda.synchronize()
                stream.append(e0.elapsed_time(e1))
            result["pause_resume_pair_ms"] = {"host": spread(host), "stream": spread(stream)}
            result["captures"] = {kind: s.captures for kind, s in sessions.items()}
    print(json.dumps(result))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--child":
        return child(sys.argv[2] == "pauses")
    parent_lib = sys.argv[sys.argv.index("--parent-lib") + 1] if "--parent-lib" in sys.argv else None
    out = {"lengths": LENGTHS, "page_rows": PAGE, "steps": STEPS, "repeats": REPEATS}
    runs = [("parent_build", parent_lib, "plain"), ("this_build", None, "plain"), ("this_build_pauses", None, "pauses")]
    if "--this-first" in sys.argv:                                 # (the order of the two (a) processes, to see what the order does)
        runs[0], runs[1] = runs[1], runs[0]
    out["order"] = [r[0] for r in runs]
    for name, lib, mode in runs:
        if name == "parent_build" and lib is None:
            continue
        env = dict(os.environ)
        env.pop("SEA_HIP_LIB", None)
        if lib:
            env["SEA_HIP_LIB"] = os.path.abspath(lib)
        res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", mode], env=env,
                             capture_output=True, text=True, timeout=900)
        if res.returncode != 0:
            sys.stderr.write(res.stderr)
            sys.exit(f"{name}: child exited with {res.returncode}")
        out[name] = json.loads(res.stdout.strip().splitlines()[-1])
    if "parent_build" in out:                                      # the bar: this build's median inside the parent's own spread
        for kind in ("contiguous", "paged"):
            new = out["this_build"]["ms_per_position"][f"{kind}_all_active"]
            old = out["parent_build"]["ms_per_position"][f"{kind}_all_active"]
            out[f"{kind}_all_active_median_within_parent_spread"] = old["min"] <= new["median"] <= old["max"] or new["median"] < old["min"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
