#!/usr/bin/env python3
"""The weight-stationary convolution (causal_conv_ring_kernel) against the register form it replaces, plus the new form's
timing-only builds (WRONG results on purpose) that drop one resource each:
   ring            the product build (64 -> 64 channel, W = 64 launches with >= 16 rows per CU take the new form)
   noring          -DSEA_CONV_NO_RING: every launch on causal_conv_c8_kernel (the parent's code)
   ring_noload     no LDS-DMA fills (the ring keeps whatever it holds: MFMA + LDS reads + stores)
   ring_nostore    no output stores
   ring_bare       neither
`--build` here, then run on the GPU box; two interleaved rounds, one child process per (round, build)."""
import json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
VARIANTS = {"ring": [], "noring": ["-DSEA_CONV_NO_RING"], "ring_noload": ["-DSEA_CONV_RING_EXP_NOLOAD"],
            "ring_nostore": ["-DSEA_CONV_RING_EXP_NOSTORE"],
            "ring_bare": ["-DSEA_CONV_RING_EXP_NOLOAD", "-DSEA_CONV_RING_EXP_NOSTORE"]}
SHAPES = {"opt13b_x8": (8, 64, 4096), "opt27b_x1": (1, 64, 8192), "opt13b_x1": (1, 64, 4096), "x1_t2048": (1, 64, 2048),
          "llama13b_x1": (1, 80, 4096), "opt125m_x8": (8, 24, 2048)}
def lib(v):
    if v == "ring": return os.path.join(ROOT, "sea-attention_amd", "libsea_hip.so")   # the product build
    return os.path.join(ROOT, "sea-attention_amd", "build", f"libsea_hip_convr_{v}.so")
if "--build" in sys.argv:
    from sea_attention_amd import _build
    for v, fl in VARIANTS.items():
        if "--only" in sys.argv and v not in sys.argv: continue
        print(_build.build_library(extra_flags=tuple(fl), out=lib(v)) if fl else _build.ensure_built(), flush=True)
elif "--one" in sys.argv:
    import torch
    from sea_attention_amd.perlin_attention import ops
    res = {}
    for name, (N, C, T) in SHAPES.items():
        torch.manual_seed(0)
        x = ops.to_c8(torch.relu(torch.randn((N, C, T, 64), device="cuda")).to(torch.bfloat16))
        wt = (torch.randn((C, C, 5, 3), device="cuda") * 0.04).to(torch.bfloat16); b = torch.zeros(C, device="cuda", dtype=torch.bfloat16)
        for _ in range(5): y = ops.causal_conv_c8(x, wt, b, 3, 2, 2)
        torch.cuda.synchronize()
        best = 1e9
        for rep in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(20): y = ops.causal_conv_c8(x, wt, b, 3, 2, 2)
            e1.record(); torch.cuda.synchronize()
            best = min(best, e0.elapsed_time(e1) / 20 * 1e3)
        res[name] = [round(best, 1), float(y.float().abs().sum())]
    print(json.dumps(res))
else:
    names = [v for v in VARIANTS if len(sys.argv) < 2 or v in sys.argv[1:]]
    for rnd in range(2):
        for v in names:
            env = dict(os.environ, SEA_HIP_LIB=lib(v))
            out = subprocess.run([sys.executable, __file__, "--one"], env=env, capture_output=True, text=True, timeout=300)
            if out.returncode != 0:
                print(v, "rc", out.returncode, out.stderr[-600:], flush=True)
                sys.exit(1)
            print(v, out.stdout.strip().splitlines()[-1], flush=True)
