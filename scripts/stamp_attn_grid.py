#!/usr/bin/env python3
"""When the workgroups of the headline attention launch are resident, per XCD: a -DSEA_STAMP build of the library (lane 0 of
wave 0 of every workgroup of the lane-group kernels stamps the 100 MHz clock at entry and exit, and its XCC) under the fused
launch on the layer's own selection.  Per XCD: resident workgroups over time, the last dispatch, the end of the launch, and the
slot-time left idle between the two as a share of slots x launch time -- what a better grid order could win at most.
`--build` where hipcc is, then on the GPU:  python scripts/stamp_attn_grid.py [--order ascending|heavy-first|grouped] [--group G]
(WL / NB as scripts/time_attn_fused.py)."""
import argparse, ctypes, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, ROOT)
LIB = os.path.join(ROOT, "sea-attention_amd", "build", "libsea_hip_stamp.so")
ap = argparse.ArgumentParser()
ap.add_argument("--build", action="store_true")
ap.add_argument("--order", default="ascending")
ap.add_argument("--group", type=int, default=None)
ap.add_argument("--samples", type=int, default=24)
args = ap.parse_args()
if args.build:
    from sea_attention_amd import _build
    print(_build.build_library(extra_flags=("-DSEA_STAMP",), out=LIB))
    sys.exit(0)
if os.environ.get("SEA_HIP_LIB") != LIB:                  # the library path is read at import: run the measurement as a child
    sys.exit(subprocess.run([sys.executable, __file__, *sys.argv[1:]], env=dict(os.environ, SEA_HIP_LIB=LIB)).returncode)
import numpy as np
import torch
import sea_attention_amd as S
from bench import WORKLOADS, _Cfg
from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
from sea_attention_amd.perlin_attention import attention as A
w = WORKLOADS[os.environ.get("WL", "opt-1.3b")]; H, d, T, T_M, k = w["H"], w["d"], w["T"], w["T_M"], w["k"]
NB, dev, dt = int(os.environ.get("NB", 8)), "cuda:0", torch.bfloat16
S.seed(42)
pc = PerlinAttentionConfig(k=k, attention_predictor_length=T_M, performer_nb_factor=w["nbf"], causal=True, k_flatten=True,
                           k_flatten_dim='causal_batch', context_output_method='mix')
layer = PerlinSelfAttention(_Cfg(H * d, H, T), pc).to(dev).to(dt).eval()
for m in layer.modules():
    if hasattr(m, 'benchmarking'): m.benchmarking = True
layer.attention.context_layer_dtype = dt
layer.attention.assume_not_padded = True
S.seed(7)
x = torch.randn((NB, H, T, d), device=dev)
q, kk, v = (x * d ** -0.5).to(dt), torch.randn_like(x).to(dt), torch.randn_like(x).to(dt)
fp_min = torch.finfo(torch.float16).min / 2
mask = ((torch.arange(T, device=dev).view(1, T) > torch.arange(T, device=dev).view(T, 1)) * fp_min).view(1, 1, T, T).to(dt).expand(NB, 1, T, T)
seen = {}
real = A.ops.sparse_attention
def spy(q_, k_, v_, csr, **kw):
    seen.update(q=q_, k=k_, v=v_, csr=csr, kw=dict(kw), pending=csr._pending)
    return real(q_, k_, v_, csr, **kw)
A.ops.sparse_attention = spy
with torch.no_grad():
    layer(None, None, None, query_layer=q, key_layer=kk, value_layer=v, attention_mask=mask)
A.ops.sparse_attention = real
csr, kw = seen["csr"], seen["kw"]
kw["grid_order"] = (args.order, args.group) if args.group else args.order
def run():
    csr._pending = seen["pending"]
    return real(seen["q"], seen["k"], seen["v"], csr, **kw)
lib = _lib.load()
fn = lib.sea_debug_attn_grid_stamps
fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_int64], ctypes.c_int
rpb = 32 if d > 64 and d != 80 else 64
pool = kw.get("row_pool")
TB = -(-T // pool) * (pool // rpb) if pool else -(-T // rpb)
blocks = 8 * ((NB * H + 7) // 8) * TB
buf = np.zeros((blocks, 3), dtype=np.uint64)
for _ in range(3): run()
torch.cuda.synchronize()
assert fn(buf.ctypes.data, blocks) == 0                    # (reads and clears: the warm-up launches' stamps go)
run()
torch.cuda.synchronize()
assert fn(buf.ctypes.data, blocks) == 0
ent, ext, xcc = buf[:, 0].astype(np.int64), buf[:, 1].astype(np.int64), buf[:, 2].astype(np.int64)
assert (ent > 0).all() and (ext >= ent).all(), "every workgroup of the grid has stamped"
t0, t1 = ent.min(), ext.max()
us = lambda ticks: round(float(ticks) / 100, 1)            # 100 MHz
bid = np.arange(blocks)
print(json.dumps({"workload": os.environ.get("WL", "opt-1.3b"), "batch": NB, "order": args.order, "group": args.group, "row_pool": pool,
                  "blocks": blocks, "TB": TB, "launch_us": us(t1 - t0),
                  "xcc_is_bid_mod_8": round(float((xcc == (bid & 7)).mean()), 4),
                  "block_us_mean": us((ext - ent).mean()), "block_us_max": us((ext - ent).max())}))
idle_all, slots_all = 0.0, 0
for X in sorted(set(xcc.tolist())):
    m = xcc == X
    e, x_ = ent[m], ext[m]
    # resident workgroups at sample times, and the peak (the XCD's slots)
    ev = np.concatenate([np.stack([e, np.ones_like(e)], 1), np.stack([x_, -np.ones_like(x_)], 1)])
    ev = ev[np.lexsort((ev[:, 1], ev[:, 0]))]              # exits before entries at the same tick
    res = np.cumsum(ev[:, 1])
    slots = int(res.max())
    ts = np.linspace(t0, t1, args.samples + 1)[:-1]
    at = [int(res[np.searchsorted(ev[:, 0], t, side="right") - 1]) if t >= ev[0, 0] else 0 for t in ts]
    last = e.max()                                         # the XCD's last dispatch
    busy = np.clip(np.minimum(x_, t1) - np.maximum(e, last), 0, None).sum()
    idle = slots * (t1 - last) - busy                      # slot-time nobody used from the last dispatch to the launch's end
    idle_all += idle; slots_all += slots
    print(json.dumps({"xcc": int(X), "blocks": int(m.sum()), "slots": slots, "last_dispatch_us": us(last - t0), "xcd_end_us": us(x_.max() - t0),
                      "launch_end_us": us(t1 - t0), "idle_share_of_slots_x_launch": round(float(idle) / (slots * (t1 - t0)), 4),
                      "resident_at_%d_samples" % args.samples: at}))
print(json.dumps({"idle_share_all_xcds": round(idle_all / (slots_all * (t1 - t0)), 4),
                  "idle_us_of_launch": us(idle_all / slots_all)}))
