#!/usr/bin/env python3
"""Lane-step efficiency of the gather attention kernels' lockstep walk on a CSR's `head_off`: the share of issued lane-steps
that carry an entry when a wave walks its rows for as long as its longest row lasts (steps of U = 4 entries), with the rows

  natural      in natural order,
  block        ranked inside the workgroup's own rows (rows_by_length: 64 rows of 8 lanes, 32 rows of 16 lanes),
  pool P       dealt from pools of P rows sorted by length (sparse_attention(row_pool=P)): wave w of the pool's block b takes
               the sorted slots (w * nb + b) * RPW .., nb = P / rows per workgroup,

for rows of 8 lanes (8 rows per wave) and of 16 lanes (4 rows per wave), and the entries a workgroup's key lists hold under
each (mean / max against the 8192 entries of the LDS list).  Host arithmetic on the lengths; the GPU only runs the layer once
to get its own selection.

  count_attn_lane_steps.py [workload] [batch] [T]      (default opt-1.3b 8; T overrides the workload's sequence length)
  count_attn_lane_steps.py --all                       (the headline, the other three BASELINE shapes and the 32768-token leg)"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
U, NWB, FUSE_CAP = 4, 8, 8192
POOLS = (128, 256, 512, 1024)


def efficiencies(cnt, lanes):
    """cnt (N, H, T) entries per (row, head), on the CPU; lanes per row 8 or 16."""
    N, H, T = cnt.shape
    rpw = 64 // lanes
    rpb = NWB * rpw
    total = float(cnt.sum())
    c4 = (cnt + U - 1) // U * U                                                  # the walk advances U entries at a time

    def pad(x, m, fill):                                                          # T up to a multiple of m: slots without a row
        r = (-T) % m
        return x if r == 0 else torch.cat([x, torch.full((N, H, r), fill, dtype=x.dtype)], -1)

    def eff(c):                                                                   # c (N, H, slots): consecutive rpw slots share a wave
        return total / (float(c.clamp_min(0).view(N, H, -1, rpw).amax(-1).sum()) * rpw)

    def lists(c):                                                                 # c (N, H, blocks, rpb) true lengths per workgroup
        s = c.clamp_min(0).sum(-1).float()
        return {"mean": round(float(s.mean()), 1), "max": int(s.max()), "over_cap": int((s > FUSE_CAP).sum())}

    out = {"natural": round(eff(pad(c4, rpw, -1)), 4)}
    blk = pad(c4, rpb, -1).view(N, H, -1, rpb).sort(-1, descending=True)
    out["block"] = round(eff(blk.values.reshape(N, H, -1)), 4)
    out["block_lists"] = lists(pad(cnt, rpb, -1).view(N, H, -1, rpb))
    for P in POOLS:
        if P % rpb:
            continue
        nb = P // rpb
        srt = pad(cnt, P, -1).view(N, H, -1, P).sort(-1, descending=True).values     # (N, H, pools, P) by true length
        out[f"pool_{P}"] = round(eff(((srt + U - 1) // U * U).reshape(N, H, -1)), 4)
        # block b of a pool: waves w = 0 .. NWB - 1 take slots (w * nb + b) * rpw ..
        dealt = srt.view(N, H, -1, NWB, nb, rpw).permute(0, 1, 2, 4, 3, 5).reshape(N, H, -1, rpb)
        out[f"pool_{P}_lists"] = lists(dealt)
    return out


def count(wname, NB, T=None):
    from bench import LayerBench
    dev = torch.device("cuda:0")
    lb = LayerBench(wname, NB, "bf16", dev, override=dict(T=T) if T else None)
    lb.layer.attention.sparse_kernel = "gather"
    csr = lb.forward().partial_attention_mask
    ho = csr.head_off.long().cpu()
    cnt = (ho[..., 1:] - ho[..., :-1]).permute(0, 2, 1).contiguous()              # (N, H, T)
    w = lb.w
    res = {"workload": wname, "batch": NB, "T": w["T"], "H": w["H"], "d": w["d"], "entries_per_row_head": round(float(cnt.float().mean()), 2),
           "std": round(float(cnt.float().std()), 2), "lanes_8": efficiencies(cnt, 8), "lanes_16": efficiencies(cnt, 16)}
    del lb
    torch.cuda.empty_cache()
    return res


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--all":
        legs = [("opt-1.3b", 8, None), ("opt-125m", 8, None), ("opt-2.7b", 1, None), ("llama-13b", 1, None), ("opt-125m", 1, 32768)]
    else:
        legs = [(sys.argv[1] if len(sys.argv) > 1 else "opt-1.3b", int(sys.argv[2]) if len(sys.argv) > 2 else 8,
                 int(sys.argv[3]) if len(sys.argv) > 3 else None)]
    for leg in legs:
        print(json.dumps(count(*leg)), flush=True)
