#!/usr/bin/env python3
"""List-scheduling model of one XCD under the attention grid orders (no GPU): workgroups are dispatched in index
order to the first free of `slots` slots; a causal row block's work is proportional to its pool's mean t (the blocks of a pool
are about equal: their rows are dealt over the whole pool) plus a fixed cost per block.  Prints makespan / ideal per order.
The model lets a block run equally fast on a full and on a draining XCD: an upper bound on what an order can win.

    python scripts/sim_attn_grid_order.py [pairs per XCD] [blocks per pair] [blocks per pool] [slots] [fixed share]"""
import heapq
import sys


def weights(TB, per_pool, fixed):
    pools = max(1, TB // per_pool)
    return [fixed + 2.0 * (min(tb // per_pool, pools - 1) + 0.5) / pools for tb in range(TB)]      # mean 1 + fixed


def orders(pairs, TB):
    yield "ascending", [(p, tb) for p in range(pairs) for tb in range(TB)]
    yield "heavy-first", [(p, tb) for p in range(pairs) for tb in reversed(range(TB))]
    for G in (2, 3, 4):
        seq = []
        for g0 in range(0, pairs, G):
            grp = range(g0, min(pairs, g0 + G))
            seq += [(p, tb) for tb in reversed(range(TB)) for p in grp]
        yield f"grouped G={G}", seq


def makespan(seq, w, slots):
    free = [0.0] * slots
    heapq.heapify(free)
    end = 0.0
    for _p, tb in seq:
        t = heapq.heappop(free) + w[tb]
        end = max(end, t)
        heapq.heappush(free, t)
    return end


def main():
    a = sys.argv[1:]
    pairs, TB = int(a[0]) if a else 32, int(a[1]) if len(a) > 1 else 64
    per_pool, slots = int(a[2]) if len(a) > 2 else 8, int(a[3]) if len(a) > 3 else 128
    fixed = float(a[4]) if len(a) > 4 else 0.08
    w = weights(TB, per_pool, fixed)
    ideal = pairs * sum(w) / slots
    print(f"pairs per XCD {pairs}, blocks per pair {TB} in pools of {per_pool}, {slots} slots, fixed cost {fixed} of the mean block")
    for name, seq in orders(pairs, TB):
        print(f"  {name:14s} makespan / ideal = {makespan(seq, w, slots) / ideal:.3f}")


if __name__ == "__main__":
    main()
