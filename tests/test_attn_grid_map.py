"""The attention grid's block map on the host (no GPU): `ops.attention_grid_map` runs the function the kernels run on their
workgroup index (`map_block`, csrc/sea_attn.hpp) for every index of a launch.

Bars, for every order and every number G of interleaved pairs: the workgroups with work are exactly {0 .. NH-1} x {0 .. TB-1},
each once (a skipped or doubled row block is the one way an order can go wrong); the pairs of the full groups of eight stay
congruent to the workgroup index modulo 8 (a pair's K / V stay in one XCD's L2); and each order is what DESIGN 6.4 says it is."""
import numpy as np
import pytest

from sea_attention_amd.perlin_attention import ops

NHS = (1, 3, 7, 8, 9, 12, 16, 24, 40, 256)
TBS = (1, 2, 5, 64, 512)


def _cases():
    for order in ops.GRID_ORDERS:
        for G in ops.GRID_GROUPS:
            yield order, G


@pytest.mark.parametrize("order,G", list(_cases()))
def test_every_row_block_once_and_pairs_stay_on_their_xcd(order, G):
    for NH in NHS:
        for TB in TBS:
            pair, tb, work = ops.attention_grid_map(NH, TB, order, G)
            blocks = 8 * ((NH + 7) // 8) * TB
            assert pair.shape == tb.shape == work.shape == (blocks,)
            w = work != 0
            assert int(w.sum()) == NH * TB, (NH, TB)
            assert pair[w].min() >= 0 and pair[w].max() < NH and tb[w].min() >= 0 and tb[w].max() < TB
            key = pair[w].astype(np.int64) * TB + tb[w]
            assert np.array_equal(np.sort(key), np.arange(NH * TB)), (NH, TB)
            bid = np.arange(blocks)
            full = w & (pair < (NH // 8) * 8)
            assert np.array_equal(pair[full] % 8, bid[full] % 8), (NH, TB)
            # the full groups come first, nothing idle among them; the idle workgroups are the tail of the partial group's deal
            assert bool(w[:(NH // 8) * 8 * TB].all())


def test_ascending_is_the_order_before_grid_orders():
    """pair = 8 * (slot // TB) + xcd, tb = slot % TB in the full groups; the partial group dealt round-robin over the XCDs."""
    for NH in NHS:
        for TB in TBS:
            for G in ops.GRID_GROUPS:                                   # (G is not read in this order)
                pair, tb, work = ops.attention_grid_map(NH, TB, "ascending", G)
                bid = np.arange(pair.size)
                xcd, slot = bid & 7, bid >> 3
                full = NH // 8
                infull = slot // TB < full
                assert np.array_equal(pair[infull], (slot // TB * 8 + xcd)[infull]) and np.array_equal(tb[infull], (slot % TB)[infull])
                item = (slot - full * TB) * 8 + xcd
                part = ~infull & (item < (NH - full * 8) * TB)
                assert np.array_equal(work != 0, infull | part)
                assert np.array_equal(pair[part], (full * 8 + item // TB)[part]) and np.array_equal(tb[part], (item % TB)[part])


@pytest.mark.parametrize("NH,TB", [(16, 5), (24, 64), (40, 2), (256, 64), (12, 5), (3, 64)])
def test_heavy_first_reverses_the_row_blocks_and_is_grouped_by_one(NH, TB):
    pa, ta, wa = ops.attention_grid_map(NH, TB, "ascending", 1)
    for G in ops.GRID_GROUPS:
        ph, th, wh = ops.attention_grid_map(NH, TB, "heavy-first", G)
        assert np.array_equal(wa, wh) and np.array_equal(pa[wa != 0], ph[wa != 0])
        assert np.array_equal(th[wa != 0], TB - 1 - ta[wa != 0])
    pg, tg, wg = ops.attention_grid_map(NH, TB, "grouped", 1)
    assert np.array_equal(pg, ph) and np.array_equal(tg, th) and np.array_equal(wg, wh)


@pytest.mark.parametrize("G", [2, 4])
@pytest.mark.parametrize("NH,TB", [(24, 5), (40, 64), (256, 64), (16, 1)])
def test_grouped_interleaves_g_pairs_heaviest_block_first(NH, TB, G):
    """XCD x walks its pairs G at a time: slot s of a group of c pairs is pair s % c of the group, row block TB - 1 - s // c;
    the last group of an XCD holds what is left (3 pairs against G = 2: two, then one; 5 against 4: four, then one)."""
    pair, tb, work = ops.attention_grid_map(NH, TB, "grouped", G)
    full = NH // 8
    for xcd in (0, 5):
        mine = np.arange(xcd, 8 * full * TB, 8)
        slot = 0
        for g0 in range(0, full, G):
            c = min(G, full - g0)
            for s in range(c * TB):
                b = mine[slot + s]
                assert work[b] and pair[b] == (g0 + s % c) * 8 + xcd and tb[b] == TB - 1 - s // c, (xcd, g0, s)
            slot += c * TB


def test_the_group_rule_keeps_the_interleaved_pairs_inside_half_an_l2():
    import torch
    assert ops.grid_group_rule(torch.bfloat16, 64, 4096) == 2          # the headline: 1 MiB of K + V a pair
    assert ops.grid_group_rule(torch.bfloat16, 128, 4096) == 1         # 2 MiB
    assert ops.grid_group_rule(torch.bfloat16, 80, 8192) == 1          # OPT-2.7B: 2.6 MiB
    assert ops.grid_group_rule(torch.bfloat16, 64, 2048) == 4
    assert ops.grid_group_rule(torch.float32, 64, 4096) == 1
    assert ops.grid_group_rule(torch.bfloat16, 64, 32768) == 1         # beyond the L2 altogether: one pair at a time


def test_the_layers_default_order_follows_the_measured_shapes():
    """`ops.grid_order_default` (what PerlinAttention.attention_grid_order = "auto" passes): DESIGN 6.4's table."""
    import torch
    from sea_attention_amd.perlin_attention import attention as A
    assert A.ATTENTION_GRID_ORDER == "auto"
    for dtype in (torch.bfloat16, torch.float16):
        assert ops.grid_order_default(dtype, 64, 4096) == ("grouped", 2)       # OPT-1.3B
        assert ops.grid_order_default(dtype, 128, 4096) == "heavy-first"       # LLaMA-13B: two pairs would fill the L2
        assert ops.grid_order_default(dtype, 80, 8192) == "heavy-first"        # OPT-2.7B
        assert ops.grid_order_default(dtype, 64, 2048) is None                 # OPT-125m: no gain measured
        assert ops.grid_order_default(dtype, 64, 32768) is None                # a pair beyond the L2: no gain measured
    for d in (32, 64, 128):
        assert ops.grid_order_default(torch.float32, d, 4096) is None


def test_bad_orders_are_refused_on_the_host():
    import torch
    from sea_attention_amd.perlin_attention.ops import flat_csr
    for bad in ("descending", ("grouped", 3), ("heavy-first", 2), ("grouped", 8)):
        with pytest.raises(ValueError, match="grid_order"):
            flat_csr._grid_order_flags(bad, torch.bfloat16, 64, 4096)
    assert flat_csr._grid_order_flags(None, torch.bfloat16, 64, 4096) == 0
    assert flat_csr._grid_order_flags("ascending", torch.bfloat16, 64, 4096) == 0
    assert flat_csr._grid_order_flags("grouped", torch.bfloat16, 64, 4096) == (2 << 16) | (1 << 18)
    assert flat_csr._grid_order_flags(("grouped", 4), torch.bfloat16, 64, 4096) == (2 << 16) | (2 << 18)
    with pytest.raises(RuntimeError, match="sea_attention_grid_map"):
        ops.attention_grid_map(8, 4, "grouped", 3)
