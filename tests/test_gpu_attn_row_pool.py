"""-m gpu: the row-pool form of the fused attention launch (`ops.sparse_attention(row_pool=...)`): a pre-pass sorts every pool of
query rows of a (n, h) by length and the gather kernels deal their rows to waves from that order instead of ranking the 64 / 32
rows of their own workgroup.

Bars: which lane group walks a row changes no bit -- the context rows and (with the columns written) the CSR's column array
equal those of the same launch without the field, `torch.equal`; and the order the pre-pass leaves in its workspace is, per
(n, h, pool), a permutation of the pool's slots with non-increasing row lengths, the slots past T_dst last.
Every shape has more than `attention_few_rows()` rows (below that the field is ignored: tests/test_attn_row_pool_host.py, which
also holds the refused argument combinations -- they return on the host)."""
import pytest
import torch

from oracle import sea_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
POOLS = (128, 256, 512)

# name: (N, H, T_dst, T_src, T_M, k, how the map is bent)
SHAPES = {
    "partial_last_pool_h3_n2": (2, 3, 700, 700, 64, 16, None),        # head rotation (H = 3, N = 2); 700 = 512 + 188 = 5 * 128 + 60
    "blocks_without_rows": (1, 4, 1100, 1100, 64, 16, None),          # 1100 = 2 * 512 + 76: most blocks of the last pool hold no row
    "one_partial_pool": (2, 8, 130, 130, 64, 16, None),               # 130 rows in one pool of 512 (and 128 + 2)
    "prefix_rows": (1, 6, 400, 2100, 64, 16, None),                   # T_dst < T_src: the last rows of a long prefix
    "empty_pairs": (1, 4, 700, 700, 64, 16, "empty"),                 # (row, head) pairs without an entry
    "one_head_takes_all": (1, 9, 1024, 1024, 64, 64, "one_head"),     # lists beyond the LDS list, lengths (<= ~k * H) beyond the last bin
}


@pytest.fixture(scope="module")
def ops():
    from sea_attention_amd.perlin_attention import ops
    return ops


def _inputs(N, H, T_dst, T_src, d, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn((N, H, T_dst, d), generator=g) * d ** -0.5).to(dtype).to(DEV)
    k = torch.randn((N, H, T_src, d), generator=g).to(dtype).to(DEV)
    v = torch.randn((N, H, T_src, d), generator=g).to(dtype).to(DEV)
    rs = torch.sigmoid(torch.randn((N, H, T_dst), generator=g)).to(DEV)
    mx = torch.sigmoid(torch.randn((N, H, T_dst), generator=g)).to(DEV)
    avg = torch.randn((N, H, T_dst, d), generator=g).to(dtype).to(DEV)
    return q, k, v, rs, mx, avg


_SELECTIONS = {}


def _selection(ops, name):
    """The shape's selection, made once: (bits, row_nnz, head_off, z_cap, reference columns, crow)."""
    if name not in _SELECTIONS:
        N, H, T_dst, T_src, T_M, k, bend = SHAPES[name]
        g = torch.Generator().manual_seed(11)
        probs = torch.softmax(torch.randn((N, H, T_dst, T_M), generator=g), -1)
        if bend == "empty":
            probs[:, 0, ::3] -= 20.0                                          # head 0 keeps nothing in every third row
            probs[:, 2, 100:164] -= 20.0                                      # head 2 nothing in a whole 64-row block
        elif bend == "one_head":
            probs[:, 1] += 10.0                                               # head 1 wins every pixel the row may keep
        keep = O.keep_counts_module(H, T_src, T_M, k)[-T_dst:].clamp_max(H * T_M).to(torch.int32).contiguous().to(DEV)
        csr0, _ = ops.topk_to_csr(probs.to(DEV), keep, k, target_width=T_src)
        _SELECTIONS[name] = csr0
    return _SELECTIONS[name]


def _pending(ops, name):
    N, H, T_dst, T_src, T_M, k, _ = SHAPES[name]
    c = _selection(ops, name)
    csr = ops.csr_from_selection(c.bits, c.row_nnz, c.head_off, H, T_M, T_src, k, True, c._col.shape[1], defer_emit=True)
    assert csr.col_is_pending
    csr._col.fill_(-7)
    return csr


def _lengths(csr, N, H, T_dst):
    ho = csr.head_off.long().view(N, T_dst, H + 1).cpu()
    return (ho[:, :, 1:] - ho[:, :, :-1]).permute(0, 2, 1).contiguous()       # (N, H, T_dst)


def _check_order(order, lens, T_dst, pool):
    """order (N, H, pools * pool) as the launch left it; lens (N, H, T_dst)."""
    N, H, _ = lens.shape
    pools = -(-T_dst // pool)
    o = order.cpu().long().view(N, H, pools, pool)
    assert torch.equal(o.sort(-1).values, torch.arange(pool).expand(N, H, pools, pool)), "a permutation of the pool's slots"
    padded = torch.full((N, H, pools * pool), -1, dtype=torch.long)
    padded[:, :, :T_dst] = lens
    dealt = padded.view(N, H, pools, pool).gather(-1, o)
    assert bool((dealt[..., 1:] <= dealt[..., :-1]).all()), "lengths non-increasing, the slots past T_dst last"


@pytest.mark.parametrize("dtype,d", [(torch.bfloat16, 64), (torch.float16, 64), (torch.bfloat16, 80), (torch.float16, 80),
                                     (torch.bfloat16, 128), (torch.float16, 128)])
@pytest.mark.parametrize("name", list(SHAPES))
def test_pooled_launch_equals_the_launch_without_pools(ops, name, dtype, d):
    N, H, T_dst, T_src, T_M, k, bend = SHAPES[name]
    assert N * H * T_dst > ops.attention_few_rows()
    q, kk, v, rs, mx, avg = _inputs(N, H, T_dst, T_src, d, dtype, 5)
    sel = _selection(ops, name)
    lens = _lengths(sel, N, H, T_dst)
    if bend == "empty":
        assert int((lens == 0).sum()) > 64
    if bend == "one_head":
        assert int((lens > 510).sum()) > 64                                   # rows beyond the histogram's last bin, of several lengths
        assert lens[lens > 510].unique().numel() > 8
        assert int(lens[0, 1, 512:].sum()) // 16 > 8192                       # the mean block of the last 512-pool (8 or 16 blocks) overflows the LDS list
    refs = {}
    for out_dtype in (torch.float32, dtype):
        csr = _pending(ops, name)
        refs[out_dtype] = ops.sparse_attention(q, kk, v, csr, row_scale=rs, avg=avg, mix=mx, path="gather", out_dtype=out_dtype)
        assert not csr.col_is_pending
        ref_col = csr._col.clone()
    for pool in POOLS:
        for out_dtype in (torch.float32, dtype):
            for write_cols in (1, 0):
                csr = _pending(ops, name)
                ws = ops.row_pool_workspace(N, H, T_dst, pool, torch.device(DEV))
                ws.fill_(-1)
                out = ops.sparse_attention(q, kk, v, csr, row_scale=rs, avg=avg, mix=mx, path="gather", out_dtype=out_dtype,
                                           row_pool=pool, keep_columns_pending=not write_cols)
                assert out.dtype == out_dtype and torch.equal(out, refs[out_dtype]), (pool, out_dtype, write_cols)
                if write_cols:
                    assert not csr.col_is_pending
                    for n in range(N):
                        z = int(csr.crow[n, -1])
                        assert torch.equal(csr._col[n, :z], ref_col[n, :z]), (pool, n)
                else:
                    assert csr.col_is_pending
                _check_order(ops.row_pool_workspace(N, H, T_dst, pool, torch.device(DEV)), lens, T_dst, pool)


def test_row_pool_is_ignored_where_the_form_does_not_exist(ops):
    """Probabilities wanted, or a launch of few rows: the call runs as without `row_pool`; a pool the head size does not take raises."""
    name = "partial_last_pool_h3_n2"
    N, H, T_dst, T_src, T_M, k, _ = SHAPES[name]
    q, kk, v, rs, mx, avg = _inputs(N, H, T_dst, T_src, 64, torch.bfloat16, 5)
    o1, p1 = ops.sparse_attention(q, kk, v, _pending(ops, name), row_scale=rs, path="gather", want_probs=True)
    o2, p2 = ops.sparse_attention(q, kk, v, _pending(ops, name), row_scale=rs, path="gather", want_probs=True, row_pool=512)
    assert torch.equal(o1, o2) and torch.equal(p1, p2)
    few = 100                                                                  # 2 * 3 * 100 rows: the few-row pair of launches
    sub_q = q[:, :, :few].contiguous()
    g = torch.Generator().manual_seed(1)
    probs = torch.softmax(torch.randn((N, H, few, T_M), generator=g), -1).to(DEV)
    keep = O.keep_counts_module(H, few, T_M, k).clamp_max(H * T_M).to(torch.int32).contiguous().to(DEV)
    small, _ = ops.topk_to_csr(probs, keep, k, target_width=few)
    a = ops.sparse_attention(sub_q, kk[:, :, :few].contiguous(), v[:, :, :few].contiguous(), small, path="gather")
    b = ops.sparse_attention(sub_q, kk[:, :, :few].contiguous(), v[:, :, :few].contiguous(), small, path="gather", row_pool=512)
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="row_pool"):
        ops.sparse_attention(q, kk, v, _pending(ops, name), path="gather", row_pool=32)
    with pytest.raises(ValueError, match="row_pool"):
        ops.sparse_attention(q, kk, v, _pending(ops, name), path="gather", row_pool=192)
