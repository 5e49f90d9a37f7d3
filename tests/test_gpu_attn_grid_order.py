"""-m gpu: the grid order of the prefill attention launches (`ops.sparse_attention(grid_order=...)`; csrc/sea_attn.hpp map_block):
in which order the workgroups of an XCD take the row blocks of its (n, h) pairs.  Rows are independent, so every order leaves
every output bit where the ascending order puts it.

Bars, for every order and every G: the context equals that of the launch without the field with `torch.equal` -- `out` is
filled with NaN before the launch, so a row block nobody took shows up -- and the CSR columns, where the launch writes them,
are equal as well.  (tests/test_attn_grid_map.py holds the map itself to "every row block exactly once" on the host.)

Shapes a and b as listed for this test hold 390 and 1600 (n, h, t) rows, not more than `attention_few_rows()` = 2048 as the
others do: such a launch keeps the ascending order whatever the field says.  They run as listed (the field must be harmless
there) and again at the smallest T_dst that lifts them over the threshold with a ragged last block (a2, b2), so that what they
are there for -- only a partial pair group; exactly one pair per XCD -- meets the orders."""
import pytest
import torch

from oracle import sea_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ORDERS = ("ascending", "heavy-first", ("grouped", 1), ("grouped", 2), ("grouped", 4), "grouped")
T_M, K = 64, 16

# name: (N, H, T_dst, T_src, row pools tried besides none)
SHAPES = {
    "a": (1, 3, 130, 130, ()),                    # only the partial pair group; a ragged last block (few rows: the field is ignored)
    "a2": (1, 3, 700, 700, (512,)),               # the same above attention_few_rows()
    "b": (1, 8, 200, 200, ()),                    # exactly one pair per XCD (few rows)
    "b2": (1, 8, 264, 264, (128,)),               # the same above attention_few_rows()
    "c": (2, 12, 700, 700, (128, 512)),           # full + partial groups; 3 pairs per XCD against G = 2 and 4; pools 128 and 512
    "d": (1, 6, 400, 2100, (128,)),               # a prefix (T_dst < T_src)
    "e": (1, 16, 320, 320, (128,)),               # d = 80
    "f": (1, 16, 320, 320, (128,)),               # d = 128, and the tile path at d = 64
    "g": (1, 12, 320, 320, ()),                   # fp32 data
}
FEW = {"a", "b"}


@pytest.fixture(scope="module")
def ops():
    from sea_attention_amd.perlin_attention import ops
    return ops


def _inputs(N, H, T_dst, T_src, d, dtype, seed=5):
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
    if name not in _SELECTIONS:
        N, H, T_dst, T_src, _ = SHAPES[name]
        g = torch.Generator().manual_seed(11)
        probs = torch.softmax(torch.randn((N, H, T_dst, T_M), generator=g), -1)
        keep = O.keep_counts_module(H, T_src, T_M, K)[-T_dst:].clamp_max(H * T_M).to(torch.int32).contiguous().to(DEV)
        _SELECTIONS[name] = ops.topk_to_csr(probs.to(DEV), keep, K, target_width=T_src)[0]
    return _SELECTIONS[name]


def _handle(ops, name, pending):
    N, H, T_dst, T_src, _ = SHAPES[name]
    c = _selection(ops, name)
    csr = ops.csr_from_selection(c.bits, c.row_nnz, c.head_off, H, T_M, T_src, K, True, c._col.shape[1], defer_emit=pending)
    assert csr.col_is_pending == pending
    if pending:
        csr._col.fill_(-7)
    return csr


def _run(ops, name, tensors, out_dtype, pending=True, **kw):
    """One launch into a NaN-filled `out`; returns (out, the handle)."""
    N, H, T_dst, T_src, _ = SHAPES[name]
    q, kk, v, rs, mx, avg = tensors
    csr = _handle(ops, name, pending)
    out = torch.full((N, H, T_dst, q.shape[-1]), float("nan"), dtype=out_dtype, device=DEV)
    res = ops.sparse_attention(q, kk, v, csr, row_scale=rs, avg=avg, mix=mx, out=out, **kw)
    assert res.data_ptr() == out.data_ptr()
    return out, csr


def _check_orders(ops, name, d, dtype, pools, path="gather", pending=True):
    N, H, T_dst, T_src, _ = SHAPES[name]
    assert (N * H * T_dst > ops.attention_few_rows()) == (name not in FEW)
    tensors = _inputs(N, H, T_dst, T_src, d, dtype)
    for out_dtype in dict.fromkeys((torch.float32, dtype)):
        ref, rcsr = _run(ops, name, tensors, out_dtype, pending, path=path)
        assert not bool(torch.isnan(ref).any())
        assert not rcsr.col_is_pending
        ref_col = rcsr._col.clone()
        for order in ORDERS:
            for pool in (None, *pools):
                for write_cols in ((1, 0) if pending else (1,)):
                    out, csr = _run(ops, name, tensors, out_dtype, pending, path=path, grid_order=order, row_pool=pool,
                                    keep_columns_pending=not write_cols)
                    assert torch.equal(out, ref), (name, d, dtype, out_dtype, order, pool, write_cols)
                    fused = pending and ops.fused_interp_supported(dtype, d, T_M, N * H * T_dst)
                    if write_cols or not fused:
                        assert not csr.col_is_pending
                        for n in range(N):
                            z = int(csr.crow[n, -1])
                            assert torch.equal(csr._col[n, :z], ref_col[n, :z]), (name, order, pool, n)
                    else:
                        assert csr.col_is_pending


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("name", ["a", "a2", "b", "b2", "c", "d"])
def test_every_order_gives_the_ascending_orders_bits_d64(ops, name, dtype):
    _check_orders(ops, name, 64, dtype, SHAPES[name][4])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_every_order_d80(ops, dtype):
    _check_orders(ops, "e", 80, dtype, SHAPES["e"][4])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_every_order_d128(ops, dtype):
    _check_orders(ops, "f", 128, dtype, SHAPES["f"][4])


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
def test_every_order_tile_path_d64(ops, dtype):
    """The MFMA tile kernel reads the column array: a handle whose columns are written, no pools."""
    _check_orders(ops, "f", 64, dtype, (), path="tile", pending=False)


@pytest.mark.parametrize("d", [32, 64, 128])
def test_every_order_fp32(ops, d):
    """fp32 data: rows of 8 and 16 lanes (the fused forms) and, at d = 128, the wave-per-row kernel behind an emit launch."""
    _check_orders(ops, "g", d, torch.float32, ())


def test_unfused_gather_launch_and_bad_orders(ops):
    """The lane-group kernel on written columns (no fused interpolation: it keeps the ascending order, the field must be
    harmless); an unknown order raises before anything is launched."""
    _check_orders(ops, "c", 64, torch.bfloat16, (), pending=False)
    tensors = _inputs(*SHAPES["b2"][:4], 64, torch.bfloat16)
    for bad in ("descending", ("grouped", 3)):
        with pytest.raises(ValueError, match="grid_order"):
            _run(ops, "b2", tensors, torch.float32, grid_order=bad)
