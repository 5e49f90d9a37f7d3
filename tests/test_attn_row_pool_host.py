"""The row-pool form of the fused `sea_sparse_attention` launch on the host (include/sea_hip.h, SEA_ATTN_ROW_POOL_SHIFT): no
new symbol -- `flags` bits 4..7 carry log2(POOL), `block_path` / `probs_stride_n` the uint16 order workspace.

  * the slot -> (block, wave, lane group) map of the gather kernels (`pooled_row`, csrc/sea_attn.hip), restated in numpy,
    hands every row of every pool to exactly one lane group, and a block that returns early holds no row;
  * every argument combination the form does not take is refused with SEA_EINVAL / SEA_EUNSUPPORTED and a message that names
    the form, before anything is launched (fake device addresses, never dereferenced).

No GPU: every call returns on the host."""
import ctypes

import numpy as np
import pytest
import torch

from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import ops

EINVAL, EUNSUPPORTED = -1, -2
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entry refuses first)
B = ctypes.c_void_p((1 << 20) + 4096)
WS = ctypes.c_void_p(1 << 24)
ODD = ctypes.c_void_p((1 << 20) + 8)             # not 16-byte aligned
N, H, T_DST, T_SRC = 2, 4, 700, 700              # 5600 rows: more than sea_attention_few_rows()
NWB = 8                                          # waves per workgroup of the fused gather kernels


# ---------------------------------------------------------------------------------------------- the dealing, in numpy
def deal(T_dst, pool, rpb, order):
    """rows[t] = how many lane groups walk query row t; order (pools, pool): per pool the rows' offsets, valid rows first."""
    rpw = rpb // NWB
    nb = pool // rpb
    pools = -(-T_dst // pool)
    walked = np.zeros(T_dst, dtype=np.int64)
    slots = np.zeros((pools, pool), dtype=np.int64)
    for tb in range(pools * nb):                 # the grid's row blocks of one (n, h)
        pl, b = divmod(tb, nb)
        rows = min(pool, T_dst - pl * pool)
        if b * rpw >= rows:                      # the block returns before any barrier: it must hold no row
            for w in range(NWB):
                for j in range(rpw):
                    assert pl * pool + order[pl, (w * nb + b) * rpw + j] >= T_dst
            continue
        for w in range(NWB):
            for j in range(rpw):
                s = (w * nb + b) * rpw + j
                assert 0 <= s < pool
                slots[pl, s] += 1
                t = pl * pool + order[pl, s]
                if t < T_dst:
                    walked[t] += 1
    return walked, slots


@pytest.mark.parametrize("pool", [128, 256, 512, 1024])
@pytest.mark.parametrize("rpb", [32, 64])
@pytest.mark.parametrize("T_dst", [1, 31, 130, 700, 1100, 2049])
def test_every_row_of_every_pool_is_dealt_exactly_once(pool, rpb, T_dst):
    rng = np.random.default_rng(pool + rpb + T_dst)
    pools = -(-T_dst // pool)
    order = np.zeros((pools, pool), dtype=np.int64)
    for pl in range(pools):                      # what the pre-pass leaves: rows by length, the slots past T_dst last
        rows = min(pool, T_dst - pl * pool)
        lens = rng.poisson(4, rows) * 16
        by_len = np.argsort(-lens, kind="stable")
        order[pl] = np.concatenate([by_len, rng.permutation(np.arange(rows, pool))])
    walked, slots = deal(T_dst, pool, rpb, order)
    assert (walked == 1).all()
    assert slots.max() <= 1
    for pl in range(pools):                      # every slot that holds a row lies in a block that runs
        rows = min(pool, T_dst - pl * pool)
        assert (slots[pl, :rows] == 1).all()


def test_a_wave_holds_neighbours_and_a_block_spans_the_range():
    """Wave w of block b takes the sorted slots (w * nb + b) * RPW ..: RPW neighbours, and the block's waves lie nb * RPW apart."""
    pool, rpb = 512, 64
    rpw, nb = rpb // NWB, pool // rpb
    for b in range(nb):
        first = [(w * nb + b) * rpw for w in range(NWB)]
        assert first == [b * rpw + w * nb * rpw for w in range(NWB)]
        assert first[0] < nb * rpw and first[-1] >= pool - nb * rpw


def test_pools_the_form_takes():
    bf, f32 = torch.bfloat16, torch.float32
    assert all(ops.row_pool_supported(bf, 64, p) for p in (64, 128, 256, 512, 1024))
    assert all(ops.row_pool_supported(bf, 80, p) for p in (64, 128, 512))
    assert ops.row_pool_supported(bf, 128, 32) and ops.row_pool_supported(f32, 64, 32) and ops.row_pool_supported(f32, 32, 64)
    assert not ops.row_pool_supported(bf, 64, 32) and not ops.row_pool_supported(bf, 80, 32) and not ops.row_pool_supported(f32, 32, 32)
    assert not ops.row_pool_supported(bf, 64, 2048) and not ops.row_pool_supported(bf, 64, 192) and not ops.row_pool_supported(bf, 64, 0)
    assert ops.row_pool_workspace_elems(2, 3, 700, 512) == 2 * 3 * 1024
    assert ops.row_pool_workspace_elems(1, 4, 1100, 128) == 4 * 9 * 128
    assert _lib.SEA_ATTN_ROW_POOL_SHIFT == 4


# ---------------------------------------------------------------------------------------------- the C boundary
def _s(*v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.sea_last_error().decode()


def need(pool, T_dst=T_DST):
    return H * -(-T_dst // pool) * pool


def call(lib, pool=512, bits=A, ws=WS, stride=None, probs=None, t_src_dev=None, table=None, page_rows=0, table_stride=0,
         dtype=_lib.SEA_BF16, D=64, T_dst=T_DST, out=B, path=1, range_keys=0, write_cols=0):
    st = _s(H * 4096 * D, 4096 * D, D)
    stride = need(pool, T_dst) if stride is None else stride
    flags = path | ((pool.bit_length() - 1) << _lib.SEA_ATTN_ROW_POOL_SHIFT) | (range_keys << 16)
    return lib.sea_sparse_attention(
        A, A, A, dtype, N, H, T_dst, T_SRC, D, st, st, st, A, A, 1 << 20, A, None, None, None, None, out, dtype, st, probs, stride,
        ws, flags, bits, 32, 1, 4, write_cols, t_src_dev, 0, table, table_stride, page_rows, None)


def test_row_pool_arguments_pass_the_forms_checks(lib):
    """A workspace of the right size, a pool the head size takes, bits: the form's own checks pass (what stops these calls is the
    entry's general alignment check, which runs after them and does not name the form)."""
    rp = "row-pool"
    for pool in (64, 128, 256, 512, 1024):
        assert call(lib, pool=pool, out=ODD) == EUNSUPPORTED
        assert "16-byte aligned" in _err(lib) and rp not in _err(lib)
    assert call(lib, out=ODD, stride=need(512) + 1) == EUNSUPPORTED and rp not in _err(lib)          # a larger stride is fine
    assert call(lib, pool=32, D=128, out=ODD) == EUNSUPPORTED and rp not in _err(lib)                # rows of 16 lanes: 32 per workgroup
    assert call(lib, pool=64, D=80, out=ODD) == EUNSUPPORTED and rp not in _err(lib)
    assert call(lib, pool=32, D=64, dtype=_lib.SEA_F32, out=ODD) == EUNSUPPORTED and rp not in _err(lib)
    assert call(lib, write_cols=1, out=ODD) == EUNSUPPORTED and rp not in _err(lib)


def test_row_pool_refusals(lib):
    rp = "row-pool form"
    assert call(lib, ws=None) == EINVAL and rp in _err(lib) and "workspace" in _err(lib)
    assert call(lib, ws=ODD) == EINVAL and rp in _err(lib) and "aligned" in _err(lib)
    assert call(lib, stride=need(512) - 1) == EINVAL and rp in _err(lib) and str(need(512)) in _err(lib) and str(need(512) - 1) in _err(lib)
    assert call(lib, pool=128, stride=need(128) - 1) == EINVAL and str(need(128)) in _err(lib)
    assert call(lib, t_src_dev=A) == EUNSUPPORTED and rp in _err(lib) and "t_src_dev" in _err(lib)
    assert call(lib, table=A, page_rows=64, table_stride=64) == EUNSUPPORTED and rp in _err(lib) and "block_table" in _err(lib)
    assert call(lib, probs=A) == EUNSUPPORTED and rp in _err(lib) and "probs_out" in _err(lib)
    assert call(lib, path=3, range_keys=100) == EUNSUPPORTED and rp in _err(lib) and "key-range" in _err(lib)
    assert call(lib, path=2) == EUNSUPPORTED and rp in _err(lib) and "tile" in _err(lib)
    assert call(lib, bits=None) == EUNSUPPORTED and rp in _err(lib) and "bits" in _err(lib)
    assert call(lib, pool=32) == EUNSUPPORTED and rp in _err(lib) and "multiple of the 64 rows" in _err(lib)
    assert call(lib, pool=32, D=80) == EUNSUPPORTED and rp in _err(lib) and "multiple of the 64 rows" in _err(lib)
    assert call(lib, pool=16, D=128) == EUNSUPPORTED and rp in _err(lib) and "multiple of the 32 rows" in _err(lib)
    assert call(lib, pool=2048) == EUNSUPPORTED and rp in _err(lib) and "1024" in _err(lib) and "2048" in _err(lib)
    assert call(lib, pool=1 << 15) == EUNSUPPORTED and rp in _err(lib) and "1024" in _err(lib)


def test_a_launch_of_few_rows_ignores_the_field(lib):
    """N * H * T_dst <= sea_attention_few_rows(): no workspace is asked for, the call goes on as without the field."""
    few = int(lib.sea_attention_few_rows())
    t = few // (N * H)
    assert call(lib, T_dst=t, ws=None, stride=0, out=ODD) == EUNSUPPORTED and "row-pool" not in _err(lib) and "16-byte aligned" in _err(lib)
    assert call(lib, T_dst=t + 1, ws=None, stride=0, out=ODD) == EINVAL and "row-pool" in _err(lib)
    # the forms that have no pools are refused whatever the size
    assert call(lib, T_dst=t, probs=A) == EUNSUPPORTED and "row-pool" in _err(lib)


def test_other_launches_are_as_before(lib):
    """Without the field nothing changes: a fused launch still refuses a block_path, path values past 3 are still no path."""
    assert call(lib, pool=1, ws=A) == EUNSUPPORTED and "row-pool" not in _err(lib) and "gather kernels" in _err(lib)
    assert call(lib, pool=1, ws=None, stride=0, path=4, bits=None) == EINVAL and "bad path 4" in _err(lib)
