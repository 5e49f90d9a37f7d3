"""No GPU: the surface of the decode sessions' attention probabilities -- the keyword on every constructor, `probs_out` on the
operator, a values handle that keeps pending columns pending -- and the C ABI's size, which the feature does not change."""
import ctypes
import inspect
import os
import re

import torch

from sea_attention_amd import _lib, opt_plumbing as P
from sea_attention_amd.perlin_attention import PerlinAttention, get_default_config, ops, register_default_config
from sea_attention_amd.perlin_attention.decode import DecodeSession

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constructors_take_attention_probs_off_by_default():
    for fn in (DecodeSession.__init__, DecodeSession.from_sequences, PerlinAttention.decode_session):
        p = inspect.signature(fn).parameters["attention_probs"]
        assert p.default is False, fn
    assert DecodeSession.attention_probs is None and DecodeSession._probs_buf is None
    params = list(inspect.signature(ops.sparse_attention).parameters.values())
    assert params[-1].name == "probs_out" and params[-1].default is None         # a trailing keyword


def test_opt_block_has_the_opt_in_flag():
    old = get_default_config()
    try:
        blk = P.SeaOPTAttention(4 * 64, 4)
        assert blk.decode_graph_attentions is False and blk.decode_graph_capacity is None
    finally:
        register_default_config(old)


def test_values_handle_keeps_pending_columns_pending():
    """`with_values` on a handle whose columns no launch has written: nothing is emitted, the new handle is pending too, and the
    first reader of either handle's `.col` runs the one emit."""
    crow = torch.tensor([[0, 3]], dtype=torch.int32)
    col = torch.zeros((1, 4), dtype=torch.int32)
    head_off = torch.tensor([[[0, 1, 3]]], dtype=torch.int32)
    csr = ops.FlatCSR(crow, col, head_off, 2, 10)
    calls = []
    csr._pending = (32, 4, True, lambda: (calls.append(1), col.copy_(torch.tensor([[1, 12, 11, 0]], dtype=torch.int32))))
    vals = torch.tensor([[0.5, 0.25, 0.25, -7.0]])
    pv = csr.with_values(vals)
    assert calls == [] and pv.col_is_pending and csr.col_is_pending and pv.vals is vals and pv.crow is crow
    assert pv.col.tolist() == [[1, 12, 11, 0]] and calls == [1]
    assert not pv.col_is_pending and not csr.col_is_pending
    assert pv.values().tolist() == [[0.5, 0.25, 0.25]] and pv.col_indices().tolist() == [[1, 12, 11]] and calls == [1]
    done = csr.with_values(vals)                                              # a handle whose columns are there: as before
    assert not done.col_is_pending and done.col is col and calls == [1]


def test_decode_entry_checks_the_probs_stride_before_any_launch():
    """`sea_sparse_attention`, decode forms with probs_out: a row of the values must be at least a row of `col` wide (SEA_EINVAL;
    fake aligned addresses, never dereferenced: the entry refuses first) -- per sequence, shared length, paged."""
    lib = _lib.load()
    A, B, C = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 4096), ctypes.c_void_p(1 << 21)
    st = (ctypes.c_int64 * 3)(8 * 64, 64, 64)

    def call(probs_stride, stride=3, T_dst=1, table=None, page_rows=0, table_stride=0):
        return lib.sea_sparse_attention(
            A, A, A, _lib.SEA_BF16, 2, 8, T_dst, 4096, 64, st, st, st, A, A, 4096, A, None, None, None, None, B, _lib.SEA_BF16, st,
            C, probs_stride, None, 0, A, 256, 1, 16, 0, A, stride, table, table_stride, page_rows, None)
    for kw in (dict(), dict(stride=0), dict(T_dst=3), dict(table=A, page_rows=64, table_stride=64)):
        assert call(4095, **kw) == -1, kw
        err = lib.sea_last_error().decode()
        assert "probs_stride_n >= col_stride_n" in err and "4095 < 4096" in err, (kw, err)


def test_header_still_declares_38_entries():
    src = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    assert "no probs_out" not in src
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert len(set(re.findall(r"\b(sea_[a-z0-9_]+)\s*\(", src))) == 37
