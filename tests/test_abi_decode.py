"""The decode-step entries of the C ABI (include/sea_hip.h): one entry per operator, whose arguments choose the
per-sequence form (a positive counter / position / length stride), the paged form (a block table) and the multi-row form (a
step of 1 .. 8 new rows per sequence: `rows`, and `y1_scratch` for the fused CNN launch).  Declared, bound, and
refusing bad arguments -- null pointers, half-specified forms (a table with stride 0, page arguments without a table, rows
without scratch, scratch with a crow), a page size that is not a power of two or not a multiple of the Performer chunk, too
small a table stride, rows 0 and 9, rings too small for the rows, wrong dtype or D -- with SEA_EINVAL / SEA_EUNSUPPORTED and
a message before anything is launched.  No GPU: every call returns on the host
(the fake device addresses below are never dereferenced)."""
import ctypes

import pytest

from sea_attention_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
DECODE = ["sea_decode_stage", "sea_performer_causal_step", "sea_decode_cnn_tail_select", "sea_sparse_attention", "sea_csr_emit"]
REMOVED = [n + "_ragged" for n in DECODE] + [n + "_paged" for n in ("sea_decode_stage", "sea_performer_causal_step",
                                                                      "sea_sparse_attention")]
REMOVED += ["sea_decode_stage_rows", "sea_decode_cnn_tail_select_rows", "sea_cumavg_sliced"]        # ABI 6
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entries refuse first)
B = ctypes.c_void_p((1 << 20) + 4096)


def _s(*v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.sea_last_error().decode()


def test_decode_entries_are_declared_and_bound(lib):
    for name in DECODE:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    for name in REMOVED:                         # ABI 5 and 6: the suffixed forms are arguments of their operator
        assert name not in _lib.EXPORTED_SYMBOLS and not hasattr(lib, name)
    assert lib.sea_version() == 7


def test_rows_entries_are_declared_and_bound(lib):
    """The multi-row forms are arguments of their operators (ABI 6): `rows` of sea_decode_stage, `y1_scratch` and `rows` of
    sea_decode_cnn_tail_select -- bound with those parameters, and no *_rows entry of either is left."""
    for name, nargs in (("sea_decode_stage", 21), ("sea_decode_cnn_tail_select", 43)):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert len(_lib._SIGNATURES[name][0]) == nargs and getattr(lib, name).argtypes == _lib._SIGNATURES[name][0]
        assert name + "_rows" not in _lib.EXPORTED_SYMBOLS and not hasattr(lib, name + "_rows")
    assert lib.sea_version() == 7 == _lib.ABI_VERSION


def test_decode_stage_refusals(lib):
    st = _s(8 * 64, 64, 64)

    def call(counters=A, stride=3, table=None, page_rows=0, table_stride=0, pool=0, dtype=_lib.SEA_BF16, D=64, cap=128, rows=1):
        return lib.sea_decode_stage(A, A, A, dtype, 2, 8, rows, D, st, st, st, B, B, cap, counters, stride, table, table_stride,
                                    page_rows, pool, None)
    # a counter per sequence
    assert call(counters=None) == EINVAL and "sea_decode_stage: null pointer" in _err(lib)
    assert call(stride=-1) == EINVAL and "counter_stride" in _err(lib)
    assert call(dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit" in _err(lib)
    # paged
    paged = lambda **kw: call(**{**dict(table=A, page_rows=64, table_stride=16, pool=32, cap=1000), **kw})
    assert paged(table=None) == EINVAL and "sea_decode_stage: null pointer" in _err(lib)
    assert paged(stride=0) == EINVAL and "counter_stride" in _err(lib)
    assert paged(page_rows=96) == EINVAL and "power of two" in _err(lib)
    assert paged(page_rows=32) == EINVAL and "multiple of the Performer chunk (64 rows)" in _err(lib)
    assert paged(table_stride=15) == EINVAL and "table_stride 15" in _err(lib)
    assert paged(pool=0) == EINVAL and "pool" in _err(lib)
    assert paged(dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit" in _err(lib)
    assert paged(D=96) == EUNSUPPORTED and "D=96" in _err(lib)
    # paged K / V takes one row per step
    assert paged(rows=2) == EUNSUPPORTED and "one row per step" in _err(lib)
    assert call(rows=0) == EINVAL and "rows 0 outside 1 .. 8" in _err(lib)
    assert call(rows=9) == EINVAL and "rows 9 outside 1 .. 8" in _err(lib)


def test_decode_stage_rows_refusals(lib):
    """`rows` in 2 .. 8: a step of several new rows per sequence."""
    st = _s(8 * 4 * 64, 4 * 64, 64)

    def call(q=A, counters=A, stride=3, rows=4, dtype=_lib.SEA_BF16, D=64, strides=st):
        return lib.sea_decode_stage(q, A, A, dtype, 2, 8, rows, D, strides, strides, strides, B, B, 128, counters, stride,
                                    None, 0, 0, 0, None)
    assert call(q=None) == EINVAL and "sea_decode_stage: null pointer" in _err(lib)
    assert call(counters=None) == EINVAL and "null pointer" in _err(lib)
    assert call(strides=None) == EINVAL and "null pointer" in _err(lib)
    assert call(rows=0) == EINVAL and "rows 0 outside 1 .. 8" in _err(lib)
    assert call(rows=9) == EINVAL and "rows 9 outside 1 .. 8" in _err(lib)
    assert call(stride=-1) == EINVAL and "counter stride" in _err(lib)
    assert call(dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit" in _err(lib)
    assert call(D=60) == EUNSUPPORTED and "multiple of 8" in _err(lib)
    assert call(strides=_s(8 * 4 * 64, 4 * 64, 60)) == EUNSUPPORTED and "16-byte aligned" in _err(lib)


def test_performer_step_refusals(lib):
    st = _s(8 * 64, 64, 64)

    def call(t_base_dev=A, stride=3, table=None, page_rows=0, table_stride=0, cap=0, dtype=_lib.SEA_BF16, D=64, T=1, state=A):
        return lib.sea_performer_causal_step(A, A, A, A, dtype, A, 2, 8, T, D, 33, st, st, st, D, B, None, state, state, 1 << 20,
                                             0, t_base_dev, stride, 1, None, 0, table, table_stride, page_rows, cap, None)
    # a position per sequence
    assert call(t_base_dev=None) == EINVAL and "null pointer" in _err(lib)
    assert call(stride=-1) == EINVAL and "t_base_stride" in _err(lib)
    assert call(state=None) == EINVAL and "null pointer" in _err(lib)
    assert call(dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit MFMA" in _err(lib)
    assert call(D=96) == EUNSUPPORTED and "sea_performer_causal_step" in _err(lib)
    # paged
    paged = lambda **kw: call(**{**dict(table=A, page_rows=64, table_stride=16, cap=1000), **kw})
    assert paged(table=None) == EINVAL and "sea_performer_causal_step: null pointer" in _err(lib)
    assert paged(t_base_dev=None) == EINVAL and "null pointer" in _err(lib)
    assert paged(stride=0) == EINVAL and "t_base_stride" in _err(lib)
    assert paged(T=2) == EINVAL and "one new row" in _err(lib)
    assert paged(page_rows=48) == EINVAL and "power of two" in _err(lib)
    assert paged(page_rows=32) == EINVAL and "64 rows" in _err(lib)
    assert paged(table_stride=10) == EINVAL and "table_stride" in _err(lib)
    assert paged(dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit MFMA" in _err(lib)
    assert paged(D=96) == EUNSUPPORTED and "sea_performer_causal_step" in _err(lib)


def test_decode_cnn_tail_select_refusals(lib):
    def call(counters, stride, W4=64, H=8):
        C = 2 * H
        return lib.sea_decode_cnn_tail_select(
            A, A, A, A, None, _lib.SEA_BF16, 2, 1, C, H, W4, 8, 9, A, A, A, A, 32, 2, 2, A, A, 32, A, A, 1e-5, None, A, counters, A,
            1, 16, A, A, A, A, None, 0, 0, 0, None, stride, None)
    # a counter triple per sequence
    assert call(None, 3) == EINVAL and "null pointer" in _err(lib)
    assert call(A, 2) == EINVAL and "counter_stride" in _err(lib)
    assert call(A, 1) == EINVAL and "counter_stride" in _err(lib)
    assert call(A, 3, W4=32) == EUNSUPPORTED and "T_m = 256" in _err(lib)
    assert call(A, 3, H=6) == EUNSUPPORTED and "sea_decode_cnn_tail_select" in _err(lib)


def test_decode_cnn_tail_select_rows_refusals(lib):
    """The multi-row form, y1_scratch != NULL: `rows` new rows per sequence, no crow and no in-launch emit."""
    H, C = 8, 16

    def call(x_new=A, scratch=A, rows=4, ring_x=12, ring_y=8, stride=3, dtype=_lib.SEA_BF16, counters=A, bits=A, crow=None,
             col=None):
        return lib.sea_decode_cnn_tail_select(
            x_new, A, A, A, scratch, dtype, 2, rows, C, H, 64, ring_x, ring_y, A, A, A, A, 32, 2, 2, A, A, 32, A, A, 1e-5,
            None, A, counters, A, 1, 16, bits, A, A, crow, col, 0, 0, 0, None, stride, None)
    nm = "sea_decode_cnn_tail_select"
    assert call(x_new=None) == EINVAL and f"{nm}: null pointer" in _err(lib)
    assert call(scratch=None) == EINVAL and "null pointer" in _err(lib)
    assert call(counters=None) == EINVAL and "null pointer" in _err(lib)
    assert call(bits=None) == EINVAL and "null pointer" in _err(lib)
    assert call(rows=0) == EINVAL and "rows 0 outside 1 .. 8" in _err(lib)
    assert call(rows=9) == EINVAL and "rows 9 outside 1 .. 8" in _err(lib)
    # dilation 2: a ring holds the 2 * 2 slots the step reads and the `rows` it writes
    assert call(ring_x=7) == EINVAL and "2 * dilation + rows = 8" in _err(lib)
    assert call(ring_y=7) == EINVAL and "2 * dilation + rows = 8" in _err(lib)
    assert call(rows=8, ring_x=12, ring_y=11) == EINVAL and "= 12" in _err(lib)
    assert call(stride=2) == EINVAL and "counter_stride must be >= 3" in _err(lib)
    assert call(stride=-3) == EINVAL and "counter_stride" in _err(lib)
    assert call(dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit" in _err(lib)
    # half-specified forms: several rows without the scratch, the scratch with the one-row form's crow / columns
    assert call(scratch=None, rows=2, crow=A) == EINVAL and "needs y1_scratch" in _err(lib)
    assert call(crow=A) == EINVAL and "crow_out / col must be NULL" in _err(lib)
    assert call(col=A) == EINVAL and "crow_out / col must be NULL" in _err(lib)


def test_sparse_attention_decode_refusals(lib):
    st = _s(8 * 64, 64, 64)

    def call(bits=A, t_src_dev=A, stride=3, table=None, page_rows=0, table_stride=0, dtype=_lib.SEA_BF16, D=64, T_dst=1,
             cap=4096, ks=st):
        return lib.sea_sparse_attention(
            A, A, A, dtype, 2, 8, T_dst, cap, D, st, ks, ks, A, A, 4096, A, None, None, None, None, B, dtype, st, None, 0, None, 0,
            bits, 256, 1, 16, 0, t_src_dev, stride, table, table_stride, page_rows, None)
    # a length per sequence
    assert call(bits=None) == EINVAL and "sea_sparse_attention: null pointer" in _err(lib)
    assert call(t_src_dev=None) == EINVAL and "null pointer" in _err(lib)
    assert call(stride=-1) == EINVAL and "t_src_stride" in _err(lib)
    assert call(D=12) == EUNSUPPORTED and "D=12" in _err(lib)
    # paged
    paged = lambda **kw: call(**{**dict(table=A, page_rows=64, table_stride=64), **kw})
    assert paged(table=None) == EINVAL and "sea_sparse_attention: null pointer" in _err(lib)
    assert paged(bits=None) == EINVAL and "null pointer" in _err(lib)
    assert paged(stride=0) == EINVAL and "t_src_stride" in _err(lib)
    assert paged(page_rows=100) == EINVAL and "power of two" in _err(lib)
    assert paged(page_rows=32) == EINVAL and "Performer chunk" in _err(lib)
    assert paged(table_stride=63) == EINVAL and "table_stride 63" in _err(lib)
    assert paged(dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit" in _err(lib)
    assert paged(D=96) == EUNSUPPORTED and "D=96" in _err(lib)
    assert paged(T_dst=2) == EUNSUPPORTED and "T_dst = 1" in _err(lib)
    assert paged(cap=1 << 20, table_stride=1 << 14) == EUNSUPPORTED and "LDS" in _err(lib)
    # a page stride whose byte offset does not fit 32 bits
    assert paged(ks=_s(1 << 31, 64, 64)) == EUNSUPPORTED and "do not fit" in _err(lib)


def test_csr_emit_decode_refusals(lib):
    def call(bits, t_src_dev, stride, T_cap=4096, values_out=None):
        return lib.sea_csr_emit(bits, A, A, 2, 8, 1, 256, T_cap, 1, 16, B, 4, 1024, 1024, values_out, t_src_dev, stride, None)
    # a length per sequence
    assert call(A, None, 3) == EINVAL and "sea_csr_emit: null pointer" in _err(lib)
    assert call(None, A, 3) == EINVAL and "null pointer" in _err(lib)
    assert call(A, A, -1) == EINVAL and "t_src_stride" in _err(lib)
    assert call(A, A, 3, values_out=A) == EUNSUPPORTED and "writes no values" in _err(lib)
    assert call(A, A, 3, T_cap=1 << 29) == EUNSUPPORTED and "int32 ids" in _err(lib)
