"""The paged decode entries of the C ABI (include/sea_hip.h, *_paged): bound, and refusing bad arguments -- null table, a
page size that is not a power of two or not a multiple of the Performer chunk, too small a table stride, wrong dtype or D
-- with SEA_EINVAL / SEA_EUNSUPPORTED and a message before anything is launched.  No GPU: every call returns on the host
(the fake device addresses below are never dereferenced)."""
import ctypes

import pytest

from sea_attention_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
PAGED = ["sea_decode_stage_paged", "sea_performer_causal_step_paged", "sea_sparse_attention_paged"]
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entries refuse first)
B = ctypes.c_void_p((1 << 20) + 4096)


def _s(*v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.sea_last_error().decode()


def test_paged_entries_are_declared_and_bound(lib):
    for name in PAGED:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.sea_version() == 4                # additive: no version bump


def test_decode_stage_paged_refusals(lib):
    st = _s(8 * 64, 64)

    def call(table=A, page_rows=64, table_stride=16, dtype=_lib.SEA_BF16, D=64, stride=3, pool=32, cap=1000):
        return lib.sea_decode_stage_paged(A, A, A, dtype, 2, 8, D, st, st, st, B, B, cap, A, stride, table, table_stride,
                                          page_rows, pool, None)
    assert call(table=None) == EINVAL and "sea_decode_stage_paged: null pointer" in _err(lib)
    assert call(stride=0) == EINVAL and "counter_stride" in _err(lib)
    assert call(page_rows=96) == EINVAL and "power of two" in _err(lib)
    assert call(page_rows=32) == EINVAL and "multiple of the Performer chunk (64 rows)" in _err(lib)
    assert call(table_stride=15) == EINVAL and "table_stride 15" in _err(lib)
    assert call(pool=0) == EINVAL and "pool" in _err(lib)
    assert call(dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit" in _err(lib)
    assert call(D=96) == EUNSUPPORTED and "D=96" in _err(lib)


def test_performer_step_paged_refusals(lib):
    st = _s(8 * 64, 64, 64)

    def call(table=A, page_rows=64, table_stride=16, dtype=_lib.SEA_BF16, D=64, T=1, t_base_dev=A, stride=3, cap=1000):
        return lib.sea_performer_causal_step_paged(A, A, A, A, dtype, A, 2, 8, T, D, 33, st, st, st, D, B, None, A, A, 1 << 20,
                                                   t_base_dev, stride, table, table_stride, page_rows, cap, None)
    assert call(table=None) == EINVAL and "sea_performer_causal_step_paged: null pointer" in _err(lib)
    assert call(t_base_dev=None) == EINVAL and "null pointer" in _err(lib)
    assert call(stride=0) == EINVAL and "t_base_stride" in _err(lib)
    assert call(T=2) == EINVAL and "one new row" in _err(lib)
    assert call(page_rows=48) == EINVAL and "power of two" in _err(lib)
    assert call(page_rows=32) == EINVAL and "64 rows" in _err(lib)
    assert call(table_stride=10) == EINVAL and "table_stride" in _err(lib)
    assert call(dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit MFMA" in _err(lib)
    assert call(D=96) == EUNSUPPORTED and "sea_performer_causal_step_paged" in _err(lib)


def test_sparse_attention_paged_refusals(lib):
    st = _s(8 * 64, 64, 64)

    def call(table=A, page_rows=64, table_stride=64, dtype=_lib.SEA_BF16, D=64, T_dst=1, bits=A, cap=4096, ks=st):
        return lib.sea_sparse_attention_paged(
            A, A, A, dtype, 2, 8, T_dst, cap, D, st, ks, ks, A, A, 4096, A, None, None, None, None, B, dtype, st,
            bits, 256, 1, 16, 0, A, 3, table, table_stride, page_rows, None)
    assert call(table=None) == EINVAL and "sea_sparse_attention_paged: null pointer" in _err(lib)
    assert call(bits=None) == EINVAL and "null pointer" in _err(lib)
    assert call(page_rows=100) == EINVAL and "power of two" in _err(lib)
    assert call(page_rows=32) == EINVAL and "Performer chunk" in _err(lib)
    assert call(table_stride=63) == EINVAL and "table_stride 63" in _err(lib)
    assert call(dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit" in _err(lib)
    assert call(D=96) == EUNSUPPORTED and "D=96" in _err(lib)
    assert call(T_dst=2) == EUNSUPPORTED and "T_dst = 1" in _err(lib)
    assert call(cap=1 << 20, table_stride=1 << 14) == EUNSUPPORTED and "LDS" in _err(lib)
    # a page stride whose byte offset does not fit 32 bits
    assert call(ks=_s(1 << 31, 64, 64)) == EUNSUPPORTED and "do not fit" in _err(lib)
