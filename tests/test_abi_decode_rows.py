"""The multi-row decode entries of the C ABI (include/sea_hip.h): `sea_decode_stage_rows` and
`sea_decode_cnn_tail_select_rows`, a step of 1 .. 8 new rows per sequence.  Declared, bound, and refusing bad arguments --
null pointers, rows 0 and 9, rings too small for the rows, a bad counter stride, fp32 data -- with SEA_EINVAL /
SEA_EUNSUPPORTED and a message before anything is launched.  No GPU: every call returns on the host (the fake device
addresses below are never dereferenced)."""
import ctypes

import pytest

from sea_attention_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
ROWS = ["sea_decode_stage_rows", "sea_decode_cnn_tail_select_rows"]
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entries refuse first)
B = ctypes.c_void_p((1 << 20) + 4096)


def _s(*v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.sea_last_error().decode()


def test_rows_entries_are_declared_and_bound(lib):
    for name in ROWS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.sea_version() == 5                # new entries, no existing prototype changed


def test_decode_stage_rows_refusals(lib):
    st = _s(8 * 4 * 64, 4 * 64, 64)

    def call(q=A, counters=A, stride=3, rows=4, dtype=_lib.SEA_BF16, D=64, strides=st):
        return lib.sea_decode_stage_rows(q, A, A, dtype, 2, 8, rows, D, strides, strides, strides, B, B, 128, counters, stride, None)
    assert call(q=None) == EINVAL and "sea_decode_stage_rows: null pointer" in _err(lib)
    assert call(counters=None) == EINVAL and "null pointer" in _err(lib)
    assert call(strides=None) == EINVAL and "null pointer" in _err(lib)
    assert call(rows=0) == EINVAL and "rows 0 outside 1 .. 8" in _err(lib)
    assert call(rows=9) == EINVAL and "rows 9 outside 1 .. 8" in _err(lib)
    assert call(stride=-1) == EINVAL and "counter stride" in _err(lib)
    assert call(dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit" in _err(lib)
    assert call(D=60) == EUNSUPPORTED and "multiple of 8" in _err(lib)
    assert call(strides=_s(8 * 4 * 64, 4 * 64, 60)) == EUNSUPPORTED and "16-byte aligned" in _err(lib)


def test_decode_cnn_tail_select_rows_refusals(lib):
    H, C = 8, 16

    def call(x_new=A, scratch=A, rows=4, ring_x=12, ring_y=8, stride=3, dtype=_lib.SEA_BF16, counters=A, bits=A):
        return lib.sea_decode_cnn_tail_select_rows(
            x_new, A, A, A, scratch, dtype, 2, rows, C, H, 64, ring_x, ring_y, A, A, A, A, 32, 2, 2, A, A, 32, A, A, 1e-5,
            None, A, counters, A, 1, 16, bits, A, A, None, stride, None)
    nm = "sea_decode_cnn_tail_select_rows"
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
