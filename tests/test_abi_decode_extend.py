"""The two entries of the C ABI behind `DecodeSession.extend` (include/sea_hip.h): `sea_decode_gather_rows` and
`sea_decode_append_rows`.  Declared, bound, exported, and refusing bad arguments -- null pointers, a bad page size or table
stride, r0 > r1, a counter stride below 3, fp32 data, other head sizes, unaligned rows -- with SEA_EINVAL / SEA_EUNSUPPORTED and
a message naming the entry before anything is launched.  No GPU: every call returns on the host (the fake device addresses
below are never dereferenced)."""
import ctypes
import os
import re

import pytest

from sea_attention_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
ENTRIES = ["sea_decode_gather_rows", "sea_decode_append_rows"]
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entries refuse first)
B = ctypes.c_void_p((1 << 20) + 4096)
ODD = ctypes.c_void_p((1 << 20) + 8)             # not 16-byte aligned


def _s(*v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.sea_last_error().decode()


def test_extend_entries_are_declared_bound_and_exported(lib):
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "sea_hip.h")).read()
    for name in ENTRIES:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _lib._SIGNATURES[name][0]
    assert lib.sea_version() == 7 == _lib.ABI_VERSION
    assert re.search(r"#define\s+SEA_ABI_VERSION\s+7\b", header)


def test_decode_gather_rows_refusals(lib):
    nm = "sea_decode_gather_rows"

    def call(pool=A, table=A, out=B, dtype=_lib.SEA_BF16, N=4, H=8, D=64, cap=300, stride=5, page=64, pages=20, slot=1,
             r0=0, r1=200, out_rows=300):
        return lib.sea_decode_gather_rows(pool, dtype, N, H, D, cap, table, stride, page, pages, slot, r0, r1, out, out_rows, None)
    for name in ("pool", "table", "out"):
        assert call(**{name: None}) == EINVAL and f"{nm}: null pointer" in _err(lib), name
    assert call(page=48) == EINVAL and f"{nm}: page_rows 48" in _err(lib)            # not a power of two
    assert call(page=32) == EINVAL and "multiple of the Performer chunk" in _err(lib)   # below the chunk of d = 64
    assert call(page=0) == EINVAL and "page_rows 0" in _err(lib)
    assert call(stride=4) == EINVAL and f"{nm}: table_stride 4" in _err(lib)         # 300 rows of 64: 5 entries
    assert call(pages=0) == EINVAL and "bad pool" in _err(lib)
    assert call(r0=9, r1=8) == EINVAL and f"{nm}: rows [9, 8)" in _err(lib)          # r0 > r1
    assert call(r0=-1) == EINVAL and "rows [-1, 200)" in _err(lib)
    assert call(r1=301) == EINVAL and "capacity = 300" in _err(lib)
    assert call(out_rows=199) == EINVAL and "a buffer of 199 rows for 200" in _err(lib)
    assert call(slot=4) == EINVAL and "slot 4 outside 0 .. 3" in _err(lib)
    assert call(slot=-1) == EINVAL and "slot -1" in _err(lib)
    assert call(dtype=_lib.SEA_F32) == EUNSUPPORTED and f"{nm}: 16-bit" in _err(lib)
    assert call(D=96) == EUNSUPPORTED and "D in {64, 80, 128}" in _err(lib)
    assert call(out=ODD) == EUNSUPPORTED and f"{nm}: rows must be 16-byte aligned" in _err(lib)
    assert call(pool=ODD) == EUNSUPPORTED and "16-byte aligned" in _err(lib)
    assert call(dtype=_lib.SEA_F16, D=128, page=32, stride=10, pages=0) == EINVAL and "bad pool" in _err(lib)   # (d = 128: a 32-row page passes)


def test_decode_append_rows_refusals(lib):
    nm = "sea_decode_append_rows"
    H, D, nb = 8, 64, 64
    st = _s(300 * 64, 64)

    def call(k=A, v=A, ks=st, vs=st, pool=B, table=A, window=A, conv1=A, x_ring=A, y1_ring=A, image_src=A, image=A, counters=A,
             dtype=_lib.SEA_BF16, slot=1, N=4, D=D, seen=100, rows=40, cap=300, stride=5, page=64, pages=20, win=8, keep=4,
             row_bytes=2 * 64 * 8 * 2, x_rows=8, y_rows=9, cstride=3):
        return lib.sea_decode_append_rows(dtype, slot, N, H, D, nb, seen, rows, cap, k, v, ks, vs, pool, table, stride, page, pages,
                                          window, win, conv1, keep, row_bytes, x_ring, x_rows, y1_ring, y_rows, image_src, image,
                                          counters, cstride, 140, 141, 140, None)
    for name in ("window", "conv1", "x_ring", "y1_ring", "image_src", "image", "counters", "k", "v", "ks", "vs", "table"):
        assert call(**{name: None}) == EINVAL and f"{nm}: null pointer" in _err(lib), name
    # a contiguous session has no pool: then no table, page size, table stride or pool size either
    assert call(pool=None) == EINVAL and "without a kv_pool" in _err(lib)
    assert call(cstride=2) == EINVAL and f"{nm}: counter_stride 2" in _err(lib)
    assert call(cstride=-3) == EINVAL and "counter_stride" in _err(lib)
    assert call(page=48) == EINVAL and f"{nm}: page_rows 48" in _err(lib)
    assert call(page=32) == EINVAL and "multiple of the Performer chunk" in _err(lib)
    assert call(stride=4) == EINVAL and f"{nm}: table_stride 4" in _err(lib)
    assert call(pages=0) == EINVAL and "bad pool" in _err(lib)
    assert call(rows=0) == EINVAL and f"{nm}: rows [100, 100)" in _err(lib)          # nothing to append
    assert call(rows=-2) == EINVAL and "rows [100, 98)" in _err(lib)                 # r0 > r1
    assert call(rows=201) == EINVAL and "capacity = 300" in _err(lib)
    assert call(slot=4) == EINVAL and "slot 4 outside 0 .. 3" in _err(lib)
    assert call(win=9) == EINVAL and "does not fit rings of 8 and 9 rows" in _err(lib)
    assert call(keep=9, y_rows=9, win=8) == EINVAL and "does not fit rings" in _err(lib)
    assert call(keep=8, y_rows=8) == EINVAL and "does not fit rings" in _err(lib)    # a ring row would take two positions
    assert call(seen=2, rows=3) == EINVAL and "does not fit rings" in _err(lib)      # a window longer than the sequence
    assert call(dtype=_lib.SEA_F32) == EUNSUPPORTED and f"{nm}: 16-bit" in _err(lib)
    assert call(D=96) == EUNSUPPORTED and nm in _err(lib)
    assert call(row_bytes=2056) == EUNSUPPORTED and "whole 16-byte chunks" in _err(lib)
    assert call(k=ODD) == EUNSUPPORTED and f"{nm}: rows must be 16-byte aligned" in _err(lib)
    assert call(window=ODD) == EUNSUPPORTED and "16-byte aligned" in _err(lib)
    assert call(image=ODD) == EUNSUPPORTED and "16-byte aligned" in _err(lib)
    assert call(ks=_s(300 * 64, 60)) == EUNSUPPORTED and "16-byte aligned" in _err(lib)
    assert call(vs=_s(300 * 64 + 4, 64)) == EUNSUPPORTED and "16-byte aligned" in _err(lib)
