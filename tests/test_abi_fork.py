"""The fork / reorder entry of the C ABI (include/sea_hip.h: sea_decode_fork): declared, bound, and refusing bad arguments --
null pointers, no moves, a bad staging count, page size, table stride, counter stride or pool, wrong dtype or D, ring bytes
that are not whole 16-byte chunks, a staging buffer that is too small -- with SEA_EINVAL / SEA_EUNSUPPORTED and a message
before anything is launched.  No GPU: every call returns on the host (the fake device addresses are never dereferenced)."""
import ctypes

import pytest

from sea_attention_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entry refuses first)
B = ctypes.c_void_p((1 << 20) + 4096)
U = ctypes.c_void_p((1 << 20) + 8)               # not 16-byte aligned


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.sea_last_error().decode()


def test_fork_entry_is_declared_and_bound_at_abi_6(lib):
    assert "sea_decode_fork" in _lib.EXPORTED_SYMBOLS and hasattr(lib, "sea_decode_fork")
    assert lib.sea_version() == 7 == _lib.ABI_VERSION


def _staging_slot(lib, H=8, D=64, nb=64, dtype=_lib.SEA_BF16, x=4096, y1=1024, cap=1000, page_rows=64):
    entries = -(-cap // page_rows)
    return lib.sea_performer_state_bytes(1, H, D, nb, dtype) + x + y1 + 16 + 16 * -(-entries // 4)


def call(lib, moves=A, M=2, n_staged=0, dtype=_lib.SEA_BF16, N=4, H=8, D=64, nb=64, image=A, x_ring=A, x_bytes=4096,
         y1_ring=A, y1_bytes=1024, counters=A, counter_stride=3, table=A, table_stride=16, cap=1000, pool=B, page_rows=64,
         pool_pages=32, staging=None, staging_bytes=0):
    return lib.sea_decode_fork(moves, M, n_staged, dtype, N, H, D, nb, image, x_ring, x_bytes, y1_ring, y1_bytes, counters,
                               counter_stride, table, table_stride, cap, pool, page_rows, pool_pages, staging, staging_bytes,
                               None)


def test_fork_null_pointers(lib):
    for name in ("moves", "image", "x_ring", "y1_ring", "counters", "table", "pool"):
        assert call(lib, **{name: None}) == EINVAL and "sea_decode_fork: null pointer" in _err(lib), name


def test_fork_move_counts(lib):
    assert call(lib, M=0) == EINVAL and "0 moves" in _err(lib)
    assert call(lib, M=5, N=4) == EINVAL and "5 moves for 4 slots" in _err(lib)
    assert call(lib, n_staged=3, M=2) == EINVAL and "n_staged 3" in _err(lib)
    assert call(lib, n_staged=-1) == EINVAL and "n_staged -1" in _err(lib)


def test_fork_layout_refusals(lib):
    assert call(lib, counter_stride=2) == EINVAL and "counter_stride 2" in _err(lib)
    assert call(lib, page_rows=96) == EINVAL and "power of two" in _err(lib)
    assert call(lib, page_rows=32) == EINVAL and "multiple of the Performer chunk (64 rows)" in _err(lib)
    assert call(lib, table_stride=15) == EINVAL and "table_stride 15" in _err(lib)
    assert call(lib, pool_pages=0) == EINVAL and "pool of 0 pages" in _err(lib)


def test_fork_dtype_and_shape_refusals(lib):
    assert call(lib, dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit" in _err(lib)
    assert call(lib, D=96) == EUNSUPPORTED and "D=96" in _err(lib)
    assert call(lib, x_bytes=4100) == EUNSUPPORTED and "16-byte chunks" in _err(lib)
    assert call(lib, y1_bytes=0) == EUNSUPPORTED and "16-byte chunks" in _err(lib)
    assert call(lib, image=U) == EUNSUPPORTED and "aligned" in _err(lib)


def test_fork_staging_refusals(lib):
    need = _staging_slot(lib)
    assert call(lib, n_staged=1) == EINVAL and "staging buffer of 0 bytes" in _err(lib)
    assert call(lib, n_staged=2, staging=A, staging_bytes=2 * need - 16) == EINVAL and f"{2 * need} needed" in _err(lib)
    assert call(lib, n_staged=2, staging=U, staging_bytes=2 * need) == EUNSUPPORTED and "aligned" in _err(lib)
