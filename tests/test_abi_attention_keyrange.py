"""The key-range form of `sea_sparse_attention` at the C boundary (include/sea_hip.h, SEA_ATTN_KEYRANGE = 3): no new symbol --
`flags` carries the path and `range_keys` (bits 16..30), `probs_out` / `probs_stride_n` the fp32 workspace -- and every
argument the form does not take is refused with SEA_EINVAL / SEA_EUNSUPPORTED and a message that names the form, before
anything is launched.  No GPU: every call returns on the host (the fake device addresses are never dereferenced; the one call
that passes the form's checks is stopped by a later, general check of the entry: a misaligned `out`)."""
import ctypes

import pytest

from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import ops

EINVAL, EUNSUPPORTED = -1, -2
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entry refuses first)
B = ctypes.c_void_p((1 << 20) + 4096)
WS = ctypes.c_void_p(1 << 24)
ODD = ctypes.c_void_p((1 << 20) + 8)             # not 16-byte aligned
N, H, T_DST, T_SRC, RANGE = 2, 4, 64, 1200, 100
RANGES = 12


def _s(*v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.sea_last_error().decode()


def need(D=64, ranges=RANGES):
    return H * ranges * T_DST * (D + 2)


def call(lib, bits=A, ws=WS, stride=None, range_keys=RANGE, block_path=None, t_src_dev=None, table=None, page_rows=0,
         table_stride=0, write_cols=0, dtype=_lib.SEA_BF16, D=64, T_src=T_SRC, out=B, path=3):
    st = _s(H * 4096 * D, 4096 * D, D)
    stride = need(D, -(-T_src // range_keys) if range_keys else 1) if stride is None else stride
    return lib.sea_sparse_attention(
        A, A, A, dtype, N, H, T_DST, T_src, D, st, st, st, A, A, 4096, A, None, None, None, None, out, dtype, st, ws, stride,
        block_path, path | (range_keys << 16), bits, 32, 1, 4, write_cols, t_src_dev, 0, table, table_stride, page_rows, None)


def test_keyrange_path_is_declared(lib):
    assert _lib.SEA_ATTN_KEYRANGE == 3 and lib.sea_version() == 7 == _lib.ABI_VERSION
    assert "sea_sparse_attention" in _lib.EXPORTED_SYMBOLS


def test_keyrange_arguments_pass_the_forms_checks(lib):
    """A workspace, range_keys, bits and D = 64: the form's own checks pass (what stops this call is the entry's general
    alignment check, which runs after them and does not name the form)."""
    assert call(lib, out=ODD) == EUNSUPPORTED
    assert "16-byte aligned" in _err(lib) and "key-range" not in _err(lib)
    assert call(lib, out=ODD, stride=need() + 4) == EUNSUPPORTED and "key-range" not in _err(lib)     # a larger stride is fine
    assert call(lib, out=ODD, dtype=_lib.SEA_F32, D=32) == EUNSUPPORTED and "key-range" not in _err(lib)


def test_keyrange_refusals(lib):
    kr = "key-range form"
    assert call(lib, bits=None) == EUNSUPPORTED and kr in _err(lib) and "bits" in _err(lib)
    assert call(lib, ws=None) == EINVAL and kr in _err(lib) and "workspace" in _err(lib)
    assert call(lib, stride=need() - 1) == EINVAL and kr in _err(lib) and str(need()) in _err(lib)
    assert call(lib, range_keys=0) == EINVAL and kr in _err(lib) and "range_keys" in _err(lib)
    assert call(lib, block_path=A) == EINVAL and kr in _err(lib) and "block_path" in _err(lib)
    assert call(lib, t_src_dev=A) == EUNSUPPORTED and kr in _err(lib) and "t_src_dev" in _err(lib)
    assert call(lib, table=A, page_rows=64, table_stride=64) == EUNSUPPORTED and kr in _err(lib) and "block_table" in _err(lib)
    assert call(lib, write_cols=1) == EUNSUPPORTED and kr in _err(lib) and "write_cols" in _err(lib)
    assert call(lib, D=80) == EUNSUPPORTED and kr in _err(lib) and "D=80" in _err(lib)
    assert call(lib, T_src=65 * 64, range_keys=64) == EUNSUPPORTED and kr in _err(lib) and "64 ranges" in _err(lib)
    # batch items of the workspace are 16-byte aligned
    assert call(lib, stride=need() + 1) == EINVAL and kr in _err(lib) and "multiple of 4" in _err(lib) and str(need() + 1) in _err(lib)
    assert call(lib, ws=ODD) == EINVAL and kr in _err(lib) and "aligned" in _err(lib)


def test_other_paths_are_as_before(lib):
    """Path values past the key-range form are still no path; the fused gather form still ignores `flags`' range field."""
    assert call(lib, path=4, bits=None, ws=None, stride=0, range_keys=0) == EINVAL and "bad path 4" in _err(lib)
    assert call(lib, path=1, ws=None, stride=0, out=ODD) == EUNSUPPORTED and "key-range" not in _err(lib)


def test_workspace_helper():
    assert ops.keyrange_workspace_floats(2, 4, 64, 64, 12) == 2 * 4 * 12 * 64 * 66
    assert ops.keyrange_workspace_floats(N, H, T_DST, 64, RANGES) == N * need()
