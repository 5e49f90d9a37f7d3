"""The per-sequence (ragged) decode entries of the C ABI (include/sea_hip.h, *_ragged): bound, and refusing bad arguments
with SEA_EINVAL / SEA_EUNSUPPORTED and a message before anything is launched.  No GPU: every call returns on the host
(the fake device addresses below are never dereferenced)."""
import ctypes

import pytest

from sea_attention_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
RAGGED = ["sea_decode_stage_ragged", "sea_performer_causal_step_ragged", "sea_decode_cnn_tail_select_ragged",
          "sea_sparse_attention_ragged", "sea_csr_emit_ragged"]
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entries refuse first)
B = ctypes.c_void_p((1 << 20) + 4096)


def _s(*v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.sea_last_error().decode()


def test_ragged_entries_are_declared_and_bound(lib):
    for name in RAGGED:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    assert lib.sea_version() == 4                # additive: no version bump


def test_decode_stage_ragged_refusals(lib):
    st = _s(8 * 64, 64)
    args = lambda ctr, stride, dtype=_lib.SEA_BF16: (A, A, A, dtype, 2, 8, 64, st, st, st, B, B, 128, ctr, stride, None)
    assert lib.sea_decode_stage_ragged(*args(None, 3)) == EINVAL
    assert "sea_decode_stage_ragged: null pointer" in _err(lib)
    assert lib.sea_decode_stage_ragged(*args(A, 0)) == EINVAL
    assert "counter_stride" in _err(lib)
    assert lib.sea_decode_stage_ragged(*args(A, 3, _lib.SEA_F32)) == EUNSUPPORTED
    assert "16-bit" in _err(lib)


def test_performer_step_ragged_refusals(lib):
    st = _s(8 * 64, 64, 64)

    def call(t_base_dev, stride, dtype=_lib.SEA_BF16, state=A, D=64):
        return lib.sea_performer_causal_step_ragged(A, A, A, A, dtype, A, 2, 8, 1, D, 33, st, st, st, D, B, None, state, state,
                                                    1 << 20, t_base_dev, stride, None)
    assert call(None, 3) == EINVAL and "null pointer" in _err(lib)
    assert call(A, 0) == EINVAL and "t_base_stride" in _err(lib)
    assert call(A, 3, state=None) == EINVAL and "null pointer" in _err(lib)
    assert call(A, 3, dtype=_lib.SEA_F32) == EUNSUPPORTED and "16-bit MFMA" in _err(lib)
    assert call(A, 3, D=96) == EUNSUPPORTED and "sea_performer_causal_step_ragged" in _err(lib)


def test_decode_cnn_tail_select_ragged_refusals(lib):
    def call(counters, stride, W4=64, H=8):
        C = 2 * H
        return lib.sea_decode_cnn_tail_select_ragged(
            A, A, A, A, _lib.SEA_BF16, 2, C, H, W4, 8, 9, A, A, A, A, 32, 2, 2, A, A, 32, A, A, 1e-5, None, A, counters, A, 1, 16,
            A, A, A, A, None, 0, 0, 0, None, stride, None)
    assert call(None, 3) == EINVAL and "null pointer" in _err(lib)
    assert call(A, 2) == EINVAL and "counter_stride" in _err(lib)
    assert call(A, 3, W4=32) == EUNSUPPORTED and "T_m = 256" in _err(lib)
    assert call(A, 3, H=6) == EUNSUPPORTED and "sea_decode_cnn_tail_select_ragged" in _err(lib)


def test_sparse_attention_ragged_refusals(lib):
    st = _s(8 * 64, 64, 64)

    def call(bits, t_src_dev, stride, D=64):
        return lib.sea_sparse_attention_ragged(
            A, A, A, _lib.SEA_BF16, 2, 8, 1, 4096, D, st, st, st, A, A, 4096, A, None, None, None, None, B, _lib.SEA_BF16, st,
            bits, 256, 1, 16, 0, t_src_dev, stride, None)
    assert call(None, A, 3) == EINVAL and "sea_sparse_attention_ragged: null pointer" in _err(lib)
    assert call(A, None, 3) == EINVAL and "null pointer" in _err(lib)
    assert call(A, A, 0) == EINVAL and "t_src_stride" in _err(lib)
    assert call(A, A, 3, D=12) == EUNSUPPORTED and "D=12" in _err(lib)


def test_csr_emit_ragged_refusals(lib):
    def call(bits, t_src_dev, stride, T_cap=4096):
        return lib.sea_csr_emit_ragged(bits, A, A, 2, 8, 1, 256, T_cap, 1, 16, B, 4, 1024, 1024, t_src_dev, stride, None)
    assert call(A, None, 3) == EINVAL and "sea_csr_emit_ragged: null pointer" in _err(lib)
    assert call(None, A, 3) == EINVAL and "null pointer" in _err(lib)
    assert call(A, A, 0) == EINVAL and "t_src_stride" in _err(lib)
    assert call(A, A, 3, T_cap=1 << 29) == EUNSUPPORTED and "int32 ids" in _err(lib)
