"""The predictor-length contract of the decode entries (include/sea_hip.h): `sea_decode_cnn_tail_select` takes rows of W4 =
T_m / 4 pixels -- W4 = 64 (T_m = 256), and W4 = 16 / 24 / 32 (T_m = 64 / 96 / 128) with the constants table of
`sea_predictor_tail_consts`, which serves any T_m <= 256 -- and the Python predicates say the same.  No GPU: every call
returns on the host (the fake device addresses below are never dereferenced: each call is made to fail on a check)."""
import ctypes

import pytest
import torch

from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import ops

EINVAL, EUNSUPPORTED = -1, -2
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entries refuse first)
NM = "sea_decode_cnn_tail_select"


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.sea_last_error().decode()


def _cnn(lib, W4, tab=A, H=8, pad_w=2, scratch=None, rows=1, crow=A):
    C = 2 * H
    return lib.sea_decode_cnn_tail_select(
        A, A, A, A, scratch, _lib.SEA_BF16, 2, rows, C, H, W4, 12, 9, A, A, A, A, 32, 2, pad_w, A, A, 32, A, A, 1e-5, None, A, A, A,
        1, 16, A, A, A, crow, None, 0, 0, 0, tab, 3, None)


def test_decode_cnn_takes_shorter_rows_with_a_table(lib):
    # W4 = 32 / 24 / 16 with a table pass the W4 checks: the call fails on the NEXT check (a pad_w that is not the dilation)
    for W4 in (32, 24, 16):
        assert _cnn(lib, W4, pad_w=3) == EUNSUPPORTED and "width-preserving" in _err(lib), W4
        assert _cnn(lib, W4, pad_w=3, scratch=A, rows=4, crow=None) == EUNSUPPORTED and "width-preserving" in _err(lib), W4
    assert _cnn(lib, 64, pad_w=3) == EUNSUPPORTED and "width-preserving" in _err(lib)
    assert _cnn(lib, 64, tab=None, pad_w=3) == EUNSUPPORTED and "width-preserving" in _err(lib)       # T_m = 256: the table is optional


def test_decode_cnn_refuses_shorter_rows_without_a_table(lib):
    for W4 in (32, 16):
        assert _cnn(lib, W4, tab=None) == EUNSUPPORTED
        assert f"{NM}: without consts_tab: needs T_m = 256 (W4 = 64)" in _err(lib) and "sea_predictor_tail_consts" in _err(lib)
    misaligned = ctypes.c_void_p((1 << 20) + 4)
    assert _cnn(lib, 32, tab=misaligned) == EUNSUPPORTED and "16-byte aligned" in _err(lib)


def test_decode_cnn_refuses_rows_it_cannot_convolve(lib):
    assert _cnn(lib, 96) == EUNSUPPORTED and "W4 <= 64" in _err(lib) and "W4 = 96" in _err(lib)
    assert _cnn(lib, 128) == EUNSUPPORTED and "W4 <= 64" in _err(lib)
    assert _cnn(lib, 20) == EUNSUPPORTED and "W4 % 8 == 0" in _err(lib)
    assert _cnn(lib, 0) == EUNSUPPORTED and NM in _err(lib)
    # multiples of 8 outside the reference's grid: not instantiated
    for W4 in (8, 40, 48, 56):
        assert _cnn(lib, W4) == EUNSUPPORTED and "W4 = 16, 24, 32" in _err(lib), W4


def test_tail_consts_serves_every_length_up_to_256(lib):
    def call(T_m, tab=A, up=4):
        return lib.sea_predictor_tail_consts(_lib.SEA_BF16, T_m // up, up, T_m, A, A, tab, None)
    for T_m in (64, 96, 128, 256):                                   # accepted up to the null-pointer check
        assert call(T_m, tab=None) == EINVAL and "sea_predictor_tail_consts: null pointer" in _err(lib), T_m
    assert call(384, tab=None) == EUNSUPPORTED and "T_m = 256" in _err(lib)
    assert call(384) == EUNSUPPORTED and "sea_predictor_tail_consts" in _err(lib)
    assert call(512) == EUNSUPPORTED
    assert lib.sea_predictor_tail_consts(_lib.SEA_BF16, 32, 4, 96, A, A, None, None) == EUNSUPPORTED     # W4 * up != T_m


def test_predicates_follow_the_kernels():
    bf16, fp16 = torch.bfloat16, torch.float16
    assert ops.DECODE_PREDICTOR_LENGTHS == (64, 96, 128, 256)
    assert ops.decode_cnn_supported(24, 12, 96, bf16)
    assert not ops.decode_cnn_supported(24, 12, 384, bf16)
    for T_m in (64, 96, 128, 256):
        for H in (4, 8, 12, 20, 32, 40):
            assert ops.decode_cnn_supported(2 * H, H, T_m, bf16) and ops.decode_cnn_supported(2 * H, H, T_m, fp16), (H, T_m)
    for T_m in (32, 160, 192, 224, 384, 512):                       # the other multiples of 32: refused, not half-served
        assert not ops.decode_cnn_supported(16, 8, T_m, bf16), T_m
    assert not ops.decode_cnn_supported(16, 8, 128, torch.float32)
    assert not ops.decode_cnn_supported(12, 6, 128, bf16) and not ops.decode_cnn_supported(88, 44, 128, bf16)
    y16 = torch.empty((1, 2, 3, 4, 8), dtype=bf16)                   # a C8 activation (only dtype and rank are read)
    assert ops.decode_tail_select_supported(y16, 12, 128)
    assert ops.decode_tail_select_supported(y16, 12, 256) and ops.decode_tail_select_supported(y16, 40, 96)
    assert not ops.decode_tail_select_supported(y16.float(), 12, 128)               # 16-bit data
    assert not ops.decode_tail_select_supported(y16, 80, 128)                       # H <= 64
    # T_m = 256 keeps its rule (the register-resident kernel: H % 4 == 0), longer rows stay with the prefill form
    assert not ops.decode_tail_select_supported(y16, 10, 256) and ops.predictor_tail_select_supported(y16, 10, 256)
    assert not ops.decode_tail_select_supported(y16, 12, 384) and ops.predictor_tail_select_supported(y16, 12, 384)
    # `decode=True` of the older predicate keeps meaning the register-resident decode form
    assert not ops.predictor_tail_select_supported(y16, 12, 128, decode=True)
    assert ops.predictor_tail_select_supported(y16, 12, 256, decode=True)


def test_session_names_the_limit_for_longer_predictor_lengths():
    from sea_attention_amd.perlin_attention.decode import _predictor_length_error
    for T_M in (64, 96, 128, 256):
        assert _predictor_length_error(T_M) is None
    for T_M in (384, 512):
        why = _predictor_length_error(T_M)
        assert "W4 = T_M / 4 <= 64 in ConvRowC8" in why and "T_m <= 256 in the one-row decode attention" in why and f"T_M = {T_M}" in why
    assert "64 / 96 / 128 / 256" in _predictor_length_error(160)
