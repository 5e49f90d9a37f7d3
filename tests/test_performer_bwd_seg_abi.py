"""The C ABI of the row-segmented Performer backward (include/sea_hip_estimator_grad_seg.h, version 1).  No GPU: the segment count
and the workspace size are host arithmetic, and every call of the entry here ends in a refusal, which comes before any launch."""
import ctypes
import os
import re

import pytest

from sea_attention_amd import _build, _lib
from test_performer_bwd_abi import A, BF, EINVAL, EUNSUPPORTED, ODD, _ctype, _s

ENTRY = "sea_performer_causal_bwd_seg"
NAMES = ("sea_estimator_grad_seg_version", ENTRY + "_count", ENTRY + "_workspace_bytes", ENTRY)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def rule(T, requested):
    nc = -(-T // 64)
    cps = -(-nc // max(1, min(requested, nc)))
    return -(-nc // cps)


def test_entries_are_declared_bound_and_apart_from_the_older_tables(lib):
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "sea_hip_estimator_grad_seg.h")).read()
    assert re.search(r"#define\s+SEA_ESTIMATOR_GRAD_SEG_ABI_VERSION\s+1\b", text)
    assert lib.sea_estimator_grad_seg_version() == 1 == _lib.ESTIMATOR_GRAD_SEG_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = dict((m.group(2), (m.group(1), m.group(3))) for m in re.finditer(r"^(int|int64_t) (sea_\w+)\((.*?)\);", code, re.M | re.S))
    assert sorted(decls) == sorted(NAMES) == sorted(_lib._ESTIMATOR_GRAD_SEG_SIGNATURES)
    older = (_lib._SIGNATURES, _lib._TRAIN_SIGNATURES, _lib._ESTIMATOR_GRAD_SIGNATURES, _lib._PREDICTOR_GRAD_SIGNATURES,
             _lib._PREDICTOR_CNN_GRAD_SIGNATURES, _lib._PREDICTOR_MLP_GRAD_SIGNATURES)
    for name in NAMES:
        ret, args = decls[name]
        argtypes, restype = _lib._ESTIMATOR_GRAD_SEG_SIGNATURES[name]
        assert getattr(lib, name).argtypes == argtypes and restype is (ctypes.c_int64 if ret == "int64_t" else ctypes.c_int), name
        assert list(argtypes) == [_ctype(a.strip()) for a in args.replace("\n", " ").split(",") if a.strip() != "void"], name
        assert not any(name in table for table in older), name
    assert any(h.endswith("sea_hip_estimator_grad_seg.h") for h in _build.HEADERS) and "sea_performer_bwd_seg.hip" in _build.SOURCES


def test_segment_count_and_workspace_are_host_arithmetic(lib):
    count, size, base = lib.sea_performer_causal_bwd_seg_count, lib.sea_performer_causal_bwd_seg_workspace_bytes, \
        lib.sea_performer_causal_bwd_workspace_bytes
    for T, r in ((1, 1), (64, 3), (65, 2), (65, 8), (200, 4), (1100, 4), (1100, 7), (4096, 8), (4096, 22), (4096, 1 << 40)):
        assert count(T, r) == rule(T, r), (T, r)
    assert (count(1100, 4), count(1100, 7), count(65, 8), count(4096, 22)) == (4, 6, 2, 22)
    assert count(0, 2) == 0 and count(100, 0) == 0 and count(100, -1) == 0
    for nb, nbp in ((33, 48), (48, 48), (49, 80), (80, 80)):
        for T, r in ((65, 8), (1100, 7), (4096, 1)):
            assert size(2, 3, T, 64, nb, BF, r) == base(2, 3, T, 64, nb, BF) + 2 * 6 * rule(T, r) * (nbp * 128 + nbp) * 4
    assert size(2, 3, 64, 72, 33, BF, 2) == 0 and size(2, 3, 64, 64, 81, BF, 2) == 0 and size(2, 3, 64, 64, 33, BF, 0) == 0


def test_refusals_before_any_launch(lib):
    H, T, D = 2, 200, 64

    def no(code, fragment, N=1, T=T, D=D, nb=33, dtype=BF, segments=2, **kw):
        rows = _s(H * T * D, T * D, D)
        a = dict(q=A, k=A, v=A, pos=A, proj=A, q_strides=rows, k_strides=rows, v_strides=rows, pos_stride=D, grad_out=A, d_q=A,
                 d_k=A, d_v=A, d_pos=A, workspace=A,
                 workspace_bytes=lib.sea_performer_causal_bwd_seg_workspace_bytes(N, H, T, D, nb, dtype, segments))
        a.update(kw)
        rc = lib.sea_performer_causal_bwd_seg(a["q"], a["k"], a["v"], a["pos"], dtype, a["proj"], N, H, T, D, nb, a["q_strides"],
                                              a["k_strides"], a["v_strides"], a["pos_stride"], a["grad_out"], a["d_q"], a["d_k"],
                                              a["d_v"], a["d_pos"], segments, a["workspace"], a["workspace_bytes"], None)
        err = lib.sea_last_error().decode()
        assert rc == code and fragment in err, (kw, rc, err)

    for segments in (0, -3):
        no(EINVAL, f"{ENTRY}: segments={segments} must be at least 1", segments=segments)
    for arg in ("q", "k", "v", "pos", "proj", "q_strides", "grad_out", "d_q", "d_pos", "workspace"):
        no(EINVAL, f"{ENTRY}: {arg} is null", **{arg: None})
    no(EINVAL, f"{ENTRY}: bad shape", T=0)
    no(EINVAL, f"{ENTRY}: k rows must be 16-byte aligned", k=ODD)
    no(EINVAL, f"{ENTRY}: bad v strides", v_strides=_s(-8, T * D, D))
    no(EUNSUPPORTED, f"{ENTRY}: D=128", D=128)
    no(EUNSUPPORTED, f"{ENTRY}: nb=81", nb=81)
    no(EUNSUPPORTED, f"{ENTRY}: unknown dtype 7", dtype=7)
    need = lib.sea_performer_causal_bwd_seg_workspace_bytes(1, H, T, D, 33, BF, 4)
    no(EINVAL, f"{ENTRY}: workspace of {need} bytes needed", segments=4,                  # the size of two segments is too short
       workspace_bytes=lib.sea_performer_causal_bwd_seg_workspace_bytes(1, H, T, D, 33, BF, 2))
    no(EINVAL, f"{ENTRY}: workspace", workspace=ODD)
