"""The C ABI of the wide-head Performer backward (include/sea_hip_estimator_grad_wide.h, version 1).  No GPU: the predicate and the
workspace size are host arithmetic, and every call of the entry here ends in a refusal, which comes before any launch."""
import ctypes
import os
import re

import pytest

from sea_attention_amd import _build, _lib
from test_performer_bwd_abi import A, BF, EINVAL, EUNSUPPORTED, F16, F32, ODD, _ctype, _s

ENTRY = "sea_performer_causal_bwd_wide"
NAMES = ("sea_estimator_grad_wide_version", ENTRY + "_supported", ENTRY + "_workspace_bytes", ENTRY)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_entries_are_declared_bound_and_apart_from_the_older_tables(lib):
    text = open(os.path.join(os.path.dirname(__file__), "..", "include", "sea_hip_estimator_grad_wide.h")).read()
    assert re.search(r"#define\s+SEA_ESTIMATOR_GRAD_WIDE_ABI_VERSION\s+1\b", text)
    assert lib.sea_estimator_grad_wide_version() == 1 == _lib.ESTIMATOR_GRAD_WIDE_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = dict((m.group(2), (m.group(1), m.group(3))) for m in re.finditer(r"^(int|int64_t) (sea_\w+)\((.*?)\);", code, re.M | re.S))
    assert sorted(decls) == sorted(NAMES) == sorted(_lib._ESTIMATOR_GRAD_WIDE_SIGNATURES)
    older = (_lib._SIGNATURES, _lib._TRAIN_SIGNATURES, _lib._ESTIMATOR_GRAD_SIGNATURES, _lib._ESTIMATOR_GRAD_SEG_SIGNATURES,
             _lib._PREDICTOR_GRAD_SIGNATURES, _lib._PREDICTOR_CNN_GRAD_SIGNATURES, _lib._PREDICTOR_MLP_GRAD_SIGNATURES)
    for name in NAMES:
        ret, args = decls[name]
        argtypes, restype = _lib._ESTIMATOR_GRAD_WIDE_SIGNATURES[name]
        assert getattr(lib, name).argtypes == argtypes and restype is (ctypes.c_int64 if ret == "int64_t" else ctypes.c_int), name
        assert list(argtypes) == [_ctype(a.strip()) for a in args.replace("\n", " ").split(",") if a.strip() != "void"], name
        assert not any(name in table for table in older), name
    assert any(h.endswith("sea_hip_estimator_grad_wide.h") for h in _build.HEADERS) and "sea_performer_bwd_wide.hip" in _build.SOURCES
    assert _build.FILE_FLAGS["sea_performer_bwd_wide.hip"] == _build.FILE_FLAGS["sea_performer_bwd_seg.hip"]


@pytest.mark.parametrize("D,nb,want", [(64, 33, 0), (80, 1, 1), (80, 43, 1), (80, 80, 1), (128, 33, 1), (128, 77, 1), (128, 81, 0),
                                       (80, 81, 0), (72, 33, 0), (96, 33, 0), (128, 0, 0), (80, -2, 0)])
def test_the_predicate_is_host_arithmetic(lib, D, nb, want):
    for dt in (F32, F16, BF):
        assert lib.sea_performer_causal_bwd_wide_supported(D, nb, dt) == want
        assert lib.sea_performer_causal_bwd_supported(D, nb, dt) == (1 if D == 64 and 1 <= nb <= 80 else 0)      # the old entry's own
    assert all(lib.sea_performer_causal_bwd_wide_supported(D, nb, code) == 0 for code in (3, 7, -1))


def test_the_workspace_size_is_the_documented_formula(lib):
    size = lib.sea_performer_causal_bwd_wide_workspace_bytes
    up = lambda b: -(-b // 16) * 16
    for N, H, T, D, nb in ((1, 1, 1, 80, 43), (2, 3, 33, 128, 77), (1, 2, 97, 80, 80), (8, 40, 4096, 128, 77), (1, 3, 1, 128, 33)):
        P = N * H
        for dt in (F32, F16, BF):
            assert size(N, H, T, D, nb, dt) == up(2 * P * T * 2 * 4) + 2 * up(2 * P * T * D * 4) + up(P * T * D * 4)
    assert size(2, 3, 64, 64, 33, BF) == 0 and size(2, 3, 64, 72, 33, BF) == 0 and size(2, 3, 64, 128, 81, BF) == 0
    assert size(2, 3, 64, 128, 33, 7) == 0 and size(2, 3, 0, 128, 33, BF) == 0 and size(0, 3, 64, 80, 33, BF) == 0


def test_refusals_before_any_launch(lib):
    H, T = 2, 70

    def no(code, fragment, N=1, T=T, D=128, nb=77, dtype=BF, **kw):
        rows = _s(H * T * D, T * D, D)
        a = dict(q=A, k=A, v=A, pos=A, proj=A, q_strides=rows, k_strides=rows, v_strides=rows, pos_stride=D, grad_out=A, d_q=A,
                 d_k=A, d_v=A, d_pos=A, workspace=A, workspace_bytes=lib.sea_performer_causal_bwd_wide_workspace_bytes(N, H, T, D, nb, dtype))
        a.update(kw)
        rc = lib.sea_performer_causal_bwd_wide(a["q"], a["k"], a["v"], a["pos"], dtype, a["proj"], N, H, T, D, nb, a["q_strides"],
                                               a["k_strides"], a["v_strides"], a["pos_stride"], a["grad_out"], a["d_q"], a["d_k"],
                                               a["d_v"], a["d_pos"], a["workspace"], a["workspace_bytes"], None)
        err = lib.sea_last_error().decode()
        assert rc == code and fragment in err, (kw, rc, err)

    D = 128
    for arg in ("q", "k", "v", "pos", "proj", "q_strides", "k_strides", "v_strides", "grad_out", "d_q", "d_k", "d_v", "d_pos", "workspace"):
        no(EINVAL, f"{ENTRY}: {arg} is null", **{arg: None})
    for shape in ({"T": 0}, {"N": 0}, {"nb": 0}):
        no(EINVAL, f"{ENTRY}: bad shape", **shape)
    for t in ("q", "k", "v"):
        no(EINVAL, f"{ENTRY}: {t} rows must be 16-byte aligned", **{t: ODD})
        no(EINVAL, f"{ENTRY}: {t} rows must be 16-byte aligned", **{t + "_strides": _s(H * T * D, T * D, D + 4)})   # bf16: 8 bytes
        no(EINVAL, f"{ENTRY}: bad {t} strides", **{t + "_strides": _s(-8, T * D, D)})
        no(EINVAL, f"{ENTRY}: bad {t} strides", **{t + "_strides": _s(H * T * D, T * D, D - 8)})                    # rows overlap
    no(EINVAL, f"{ENTRY}: pos rows must be 16-byte aligned", pos=ODD)
    no(EINVAL, f"{ENTRY}: pos rows must be 16-byte aligned", pos_stride=D + 4)
    no(EINVAL, f"{ENTRY}: bad pos stride", pos_stride=-D)
    no(EINVAL, f"{ENTRY}: proj rows must be 16-byte aligned", proj=ODD)
    no(EINVAL, f"{ENTRY}: grad_out rows must be 16-byte aligned", grad_out=ODD)
    for t in ("d_q", "d_k", "d_v", "d_pos"):
        no(EINVAL, f"{ENTRY}: d_q, d_k, d_v, d_pos rows must be 16-byte aligned", **{t: ODD})
    # ---- what the kernels have no form for
    no(EUNSUPPORTED, f"{ENTRY}: D=64", D=64, nb=33)
    no(EUNSUPPORTED, f"{ENTRY}: D=72", D=72)
    no(EUNSUPPORTED, f"{ENTRY}: nb=81", nb=81)
    no(EUNSUPPORTED, f"{ENTRY}: nb=81", D=80, nb=81)
    for code in (3, 7, -1):
        no(EUNSUPPORTED, f"{ENTRY}: unknown dtype {code}", dtype=code)
    no(EUNSUPPORTED, f"{ENTRY}: T=", T=1 << 24)
    # ---- the workspace, one byte short and misaligned
    need = lib.sea_performer_causal_bwd_wide_workspace_bytes(1, H, T, D, 77, BF)
    no(EINVAL, f"{ENTRY}: workspace of {need} bytes needed", workspace_bytes=need - 1)
    no(EINVAL, f"{ENTRY}: workspace", workspace=ODD)
