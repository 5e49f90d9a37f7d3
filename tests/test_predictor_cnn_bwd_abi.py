"""The C ABI of the (convolution, ReLU) backward (include/sea_hip_predictor_cnn_grad.h, version 1).  No GPU: the predicate and the
workspace size are host arithmetic, and every call of the entry here passes never-dereferenced pointers and a null stream and ends
in a refusal, which comes before any launch."""
import ctypes
import os
import re

import pytest

from sea_attention_amd import _build, _lib

EINVAL, EUNSUPPORTED = -1, -2
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entry refuses first)
ODD = ctypes.c_void_p((1 << 20) + 8)
F32, F16, BF = _lib.SEA_F32, _lib.SEA_F16, _lib.SEA_BF16
ENTRY = "sea_causal_conv_relu_bwd"
NAMES = ("sea_predictor_cnn_grad_version", "sea_causal_conv_relu_bwd_supported", "sea_causal_conv_relu_bwd_workspace_bytes", ENTRY)
ROOT = os.path.join(os.path.dirname(__file__), "..")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _ctype(arg):
    return (ctypes.c_void_p if "*" in arg or arg.startswith("sea_stream_t")
            else ctypes.c_int64 if arg.startswith("int64_t") else ctypes.c_int)


def test_entries_are_declared_and_bound_argument_by_argument(lib):
    text = open(os.path.join(ROOT, "include", "sea_hip_predictor_cnn_grad.h")).read()
    assert re.search(r"#define\s+SEA_PREDICTOR_CNN_GRAD_ABI_VERSION\s+1\b", text)
    assert lib.sea_predictor_cnn_grad_version() == 1 == _lib.PREDICTOR_CNN_GRAD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = dict((m.group(2), (m.group(1), m.group(3))) for m in re.finditer(r"^(int|int64_t) (sea_\w+)\((.*?)\);", code, re.M | re.S))
    assert sorted(decls) == sorted(NAMES) == sorted(_lib._PREDICTOR_CNN_GRAD_SIGNATURES)
    older = (_lib.EXPORTED_SYMBOLS, _lib._TRAIN_SIGNATURES, _lib._ESTIMATOR_GRAD_SIGNATURES, _lib._PREDICTOR_GRAD_SIGNATURES)
    for name in NAMES:
        ret, args = decls[name]
        argtypes, restype = _lib._PREDICTOR_CNN_GRAD_SIGNATURES[name]
        assert getattr(lib, name).argtypes == argtypes and restype is (ctypes.c_int64 if ret == "int64_t" else ctypes.c_int), name
        assert list(argtypes) == [_ctype(a.strip()) for a in args.replace("\n", " ").split(",") if a.strip() != "void"], name
        assert not any(name in table for table in older)
    assert any(h.endswith("sea_hip_predictor_cnn_grad.h") for h in _build.HEADERS) and "sea_conv_bwd.hip" in _build.SOURCES


def test_the_predicate_is_host_arithmetic(lib):
    ok = lib.sea_causal_conv_relu_bwd_supported                                # (C, W, ksize, dilation, pad_w, dtype)
    for dt in (F16, BF):
        assert all(ok(C, W, 3, d, d, dt) == 1 for C in (8, 24, 40, 64, 80) for W in (8, 16, 24, 64) for d in (1, 2))
        assert not any(ok(C, 64, 3, 2, 2, dt) for C in (96, 128, 0, 12, 60))    # the forward's weight image; C % 8
        assert not any(ok(64, W, 3, 2, 2, dt) for W in (12, 72, 0))
        assert ok(64, 64, 3, 3, 3, dt) == 0 and ok(64, 64, 3, 2, 1, dt) == 0 and ok(64, 64, 3, 1, 2, dt) == 0
        assert ok(64, 64, 1, 1, 0, dt) == 0 and ok(64, 64, 1, 2, 2, dt) == 0
    assert not any(ok(64, 64, 3, 2, 2, code) for code in (F32, 3, 7, -1, 99))


def test_the_workspace_size_is_positive_a_multiple_of_16_and_monotone_in_rows(lib):
    size = lib.sea_causal_conv_relu_bwd_workspace_bytes                        # (N, T, W, C, dilation, dtype)
    for dt in (F16, BF):
        sizes = [size(N, T, 64, 64, 2, dt) for N, T in ((1, 1), (1, 8), (1, 9), (2, 9), (3, 700), (1, 4096), (8, 4096), (9, 4096))]
        assert sizes[0] > 0 and all(b % 16 == 0 for b in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        assert size(8, 4096, 64, 64, 2, dt) <= 128 << 20
    assert size(1, 8, 64, 96, 2, BF) == 0 and size(1, 8, 72, 64, 2, BF) == 0 and size(1, 8, 64, 64, 3, BF) == 0
    assert size(1, 8, 64, 64, 2, F32) == 0 and size(0, 8, 64, 64, 2, BF) == 0 and size(1, 0, 64, 64, 2, BF) == 0


def _call(lib, N=2, T=5, W=16, C=16, CinP=32, dilation=2, pad_w=2, dtype=BF, **kw):
    a = dict(x=A, y=A, g=A, w_packed=A, d_x=A, d_w=A, d_b=A, workspace=A)
    a["workspace_bytes"] = lib.sea_causal_conv_relu_bwd_workspace_bytes(N, T, W, C, dilation, dtype)
    a.update(kw)
    return lib.sea_causal_conv_relu_bwd(a["x"], a["y"], a["g"], dtype, N, T, W, C, a["w_packed"], CinP, dilation, pad_w, a["d_x"],
                                        a["d_w"], a["d_b"], a["workspace"], a["workspace_bytes"], None)


def test_refusals_before_any_launch(lib):
    def no(code, fragment, **kw):
        rc = _call(lib, **kw)
        err = lib.sea_last_error().decode()
        assert rc == code and fragment in err, (kw, rc, err)

    for arg in ("x", "y", "g", "w_packed", "d_w", "d_b", "workspace"):
        no(EINVAL, f"{ENTRY}: {arg} is null", **{arg: None})
    no(EINVAL, f"{ENTRY}: workspace", d_x=None, workspace_bytes=0)              # d_x is optional: as far as the workspace
    for dim in ("N", "T", "W", "C", "CinP", "dilation"):
        no(EINVAL, f"{ENTRY}: bad shape", **{dim: 0})
    no(EINVAL, f"{ENTRY}: bad shape", pad_w=-1)
    no(EINVAL, f"{ENTRY}: CinP=64", CinP=64)
    for code in (3, 7, -1):
        no(EUNSUPPORTED, f"{ENTRY}: unknown dtype {code}", dtype=code)
    no(EUNSUPPORTED, f"{ENTRY}: fp32 data", dtype=F32)
    no(EUNSUPPORTED, f"{ENTRY}: C=96", C=96, CinP=96)
    no(EUNSUPPORTED, f"{ENTRY}: C=12", C=12)
    no(EUNSUPPORTED, f"{ENTRY}: dilation=3", dilation=3, pad_w=3)
    no(EUNSUPPORTED, f"{ENTRY}: dilation=2, pad_w=1", pad_w=1)
    no(EUNSUPPORTED, f"{ENTRY}: W=12", W=12)
    no(EUNSUPPORTED, f"{ENTRY}: W=72", W=72)
    no(EUNSUPPORTED, f"{ENTRY}: N*T=", N=1 << 16, T=1 << 15)
    for t in ("x", "y", "g", "w_packed"):
        no(EINVAL, f"{ENTRY}: x, y, g, w_packed must be 16-byte aligned", **{t: ODD})
    for t in ("d_x", "d_w", "d_b"):
        no(EINVAL, f"{ENTRY}: d_x, d_w, d_b must be 16-byte aligned", **{t: ODD})
    need = lib.sea_causal_conv_relu_bwd_workspace_bytes(2, 5, 16, 16, 2, BF)
    assert need > 0
    no(EINVAL, f"{ENTRY}: workspace of {need} bytes needed", workspace_bytes=need - 1)
    no(EINVAL, f"{ENTRY}: workspace", workspace=ODD)
