"""The C ABI of the predictor tail's backward (include/sea_hip_predictor_grad.h, version 1).  No GPU: the predicate and the
workspace size are host arithmetic, and every call of the entry here passes never-dereferenced pointers and a null stream and ends
in a refusal, which comes before any launch.

The declarations against the ctypes binding argument by argument, the version, the three older headers untouched; the predicate;
the workspace size; then every refusal with its code (SEA_EINVAL: nulls, both gradients null, shapes, strides, alignment, a short
workspace; SEA_EUNSUPPORTED: what the kernel has no form for) and the fragment of `sea_last_error()` naming the entry and the
argument."""
import ctypes
import os
import re

import pytest

from sea_attention_amd import _build, _lib

EINVAL, EUNSUPPORTED = -1, -2
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entry refuses first)
ODD = ctypes.c_void_p((1 << 20) + 8)
F32, F16, BF = _lib.SEA_F32, _lib.SEA_F16, _lib.SEA_BF16
ENTRY = "sea_predictor_tail_bwd"
NAMES = ("sea_predictor_grad_version", "sea_predictor_tail_bwd_supported", "sea_predictor_tail_bwd_workspace_bytes", ENTRY)
ROOT = os.path.join(os.path.dirname(__file__), "..")


def _s(*v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _ctype(arg):
    return (_lib._i64p if arg.startswith("const int64_t*")
            else ctypes.c_void_p if "*" in arg or arg.startswith("sea_stream_t")
            else ctypes.c_int64 if arg.startswith("int64_t") else ctypes.c_float if arg.startswith("float") else ctypes.c_int)


def test_entries_are_declared_bound_and_apart_from_the_older_headers(lib):
    read = lambda name: open(os.path.join(ROOT, "include", name)).read()
    pred, grad, train, main = (read(n) for n in ("sea_hip_predictor_grad.h", "sea_hip_estimator_grad.h", "sea_hip_train.h", "sea_hip.h"))
    assert re.search(r"#define\s+SEA_PREDICTOR_GRAD_ABI_VERSION\s+1\b", pred)
    assert lib.sea_predictor_grad_version() == 1 == _lib.PREDICTOR_GRAD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", pred, flags=re.S)
    decls = dict((m.group(2), (m.group(1), m.group(3))) for m in re.finditer(r"^(int|int64_t) (sea_\w+)\((.*?)\);", code, re.M | re.S))
    assert sorted(decls) == sorted(NAMES) == sorted(_lib._PREDICTOR_GRAD_SIGNATURES)
    for name in NAMES:
        ret, args = decls[name]
        argtypes, restype = _lib._PREDICTOR_GRAD_SIGNATURES[name]
        assert hasattr(lib, name) and getattr(lib, name).argtypes == argtypes
        assert restype is (ctypes.c_int64 if ret == "int64_t" else ctypes.c_int), name
        want = [_ctype(a.strip()) for a in args.replace("\n", " ").split(",") if a.strip() != "void"]
        assert list(argtypes) == want, name                                    # argument by argument
        assert (name not in _lib.EXPORTED_SYMBOLS and name not in _lib._TRAIN_SIGNATURES and name not in _lib._ESTIMATOR_GRAD_SIGNATURES
                and name not in main and name not in train and name not in grad)
    # the three older headers and their versions are as they were
    assert (re.search(r"#define\s+SEA_ESTIMATOR_GRAD_ABI_VERSION\s+1\b", grad) and re.search(r"#define\s+SEA_TRAIN_ABI_VERSION\s+2\b", train)
            and re.search(r"#define\s+SEA_ABI_VERSION\s+7\b", main))
    assert lib.sea_estimator_grad_version() == 1 == _lib.ESTIMATOR_GRAD_ABI_VERSION
    assert lib.sea_train_version() == 2 == _lib.TRAIN_ABI_VERSION and lib.sea_version() == 7 == _lib.ABI_VERSION
    declared = sorted(set(re.findall(r"\b(sea_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S))))
    assert len(declared) == 37 and sorted(_lib.EXPORTED_SYMBOLS) == declared
    train_code = re.sub(r"/\*.*?\*/", "", train, flags=re.S)
    assert sorted(re.findall(r"^int (sea_\w+)\(", train_code, re.M)) == sorted(_lib._TRAIN_SIGNATURES) and len(_lib._TRAIN_SIGNATURES) == 5
    grad_code = re.sub(r"/\*.*?\*/", "", grad, flags=re.S)
    assert sorted(re.findall(r"^(?:int|int64_t) (sea_\w+)\(", grad_code, re.M)) == sorted(_lib._ESTIMATOR_GRAD_SIGNATURES)
    assert len(_lib._ESTIMATOR_GRAD_SIGNATURES) == 4
    assert any(h.endswith("sea_hip_predictor_grad.h") for h in _build.HEADERS) and "sea_tail_bwd.hip" in _build.SOURCES


def test_the_predicate_is_host_arithmetic(lib):
    ok = lib.sea_predictor_tail_bwd_supported                                  # (C, H, W4, up, T_m, dtype)
    for dt in (F32, F16, BF):
        for T_m in (32, 64, 96, 128, 256):
            assert all(ok(C, H, T_m // 4, 4, T_m, dt) == 1 for H in (1, 12, 32, 64) for C in (8, 24, 64, 80, 128))
        # what the LDS and lane plan does not fit is refused, not emulated
        assert ok(64, 32, 96, 4, 384, dt) == 0 and ok(64, 32, 128, 4, 512, dt) == 0
        assert ok(64, 32, 12, 4, 48, dt) == 0                                  # T_m % 32
        assert ok(64, 32, 32, 2, 64, dt) == 0 and ok(64, 32, 16, 4, 128, dt) == 0           # up != 4; W4 up != T_m
        assert ok(64, 65, 16, 4, 64, dt) == 0 and ok(64, 0, 16, 4, 64, dt) == 0
        assert ok(136, 32, 16, 4, 64, dt) == 0 and ok(60, 32, 16, 4, 64, dt) == 0 and ok(0, 32, 16, 4, 64, dt) == 0
    for code in (3, 5, 7, -1, 99):
        assert ok(64, 32, 16, 4, 64, code) == 0


def test_the_workspace_size_is_positive_a_multiple_of_16_and_monotone_in_rows(lib):
    size = lib.sea_predictor_tail_bwd_workspace_bytes                          # (N, C, H, T, W4, up, T_m, dtype)
    for dt in (F32, F16, BF):
        sizes = [size(N, 64, 32, T, 64, 4, 256, dt) for N, T in ((1, 1), (1, 7), (1, 8), (1, 9), (3, 700), (1, 4096), (2, 4096), (8, 4096), (9, 4096))]
        assert sizes[0] > 0 and all(b % 16 == 0 for b in sizes) and all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
        assert size(8, 64, 32, 4096, 64, 4, 256, dt) <= 64 << 20                # a few tens of MB at 32 768 rows
    assert size(1, 64, 32, 8, 96, 4, 384, BF) == 0 and size(1, 64, 65, 8, 16, 4, 64, BF) == 0 and size(1, 64, 32, 8, 16, 4, 64, 7) == 0
    assert size(1, 64, 32, 0, 16, 4, 64, BF) == 0 and size(0, 64, 32, 8, 16, 4, 64, BF) == 0


def _call(lib, N=2, C=16, H=8, T=5, W4=16, up=4, T_m=64, dtype=BF, eps=1e-5, **kw):
    a = dict(y=A, y_strides=_s(C * T * W4, T * W4, W4, 1), conv_w=A, gamma=A, beta=A, g_scores=A, g_probs=A, d_y=A, d_w=A, d_gamma=A,
             d_beta=A, workspace=A)
    a["workspace_bytes"] = lib.sea_predictor_tail_bwd_workspace_bytes(N, C, H, T, W4, up, T_m, dtype)
    a.update(kw)
    return lib.sea_predictor_tail_bwd(a["y"], dtype, N, C, H, T, W4, up, T_m, a["y_strides"], a["conv_w"], a["gamma"], a["beta"], eps,
                                      a["g_scores"], a["g_probs"], a["d_y"], a["d_w"], a["d_gamma"], a["d_beta"], a["workspace"],
                                      a["workspace_bytes"], None)


def test_refusals_before_any_launch(lib):
    C, T, W4 = 16, 5, 16

    def no(code, fragment, **kw):
        rc = _call(lib, **kw)
        err = lib.sea_last_error().decode()
        assert rc == code and fragment in err, (kw, rc, err)

    # ---- every named null that is not optional; either gradient alone may be null, not both
    for arg in ("y", "y_strides", "conv_w", "gamma", "beta", "d_y", "d_w", "d_gamma", "d_beta", "workspace"):
        no(EINVAL, f"{ENTRY}: {arg} is null", **{arg: None})
    no(EINVAL, f"{ENTRY}: g_scores and g_probs are both null", g_scores=None, g_probs=None)
    no(EINVAL, f"{ENTRY}: workspace", g_scores=None, workspace_bytes=0)          # one gradient null: as far as the workspace
    no(EINVAL, f"{ENTRY}: workspace", g_probs=None, workspace_bytes=0)
    # ---- shapes
    for dim in ("N", "C", "H", "T", "W4", "up", "T_m"):
        no(EINVAL, f"{ENTRY}: bad shape", **{dim: 0})
    no(EINVAL, f"{ENTRY}: bad shape", T=-3)
    # ---- strides of y: negative, overlapping, misaligned; its base
    no(EINVAL, f"{ENTRY}: bad y strides", y_strides=_s(-8, T * W4, W4, 1))
    no(EINVAL, f"{ENTRY}: bad y strides", y_strides=_s(C * T * W4, T * W4, W4 - 8, 1))                    # rows overlap
    no(EINVAL, f"{ENTRY}: bad y strides", y_strides=_s(C * T * W4, T * W4, 0, 1))                         # every row the same
    no(EINVAL, f"{ENTRY}: bad y strides", y_strides=_s(T * W4 * C, 1, W4 * C, C - 8))                      # channels-last, pixels overlap
    no(EINVAL, f"{ENTRY}: y rows must be 16-byte aligned", y=ODD)
    no(EINVAL, f"{ENTRY}: y rows must be 16-byte aligned", y_strides=_s(C * T * (W4 + 4), T * (W4 + 4), W4 + 4, 1))   # bf16: 8 bytes
    no(EINVAL, f"{ENTRY}: y rows must be 16-byte aligned", y_strides=_s(C * T * W4 + 4, T * W4, W4, 1))
    no(EINVAL, f"{ENTRY}: y rows must be 16-byte aligned", y_strides=_s(T * W4 * (C + 4), 1, W4 * (C + 4), C + 4))
    # fp32 rows of W4 + 4 elements ARE aligned, and so are channels-last rows: the same strides get as far as the workspace
    no(EINVAL, f"{ENTRY}: workspace", dtype=F32, y_strides=_s(C * T * (W4 + 4), T * (W4 + 4), W4 + 4, 1), workspace_bytes=0)
    no(EINVAL, f"{ENTRY}: workspace", y_strides=_s(T * W4 * C, 1, W4 * C, C), workspace_bytes=0)
    # ---- the other bases
    no(EINVAL, f"{ENTRY}: conv_w rows must be 16-byte aligned", conv_w=ODD)
    for t in ("gamma", "beta"):
        no(EINVAL, f"{ENTRY}: gamma, beta rows must be 16-byte aligned", **{t: ODD})
    for t in ("g_scores", "g_probs"):
        no(EINVAL, f"{ENTRY}: g_scores, g_probs rows must be 16-byte aligned", **{t: ODD})
    for t in ("d_y", "d_w", "d_gamma", "d_beta"):
        no(EINVAL, f"{ENTRY}: d_y, d_w, d_gamma, d_beta rows must be 16-byte aligned", **{t: ODD})
    # ---- what the kernel has no form for
    for code in (3, 7, -1):
        no(EUNSUPPORTED, f"{ENTRY}: unknown dtype {code}", dtype=code)
    no(EUNSUPPORTED, f"{ENTRY}: up=2", up=2, W4=32)
    no(EUNSUPPORTED, f"{ENTRY}: up=4, W4=16, T_m=128", T_m=128)
    no(EUNSUPPORTED, f"{ENTRY}: T_m=384", W4=96, T_m=384, y_strides=_s(C * T * 96, T * 96, 96, 1))
    no(EUNSUPPORTED, f"{ENTRY}: T_m=512", W4=128, T_m=512, y_strides=_s(C * T * 128, T * 128, 128, 1))
    no(EUNSUPPORTED, f"{ENTRY}: T_m=48", W4=12, T_m=48)
    no(EUNSUPPORTED, f"{ENTRY}: H=65", H=65)
    no(EUNSUPPORTED, f"{ENTRY}: C=136", C=136, y_strides=_s(136 * T * W4, T * W4, W4, 1))
    no(EUNSUPPORTED, f"{ENTRY}: C=12", C=12, y_strides=_s(12 * T * W4, T * W4, W4, 1))
    no(EUNSUPPORTED, f"{ENTRY}: N*T=", N=1 << 16, T=1 << 15)
    no(EUNSUPPORTED, f"{ENTRY}: y must have unit stride", y_strides=_s(C * T * W4 * 2, T * W4 * 2, W4 * 2, 2))
    # ---- the workspace, one byte short and misaligned
    need = lib.sea_predictor_tail_bwd_workspace_bytes(2, C, 8, T, W4, 4, 64, BF)
    assert need > 0
    no(EINVAL, f"{ENTRY}: workspace of {need} bytes needed", workspace_bytes=need - 1)
    no(EINVAL, f"{ENTRY}: workspace", workspace=ODD)
