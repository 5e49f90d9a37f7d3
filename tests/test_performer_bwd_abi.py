"""The C ABI of the causal Performer's backward (include/sea_hip_estimator_grad.h, version 1).  No GPU: the predicate and the
workspace size are host arithmetic, and every call of the entry here passes never-dereferenced pointers and a null stream and ends
in a refusal, which comes before any launch.

The declarations against the ctypes binding argument by argument, the version, the two older headers untouched; the predicate;
the workspace size; then every refusal with its code (SEA_EINVAL: nulls, shapes, strides, alignment, a short workspace;
SEA_EUNSUPPORTED: what the kernels have no form for) and the fragment of `sea_last_error()` naming the entry and the argument."""
import ctypes
import os
import re

import pytest

from sea_attention_amd import _build, _lib

EINVAL, EUNSUPPORTED = -1, -2
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entry refuses first)
ODD = ctypes.c_void_p((1 << 20) + 8)
F32, F16, BF = _lib.SEA_F32, _lib.SEA_F16, _lib.SEA_BF16
ENTRY = "sea_performer_causal_bwd"
NAMES = ("sea_estimator_grad_version", "sea_performer_causal_bwd_supported", "sea_performer_causal_bwd_workspace_bytes", ENTRY)
ROOT = os.path.join(os.path.dirname(__file__), "..")


def _s(*v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _ctype(arg):
    return (_lib._i64p if arg.startswith("const int64_t*")
            else ctypes.c_void_p if "*" in arg or arg.startswith("sea_stream_t")
            else ctypes.c_int64 if arg.startswith("int64_t") else ctypes.c_int)


def test_entries_are_declared_bound_and_apart_from_the_older_headers(lib):
    grad = open(os.path.join(ROOT, "include", "sea_hip_estimator_grad.h")).read()
    train = open(os.path.join(ROOT, "include", "sea_hip_train.h")).read()
    main = open(os.path.join(ROOT, "include", "sea_hip.h")).read()
    assert re.search(r"#define\s+SEA_ESTIMATOR_GRAD_ABI_VERSION\s+1\b", grad)
    assert lib.sea_estimator_grad_version() == 1 == _lib.ESTIMATOR_GRAD_ABI_VERSION
    code = re.sub(r"/\*.*?\*/", "", grad, flags=re.S)
    decls = dict((m.group(2), (m.group(1), m.group(3))) for m in re.finditer(r"^(int|int64_t) (sea_\w+)\((.*?)\);", code, re.M | re.S))
    assert sorted(decls) == sorted(NAMES) == sorted(_lib._ESTIMATOR_GRAD_SIGNATURES)
    for name in NAMES:
        ret, args = decls[name]
        argtypes, restype = _lib._ESTIMATOR_GRAD_SIGNATURES[name]
        assert hasattr(lib, name) and getattr(lib, name).argtypes == argtypes
        assert restype is (ctypes.c_int64 if ret == "int64_t" else ctypes.c_int), name
        want = [_ctype(a.strip()) for a in args.replace("\n", " ").split(",") if a.strip() != "void"]
        assert list(argtypes) == want, name                                    # argument by argument
        assert name not in _lib.EXPORTED_SYMBOLS and name not in _lib._TRAIN_SIGNATURES and name not in main and name not in train
    # the two older headers and their versions are as they were
    assert re.search(r"#define\s+SEA_TRAIN_ABI_VERSION\s+2\b", train) and re.search(r"#define\s+SEA_ABI_VERSION\s+7\b", main)
    assert lib.sea_train_version() == 2 == _lib.TRAIN_ABI_VERSION and lib.sea_version() == 7 == _lib.ABI_VERSION
    declared = sorted(set(re.findall(r"\b(sea_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S))))
    assert len(declared) == 37 and sorted(_lib.EXPORTED_SYMBOLS) == declared
    train_code = re.sub(r"/\*.*?\*/", "", train, flags=re.S)
    assert sorted(re.findall(r"^int (sea_\w+)\(", train_code, re.M)) == sorted(_lib._TRAIN_SIGNATURES) and len(_lib._TRAIN_SIGNATURES) == 5
    assert any(h.endswith("sea_hip_estimator_grad.h") for h in _build.HEADERS) and "sea_performer_bwd.hip" in _build.SOURCES


def test_the_predicate_is_host_arithmetic(lib):
    ok = lib.sea_performer_causal_bwd_supported
    for dt in (F32, F16, BF):
        assert all(ok(64, nb, dt) == 1 for nb in range(1, 81))
        assert ok(72, 33, dt) == 0 and ok(64, 81, dt) == 0 and ok(64, 0, dt) == 0 and ok(64, -3, dt) == 0
    for code in (3, 5, 7, -1, 99):
        assert ok(64, 33, code) == 0


def test_the_workspace_size_is_positive_and_monotone_in_T(lib):
    size = lib.sea_performer_causal_bwd_workspace_bytes
    for dt in (F32, F16, BF):
        sizes = [size(2, 3, T, 64, 33, dt) for T in (1, 2, 63, 64, 65, 200, 4096, 16384)]
        assert sizes[0] > 0 and all(b % 16 == 0 for b in sizes) and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert size(2, 3, 64, 72, 33, BF) == 0 and size(2, 3, 64, 64, 81, BF) == 0 and size(2, 3, 64, 64, 33, 7) == 0
    assert size(2, 3, 0, 64, 33, BF) == 0


def _call(lib, N=1, H=2, T=64, D=64, nb=33, dtype=BF, **kw):
    rows = _s(H * T * D, T * D, D)
    a = dict(q=A, k=A, v=A, pos=A, proj=A, q_strides=rows, k_strides=rows, v_strides=rows, pos_stride=D, grad_out=A,
             d_q=A, d_k=A, d_v=A, d_pos=A, workspace=A)
    a["workspace_bytes"] = lib.sea_performer_causal_bwd_workspace_bytes(N, H, T, D, nb, dtype)
    a.update(kw)
    return lib.sea_performer_causal_bwd(a["q"], a["k"], a["v"], a["pos"], dtype, a["proj"], N, H, T, D, nb, a["q_strides"],
                                        a["k_strides"], a["v_strides"], a["pos_stride"], a["grad_out"], a["d_q"], a["d_k"], a["d_v"],
                                        a["d_pos"], a["workspace"], a["workspace_bytes"], None)


def test_refusals_before_any_launch(lib):
    H, T, D = 2, 64, 64

    def no(code, fragment, **kw):
        rc = _call(lib, **kw)
        err = lib.sea_last_error().decode()
        assert rc == code and fragment in err, (kw, rc, err)

    # ---- every named null
    for arg in ("q", "k", "v", "pos", "proj", "q_strides", "k_strides", "v_strides", "grad_out", "d_q", "d_k", "d_v", "d_pos", "workspace"):
        no(EINVAL, f"{ENTRY}: {arg} is null", **{arg: None})
    # ---- shapes
    no(EINVAL, f"{ENTRY}: bad shape", T=0)
    no(EINVAL, f"{ENTRY}: bad shape", N=0)
    no(EINVAL, f"{ENTRY}: bad shape", nb=0)
    # ---- bases and strides of every tensor the entry reads through strides
    for t in ("q", "k", "v"):
        no(EINVAL, f"{ENTRY}: {t} rows must be 16-byte aligned", **{t: ODD})
        no(EINVAL, f"{ENTRY}: {t} rows must be 16-byte aligned", **{t + "_strides": _s(H * T * D, T * D, D + 4)})   # bf16: 8 bytes
        no(EINVAL, f"{ENTRY}: {t} rows must be 16-byte aligned", **{t + "_strides": _s(H * T * D + 4, T * D, D)})
        no(EINVAL, f"{ENTRY}: bad {t} strides", **{t + "_strides": _s(-8, T * D, D)})
        no(EINVAL, f"{ENTRY}: bad {t} strides", **{t + "_strides": _s(H * T * D, T * D, D - 8)})                    # rows overlap
    no(EINVAL, f"{ENTRY}: pos rows must be 16-byte aligned", pos=ODD)
    no(EINVAL, f"{ENTRY}: pos rows must be 16-byte aligned", pos_stride=D + 4)
    no(EINVAL, f"{ENTRY}: bad pos stride", pos_stride=-D)
    no(EINVAL, f"{ENTRY}: proj rows must be 16-byte aligned", proj=ODD)
    no(EINVAL, f"{ENTRY}: grad_out rows must be 16-byte aligned", grad_out=ODD)
    for t in ("d_q", "d_k", "d_v", "d_pos"):
        no(EINVAL, f"{ENTRY}: d_q, d_k, d_v, d_pos rows must be 16-byte aligned", **{t: ODD})
    # fp32 rows of D + 4 elements ARE aligned: the same strides get as far as the workspace
    no(EINVAL, f"{ENTRY}: workspace", dtype=F32, q_strides=_s(H * T * (D + 4), T * (D + 4), D + 4), workspace_bytes=0)
    # ---- what the kernels have no form for
    r72 = _s(H * T * 72, T * 72, 72)
    no(EUNSUPPORTED, f"{ENTRY}: D=72", D=72, q_strides=r72, k_strides=r72, v_strides=r72, pos_stride=72)
    no(EUNSUPPORTED, f"{ENTRY}: nb=81", nb=81)
    for code in (3, 7, -1):
        no(EUNSUPPORTED, f"{ENTRY}: unknown dtype {code}", dtype=code)
    no(EUNSUPPORTED, f"{ENTRY}: T=", T=1 << 24)
    # ---- the workspace, one byte short and misaligned
    need = lib.sea_performer_causal_bwd_workspace_bytes(1, H, T, D, 33, BF)
    no(EINVAL, f"{ENTRY}: workspace of {need} bytes needed", workspace_bytes=need - 1)
    no(EINVAL, f"{ENTRY}: workspace", workspace=ODD)
