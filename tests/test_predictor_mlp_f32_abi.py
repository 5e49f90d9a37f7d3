"""The C ABI of the one-launch fp32 predictor MLP (include/sea_hip_predictor_mlp_f32.h, version 1).  No GPU: the predicate is host
arithmetic, and every call of the entry passes never-dereferenced pointers and ends in a refusal, which comes before any launch."""
import ctypes
import re

import pytest

from sea_attention_amd import _build, _lib

EINVAL, EUNSUPPORTED = -1, -2
A, ODD = ctypes.c_void_p(1 << 20), ctypes.c_void_p((1 << 20) + 8)      # 16-byte aligned / not; never dereferenced
ENTRY = "sea_predictor_mlp_f32"
POINTERS = ("x", "w1_packed", "w2_packed", "vectors", "x_c8", "tpred", "row_scale", "avg_scale")
C_TYPES = {"int64_t": ctypes.c_int64, "float": ctypes.c_float, "const float*": ctypes.c_void_p, "float*": ctypes.c_void_p,
           "const int64_t*": ctypes.POINTER(ctypes.c_int64), "sea_stream_t": ctypes.c_void_p, "void": None}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_header_declarations_match_the_binding(lib):
    text = open(next(h for h in _build.HEADERS if h.endswith("_mlp_f32.h"))).read()
    assert "#define SEA_PREDICTOR_MLP_F32_ABI_VERSION 1" in text and "sea_mlp_f32.hip" in _build.SOURCES
    assert lib.sea_predictor_mlp_f32_version() == 1 == _lib.PREDICTOR_MLP_F32_ABI_VERSION
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decls = {name: [" ".join(a.split()[:-1]).replace(" *", "*") for a in args.split(",") if a.strip() != "void"]
             for name, args in re.findall(r"^int (sea_\w+)\(([^)]*)\);", text, flags=re.M)}
    assert sorted(decls) == sorted(_lib._PREDICTOR_MLP_F32_SIGNATURES)
    for name, (argtypes, restype) in _lib._PREDICTOR_MLP_F32_SIGNATURES.items():
        assert [C_TYPES[a] for a in decls[name]] == argtypes and restype is ctypes.c_int, name
        assert getattr(lib, name).argtypes == argtypes


@pytest.mark.parametrize("D1,D2,H,Din,ok",
                         [(128, D2, H, 192, 1) for D2 in (32, 48, 64, 128) for H in (4, 12, 32)]
                         + [(160, 128, 32, 192, 0), (256, 128, 32, 192, 0), (128, 256, 32, 192, 0), (128, 40, 32, 192, 0),
                            (128, 72, 32, 192, 0), (128, 128, 6, 192, 0), (128, 128, 32, 190, 0), (128, 0, 32, 192, 0), (128, 128, 0, 192, 0)])
def test_the_predicate_is_host_arithmetic(lib, D1, D2, H, Din, ok):
    assert lib.sea_predictor_mlp_f32_supported(D1, D2, H, Din) == ok


def _call(lib, N=2, H=4, T=5, Din=192, D1=128, D2=32, strides=(3840, 192, 768), stride_n=0, **kw):
    a = dict.fromkeys(POINTERS, A)
    a["x_strides"] = (ctypes.c_int64 * 3)(*strides)
    a.update(kw)
    return lib.sea_predictor_mlp_f32(a["x"], N, H, T, Din, a["x_strides"], D1, D2, a["w1_packed"], a["w2_packed"], a["vectors"], 1e-5, 1e-5,
                                     a["x_c8"], stride_n, a["tpred"], a["row_scale"], a["avg_scale"], None)


def test_refusals_before_any_launch(lib):
    def no(code, fragment, **kw):
        rc = _call(lib, **kw)
        err = lib.sea_last_error().decode()
        assert rc == code and fragment in err, (kw, rc, err)

    for arg in ("x", "x_strides", "w1_packed", "w2_packed", "vectors", "x_c8", "row_scale", "avg_scale"):
        no(EINVAL, f"{ENTRY}: {arg} is null", **{arg: None})
    no(EUNSUPPORTED, f"{ENTRY}: (D1=160", tpred=None, D1=160)                  # tpred is optional: as far as the predicate
    for dim in ("N", "H", "T", "Din", "D1", "D2"):
        no(EINVAL, f"{ENTRY}: bad shape", **{dim: 0})
    for kw in (dict(D1=160), dict(D1=256), dict(D2=256), dict(D2=40), dict(H=6), dict(Din=190)):
        no(EUNSUPPORTED, f"{ENTRY}: (D1={kw.get('D1', 128)}, D2={kw.get('D2', 32)}, H={kw.get('H', 4)}, Din={kw.get('Din', 192)})", **kw)
    no(EUNSUPPORTED, f"{ENTRY}: N*H*T", N=1 << 16, T=1 << 15)
    for t in ("x", "w1_packed", "w2_packed", "vectors", "x_c8", "tpred"):
        no(EINVAL, f"{ENTRY}: x, w1_packed, w2_packed, vectors, x_c8, tpred must be 16-byte aligned", **{t: ODD})
    no(EINVAL, f"{ENTRY}: row_scale, avg_scale", avg_scale=ctypes.c_void_p((1 << 20) + 2))
    no(EINVAL, f"{ENTRY}: x_strides", strides=(3840, 190, 768))
    no(EINVAL, f"{ENTRY}: x_c8_stride_n", stride_n=5 * 1 * 16 * 8 - 4)
