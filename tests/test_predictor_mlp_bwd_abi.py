"""The C ABI of the predictor MLP's backward (include/sea_hip_predictor_mlp_grad.h, version 1).  No GPU: the predicate and the
workspace size are host arithmetic, and every call of the entry here passes never-dereferenced pointers and a null stream and ends
in a refusal, which comes before any launch."""
import ctypes

import pytest

from sea_attention_amd import _build, _lib

EINVAL, EUNSUPPORTED = -1, -2
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entry refuses first)
ODD = ctypes.c_void_p((1 << 20) + 8)
F32, F16, BF = _lib.SEA_F32, _lib.SEA_F16, _lib.SEA_BF16
ENTRY = "sea_predictor_mlp_bwd"
POINTERS = ("x", "g_y", "g_tpred", "w1_packed", "w2_packed", "vectors", "d_x", "d_w1", "d_b1", "d_g1", "d_be1", "d_w2", "d_b2", "d_g2",
            "d_be2", "workspace")


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_version_and_binding(lib):
    assert lib.sea_predictor_mlp_grad_version() == 1 == _lib.PREDICTOR_MLP_GRAD_ABI_VERSION
    assert "#define SEA_PREDICTOR_MLP_GRAD_ABI_VERSION 1" in open(next(h for h in _build.HEADERS if h.endswith("_mlp_grad.h"))).read()
    assert "sea_mlp_bwd.hip" in _build.SOURCES and all(getattr(lib, n).argtypes == a for n, (a, _r) in _lib._PREDICTOR_MLP_GRAD_SIGNATURES.items())


#                      D1   D2   H   Din  dtype  accepted
@pytest.mark.parametrize("D1,D2,H,Din,dtype,ok", [
    (128, 128, 32, 192, BF, 1), (128, 16, 4, 64, F16, 1), (128, 48, 12, 192, F16, 1), (128, 64, 40, 256, BF, 1), (128, 128, 16, 32, BF, 1),
    (160, 128, 32, 240, BF, 0), (256, 128, 32, 384, BF, 0),          # d = 80 / 128
    (128, 144, 32, 192, BF, 0), (128, 256, 32, 192, BF, 0), (128, 8, 32, 192, BF, 0), (128, 40, 32, 192, BF, 0), (128, 0, 32, 192, BF, 0),
    (128, 128, 6, 192, BF, 0), (128, 128, 0, 192, BF, 0), (128, 128, 32, 200, BF, 0), (128, 128, 32, 288, BF, 0), (128, 128, 32, 0, BF, 0),
    (128, 128, 32, 192, F32, 0), (128, 128, 32, 192, 3, 0), (128, 128, 32, 192, -1, 0)])
def test_the_predicate_is_host_arithmetic(lib, D1, D2, H, Din, dtype, ok):
    assert lib.sea_predictor_mlp_bwd_supported(D1, D2, H, Din, dtype) == ok
    assert (lib.sea_predictor_mlp_bwd_workspace_bytes(2, H, 3, Din, D1, D2, dtype) > 0) == bool(ok)


def test_the_workspace_size_is_a_multiple_of_16_and_monotone_in_rows(lib):
    size = lambda N, T: lib.sea_predictor_mlp_bwd_workspace_bytes(N, 32, T, 192, 128, 128, BF)
    sizes = [size(N, T) for N, T in ((1, 1), (1, 8), (1, 9), (2, 9), (1, 2048), (1, 2049), (3, 700), (1, 4096), (8, 4096), (9, 4096))]
    assert sizes[0] > 0 and all(b % 16 == 0 for b in sizes) and all(a < b for a, b in zip(sizes, sizes[1:]))
    assert size(0, 8) == 0 and size(1, 0) == 0 and size(1 << 20, 1 << 10) == 0


def _call(lib, N=2, H=4, T=5, Din=64, D1=128, D2=32, dtype=BF, strides=(1280, 64, 256), **kw):
    a = dict.fromkeys(POINTERS, A)
    a["x_strides"] = (ctypes.c_int64 * 3)(*strides)
    a["workspace_bytes"] = lib.sea_predictor_mlp_bwd_workspace_bytes(N, H, T, Din, D1, D2, dtype)
    a.update(kw)
    return lib.sea_predictor_mlp_bwd(a["x"], a["x_strides"], a["g_y"], a["g_tpred"], dtype, N, H, T, Din, D1, D2, a["w1_packed"],
                                     a["w2_packed"], a["vectors"], 1e-5, 1e-5, *[a[n] for n in POINTERS[6:]], a["workspace_bytes"], None)


def test_refusals_before_any_launch(lib):
    def no(code, fragment, **kw):
        rc = _call(lib, **kw)
        err = lib.sea_last_error().decode()
        assert rc == code and fragment in err, (kw, rc, err)

    for arg in ("x", "x_strides", "g_y", "w1_packed", "w2_packed", "vectors", *POINTERS[7:]):
        no(EINVAL, f"{ENTRY}: {arg} is null", **{arg: None})
    no(EINVAL, f"{ENTRY}: workspace", g_tpred=None, d_x=None, workspace_bytes=0)   # both optional: as far as the workspace
    for dim in ("N", "H", "T", "Din", "D1", "D2"):
        no(EINVAL, f"{ENTRY}: bad shape", **{dim: 0})
    for code in (3, -1):
        no(EUNSUPPORTED, f"{ENTRY}: unknown dtype {code}", dtype=code)
    no(EUNSUPPORTED, f"{ENTRY}: fp32 data", dtype=F32)
    for kw in (dict(D1=160), dict(D1=256, Din=384), dict(D2=144), dict(D2=40), dict(H=6), dict(Din=48), dict(Din=288)):
        no(EUNSUPPORTED, f"{ENTRY}: (D1={kw.get('D1', 128)}, D2={kw.get('D2', 32)}, H={kw.get('H', 4)}, Din={kw.get('Din', 64)})", **kw)
    no(EUNSUPPORTED, f"{ENTRY}: N*H*T", N=1 << 16, T=1 << 15)
    for t in ("x", "g_y", "g_tpred", "w1_packed", "w2_packed", "vectors", "d_x"):
        no(EINVAL, f"{ENTRY}: x, g_y, g_tpred, w1_packed, w2_packed, vectors, d_x must be 16-byte aligned", **{t: ODD})
    no(EINVAL, f"{ENTRY}: x_strides", strides=(1280, 60, 256))
    no(EINVAL, f"{ENTRY}: the fp32 outputs", d_g2=ctypes.c_void_p((1 << 20) + 2))
    need = lib.sea_predictor_mlp_bwd_workspace_bytes(2, 4, 5, 64, 128, 32, BF)
    no(EINVAL, f"{ENTRY}: workspace of {need} bytes needed", workspace_bytes=need - 1)
    no(EINVAL, f"{ENTRY}: workspace", workspace=ODD)
