"""The C ABI of the sparse context branch's kernels (include/sea_hip_context_grad.h, version 1).  No GPU: the predicate and the
workspace size are host arithmetic, and every call of an entry here passes never-dereferenced pointers and a null stream and ends in
a refusal, which comes before any launch."""
import ctypes

import pytest

from sea_attention_amd import _build, _lib

EINVAL, EUNSUPPORTED = -1, -2
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entry refuses first)
ODD = ctypes.c_void_p((1 << 20) + 8)
F32, F16, BF = _lib.SEA_F32, _lib.SEA_F16, _lib.SEA_BF16
# entry -> (its pointer arguments in order, the optional ones, the 16-byte-aligned ones)
ENTRIES = {
    "sea_context_mix_fwd": (("v", "v_strides", "o", "row_scale", "mix", "ctx", "workspace"), ("row_scale",), ("v", "o", "ctx", "workspace")),
    "sea_context_mix_bwd": (("v", "v_strides", "o", "g", "row_scale", "mix", "d_o", "d_row_scale", "d_mix", "workspace"),
                            ("row_scale", "d_row_scale", "d_mix"), ("v", "o", "g", "d_o", "workspace")),
    "sea_context_dv_finish": (("g", "mix", "dv_attn", "dv", "workspace"), (), ("g", "dv_attn", "dv", "workspace")),
}


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def test_names_version_and_binding(lib):
    assert lib.sea_context_grad_version() == 1 == _lib.CONTEXT_GRAD_ABI_VERSION
    assert "#define SEA_CONTEXT_GRAD_ABI_VERSION 1" in open(next(h for h in _build.HEADERS if h.endswith("_context_grad.h"))).read()
    assert "sea_context_grad.hip" in _build.SOURCES and "sea_context_grad.hip" in _build.FILE_FLAGS
    assert set(ENTRIES) | {"sea_context_grad_version", "sea_context_grad_supported", "sea_context_grad_workspace_bytes"} \
        == set(_lib._CONTEXT_GRAD_SIGNATURES)
    assert all(getattr(lib, n).argtypes == a for n, (a, _r) in _lib._CONTEXT_GRAD_SIGNATURES.items())


@pytest.mark.parametrize("N,H,T,D", [(1, 2, 1, 64), (1, 2, 64, 64), (1, 2, 65, 64), (2, 3, 130, 80), (8, 32, 4096, 64), (1, 1, 193, 128)])
def test_the_workspace_size_follows_its_formula(lib, N, H, T, D):
    chunks = (T + 63) // 64
    assert lib.sea_context_grad_workspace_bytes(N, H, T, D, 0) == N * H * chunks * D * 4
    assert lib.sea_context_grad_workspace_bytes(N, H, T, D, 1) == 2 * N * H * chunks * D * 4
    assert not any(lib.sea_context_grad_workspace_bytes(*bad, 1) for bad in ((0, H, T, D), (N, H, 0, D), (N, H, T, 96), (N, H, 1 << 24, D)))


def _call(lib, entry, N=2, H=3, T=70, D=64, dtype=BF, out_dtype=F32, strides=(3 * 70 * 64, 70 * 64, 64), **kw):
    names = ENTRIES[entry][0]
    a = dict.fromkeys(names, A)
    a["v_strides"] = (ctypes.c_int64 * 3)(*strides)
    a["workspace_bytes"] = lib.sea_context_grad_workspace_bytes(N, H, T, D, entry != "sea_context_mix_fwd")
    a.update(kw)
    p = [a[n] for n in names]
    shape = (dtype, out_dtype, N, H, T, D)
    if entry == "sea_context_mix_fwd":
        return lib.sea_context_mix_fwd(*p[:5], *shape, p[5], p[6], a["workspace_bytes"], None)
    if entry == "sea_context_mix_bwd":
        return lib.sea_context_mix_bwd(*p[:6], *shape, *p[6:10], a["workspace_bytes"], None)
    return lib.sea_context_dv_finish(*p[:3], *shape, p[3], p[4], a["workspace_bytes"], None)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_refusals_before_any_launch(lib, entry):
    names, optional, aligned = ENTRIES[entry]

    def no(code, fragment, **kw):
        rc = _call(lib, entry, **kw)
        err = lib.sea_last_error().decode()
        assert rc == code and err.startswith(f"{entry}: ") and fragment in err, (kw, rc, err)

    for arg in names:
        if arg not in optional:
            no(EINVAL, f"{arg} is null", **{arg: None})
    for dim, bad in [(d, b) for d in "NHTD" for b in (0, -1)]:
        no(EINVAL, "bad shape", **{dim: bad})
    for code in (3, -1):
        no(EUNSUPPORTED, f"unknown dtype {code}", dtype=code)
        no(EUNSUPPORTED, f"unknown out_dtype {code}", out_dtype=code)
    for D in (32, 96, 256):
        no(EUNSUPPORTED, f"D={D} has no kernel", D=D)
    no(EUNSUPPORTED, "T=16777216 beyond the limit", T=1 << 24)
    for arg in aligned:
        no(EINVAL, "16-byte aligned", **{arg: ODD})
    no(EINVAL, "4-byte aligned", mix=ctypes.c_void_p((1 << 20) + 2))
    if "v" in names:
        no(EINVAL, "v_strides", strides=(3 * 70 * 64, 70 * 64, 68))           # bf16 rows: multiples of 8 elements
        no(EINVAL, "v_strides", dtype=F32, strides=(3 * 70 * 64, 70 * 64, 66))
    need = lib.sea_context_grad_workspace_bytes(2, 3, 70, 64, entry != "sea_context_mix_fwd")
    no(EINVAL, f"workspace of {need} bytes needed", workspace_bytes=need - 1)
