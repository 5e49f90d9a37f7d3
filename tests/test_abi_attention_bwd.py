"""The C ABI of the sparse attention's backward (include/sea_hip.h, version 7): one entry, `sea_sparse_attention_bwd`, whose
`form` argument picks the gather or the atomic form, and the workspace query that follows the same rule.  No GPU: every call of
the entry passes aligned, never-dereferenced pointers and a null stream and ends in a refusal, which comes before any launch or
memset; the query touches no memory at all.

The declarations against the ctypes binding argument by argument, the removed `_gather` symbol, the version and symbol counts;
every refusal with its code (SEA_EINVAL: null pointers, a bad dtype, shape or form, a workspace that is missing or too small;
SEA_EUNSUPPORTED: D, strides, alignment, a pinned form without kernels) and the fragment of `sea_last_error()` that names the
entry and the argument; the workspace sizes against the documented layout."""
import ctypes
import os
import re

import pytest

from sea_attention_amd import _lib

EINVAL, EUNSUPPORTED = -1, -2
ENTRY, QUERY, GONE = "sea_sparse_attention_bwd", "sea_sparse_attention_bwd_workspace_bytes", "sea_sparse_attention_bwd_gather"
F32, F16, BF = _lib.SEA_F32, _lib.SEA_F16, _lib.SEA_BF16
AUTO, GATHER, ATOMIC = _lib.SEA_ATTN_BWD_AUTO, _lib.SEA_ATTN_BWD_GATHER, _lib.SEA_ATTN_BWD_ATOMIC
BASE = 1 << 20                                   # 16-byte aligned, never dereferenced (the entry refuses first)
ODD = ctypes.c_void_p(BASE + 8)
POINTERS = ("q", "k", "v", "crow", "col", "head_off", "probs", "out", "dout", "dq", "dk", "dv")
ALIGNED = ("q", "k", "v", "dout", "dq", "dk", "dv")


def _s(*v):
    return (ctypes.c_int64 * len(v))(*v)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.sea_last_error().decode()


def ws_bytes(N, H, T_src, col_stride_n):
    """The documented layout: list starts and cursors, (N, H * T_src + 1) int32 each in whole 16 bytes, then 16 bytes per CSR
    slot, or the scan's 32 chunk totals per item where those are more."""
    ceil4 = lambda x: (x + 3) // 4 * 4
    return 2 * 4 * ceil4(N * (H * T_src + 1)) + max(16 * N * col_stride_n, 128 * N)


def _call(lib, dtype=BF, N=1, H=2, T_dst=64, T_src=64, D=64, stride=4096, form=AUTO, ws="enough", ws_bytes_=None, **kw):
    """The entry with good arguments (never-dereferenced pointers) except for what the keywords replace; ws: "enough" = an
    aligned pointer and the bytes the layout needs, else the pointer to pass"""
    rows = lambda T: _s(H * T * D, T * D, D)
    a = {name: ctypes.c_void_p(BASE + 4096 * i) for i, name in enumerate(POINTERS)}
    a.update(qs=rows(T_dst), ks=rows(T_src), vs=rows(T_src))
    a.update(kw)
    need = ws_bytes(N, H, T_src, stride)
    wptr = ctypes.c_void_p(BASE + 4096 * 64) if ws == "enough" else ws
    nbytes = need if ws_bytes_ is None else ws_bytes_
    return lib.sea_sparse_attention_bwd(a["q"], a["k"], a["v"], dtype, N, H, T_dst, T_src, D, a["qs"], a["ks"], a["vs"], a["crow"],
                                        a["col"], stride, a["head_off"], a["probs"], stride, a["out"], a["dout"], a["dq"], a["dk"],
                                        a["dv"], wptr, nbytes, form, None)


def test_one_entry_is_declared_and_bound(lib):
    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "sea_hip.h")).read()
    assert re.search(r"#define\s+SEA_ABI_VERSION\s+7\b", header) and lib.sea_version() == 7 == _lib.ABI_VERSION
    assert re.search(r"^ \*   7  .*sea_sparse_attention_bwd_gather is gone", header, re.M), "the version history's entry"
    assert re.search(r"enum sea_attn_bwd_form \{ SEA_ATTN_BWD_AUTO = 0, SEA_ATTN_BWD_GATHER = 1, SEA_ATTN_BWD_ATOMIC = 2 \};", header)
    assert (AUTO, GATHER, ATOMIC) == (0, 1, 2)
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = sorted(set(re.findall(r"\b(sea_[a-z0-9_]+)\s*\(", code)))
    assert len(declared) == 37 and sorted(_lib.EXPORTED_SYMBOLS) == declared
    assert GONE not in code and GONE not in _lib._SIGNATURES and not hasattr(lib, GONE)
    assert [n for n in declared if n.startswith(ENTRY)] == [ENTRY, QUERY]
    for name, ret, restype in ((ENTRY, "int", ctypes.c_int), (QUERY, "int64_t", ctypes.c_int64)):
        decl = re.search(r"^%s %s\((.*?)\);" % (ret, name), code, re.M | re.S)
        assert decl, name
        argtypes, bound = _lib._SIGNATURES[name]
        assert getattr(lib, name).argtypes == argtypes and bound is restype
        want = []                                                              # the binding matches the declaration, argument by argument
        for arg in decl.group(1).replace("\n", " ").split(","):
            arg = arg.strip()
            want.append(_lib._i64p if arg.startswith("const int64_t*")
                        else ctypes.c_void_p if "*" in arg or arg.startswith("sea_stream_t")
                        else ctypes.c_int64 if arg.startswith("int64_t") else ctypes.c_int)
        assert list(argtypes) == want, name
    args = re.search(r"^int %s\((.*?)\);" % ENTRY, code, re.M | re.S).group(1)
    assert re.search(r"float\* dq, float\* dk, float\* dv, void\* workspace, int64_t workspace_bytes, int form,\s*sea_stream_t stream$", args)


def test_refusals_before_any_launch(lib):
    def no(code, fragment, **kw):
        rc = _call(lib, **kw)
        assert rc == code and _err(lib).startswith(ENTRY + ": ") and fragment in _err(lib), (kw, rc, _err(lib))

    # ---- SEA_EINVAL: null pointers, dtype, shape, form
    for name in (*POINTERS, "qs", "ks", "vs"):
        no(EINVAL, "null pointer", **{name: None})
    for code in (3, -1):
        no(EINVAL, f"bad dtype {code}", dtype=code)
    for arg in ("N", "H", "T_dst", "T_src", "D", "stride"):
        for bad in (0, -4):
            no(EINVAL, "bad shape", **{arg: bad})
    for form in (3, -1):
        no(EINVAL, f"bad form {form}", form=form)
        assert lib.sea_sparse_attention_bwd_workspace_bytes(BF, 1, 2, 64, 64, 4096, form) == 0

    # ---- SEA_EUNSUPPORTED: head sizes, strides, alignment -- the same for every form
    for form in (AUTO, GATHER, ATOMIC):
        no(EUNSUPPORTED, "D=36 must be a multiple of 8", D=36, form=form)
        no(EUNSUPPORTED, "D=520 must be a multiple of 8 and <= 512", D=520, form=form)
        no(EUNSUPPORTED, "D=260 must be a multiple of 4 and <= 256", dtype=F32, D=260, form=form)
        for sarg in ("qs", "ks", "vs"):
            no(EUNSUPPORTED, "row strides must be multiples of 8 elements", form=form, **{sarg: _s(2 * 64 * 64, 64 * 64 + 4, 64)})
        no(EUNSUPPORTED, "row strides must be multiples of 4 elements", dtype=F32, form=form, qs=_s(2 * 64 * 64, 64 * 64, 66))
        for name in ALIGNED:
            no(EUNSUPPORTED, "q/k/v/dout/dq/dk/dv", form=form, **{name: ODD})
            no(EUNSUPPORTED, "must be 16-byte aligned", form=form, **{name: ODD})
    no(EUNSUPPORTED, "q/k/v/dout/dq/dk/dv must be 16-byte aligned", form=ATOMIC, dk=ODD)     # the issue's case, to the letter
    no(EUNSUPPORTED, "q/k/v/dout/dq/dk/dv must be 16-byte aligned", dtype=F32, D=128, form=ATOMIC, dout=ODD)   # fp32: new in ABI 7
    for form in (AUTO, GATHER):
        no(EUNSUPPORTED, "dv/workspace must be 16-byte aligned", form=form, ws=ODD)
    # the atomic form reads neither workspace nor workspace_bytes: a misaligned, NULL or short one gets as far as the next refusal
    for ws, nb in ((ODD, 0), (None, 0), (ODD, -1)):
        no(EUNSUPPORTED, "must be 16-byte aligned", form=ATOMIC, ws=ws, ws_bytes_=nb, dk=ODD)
        no(EUNSUPPORTED, "must be 16-byte aligned", dtype=F32, D=128, form=AUTO, ws=ws, ws_bytes_=nb, dk=ODD)

    # ---- the lane rule: the gather form has no kernel above 16 lanes per row
    no(EUNSUPPORTED, "SEA_ATTN_BWD_GATHER has no kernel for rows of 32 lanes (D=128)", dtype=F32, D=128, form=GATHER)
    no(EUNSUPPORTED, "SEA_ATTN_BWD_GATHER has no kernel for rows of 32 lanes (D=256)", dtype=BF, D=256, form=GATHER)
    no(EUNSUPPORTED, "SEA_ATTN_BWD_GATHER has no kernel for rows of 64 lanes (D=256)", dtype=F32, D=256, form=GATHER)

    # ---- the workspace, where the gather form runs
    need = ws_bytes(1, 2, 64, 4096)
    assert lib.sea_sparse_attention_bwd_workspace_bytes(BF, 1, 2, 64, 64, 4096, AUTO) == need
    for form in (AUTO, GATHER):
        no(EINVAL, f"workspace of {need} bytes (NULL), need {need}", form=form, ws=None)
        no(EINVAL, f"workspace of {need - 1} bytes, need {need}", form=form, ws_bytes_=need - 1)
        no(EINVAL, f"workspace of 0 bytes (NULL), need {need}", form=form, ws=None, ws_bytes_=0)


@pytest.mark.parametrize("args", [(F32, 1, 3, 100, 16, 700), (BF, 2, 32, 4096, 64, 300000), (BF, 1, 1, 8, 32, 4)])
def test_workspace_bytes_follow_the_layout(lib, args):
    dtype, N, H, T_src, D, stride = args
    want = ws_bytes(N, H, T_src, stride)
    if args == (BF, 1, 1, 8, 32, 4):
        assert 128 * N > 16 * N * stride and want == 2 * 4 * 12 + 128          # the chunk totals exceed the records
    query = lib.sea_sparse_attention_bwd_workspace_bytes
    assert query(dtype, N, H, T_src, D, stride, AUTO) == want == query(dtype, N, H, T_src, D, stride, GATHER)
    assert query(dtype, N, H, T_src, D, stride, ATOMIC) == 0                   # pinned: the atomic form takes no workspace


def test_workspace_bytes_are_zero_without_the_gather_form(lib):
    query = lib.sea_sparse_attention_bwd_workspace_bytes
    for dtype, D in ((F32, 128), (BF, 256), (F16, 256), (F32, 256), (BF, 512)):            # 32 and 64 lanes per row
        for form in (AUTO, ATOMIC, GATHER):                                    # (GATHER there: an argument the entry refuses)
            assert query(dtype, 1, 2, 100, D, 700, form) == 0, (dtype, D, form)
    for dtype, D in ((F32, 64), (BF, 128), (F16, 80), (F32, 16)):              # up to 16 lanes: the rule's other side
        assert query(dtype, 1, 2, 100, D, 700, AUTO) == ws_bytes(1, 2, 100, 700)
    good = dict(dtype=BF, N=1, H=2, T_src=100, D=64, col_stride_n=700)
    for arg in ("N", "H", "T_src", "D", "col_stride_n"):
        for bad in (0, -1):
            a = dict(good, **{arg: bad})
            assert query(a["dtype"], a["N"], a["H"], a["T_src"], a["D"], a["col_stride_n"], AUTO) == 0, (arg, bad)
    assert query(7, 1, 2, 100, 64, 700, AUTO) == 0 and query(BF, 1, 2, 100, 36, 700, AUTO) == 0
