"""The C ABI of the distillation losses (include/sea_hip_train.h, version 2): four operators, four entries, the teacher given as
its score tensor or factored, and one rule for what is refused.  No GPU: every call here passes never-dereferenced pointers and
a null stream and ends in a refusal, which comes before any launch or memset.

The declarations against the ctypes binding argument by argument, the version numbers, the untouched inference ABI; then every
refusal, per entry and per form of the teacher, with its code under the one rule (SEA_EINVAL: null pointers, shapes that are not
positive, strides, alignment, a teacher given twice; SEA_EUNSUPPORTED: what the kernels have no form for) and the fragment of
`sea_last_error()` that names the entry and the argument."""
import ctypes
import os
import re

import pytest

from sea_attention_amd import _build, _lib

EINVAL, EUNSUPPORTED = -1, -2
A = ctypes.c_void_p(1 << 20)                     # 16-byte aligned, never dereferenced (the entries refuse first)
B = ctypes.c_void_p((1 << 20) + 4096)
ODD = ctypes.c_void_p((1 << 20) + 8)
EST, EST_BWD, SCORE, SCORE_BWD = "sea_kd_estimator_loss", "sea_kd_estimator_loss_bwd", "sea_kd_score_loss", "sea_kd_score_loss_bwd"
NAMES = ("sea_train_version", EST, EST_BWD, SCORE, SCORE_BWD)
F32, F16, BF = _lib.SEA_F32, _lib.SEA_F16, _lib.SEA_BF16


def _s(*v):
    return (ctypes.c_int64 * len(v))(*v)


def _rows(H, T, row):
    return _s(H * T * row, T * row, row)


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _err(lib):
    return lib.sea_last_error().decode()


def test_train_entries_are_declared_bound_and_apart_from_the_inference_abi(lib):
    root = os.path.join(os.path.dirname(__file__), "..")
    train = open(os.path.join(root, "include", "sea_hip_train.h")).read()
    main = open(os.path.join(root, "include", "sea_hip.h")).read()
    assert re.search(r"#define\s+SEA_TRAIN_ABI_VERSION\s+2\b", train) and re.search(r"#define\s+SEA_ABI_VERSION\s+7\b", main)
    assert lib.sea_train_version() == 2 == _lib.TRAIN_ABI_VERSION and lib.sea_version() == 7 == _lib.ABI_VERSION
    assert "WITHOUT a bump" not in train
    code = re.sub(r"/\*.*?\*/", "", train, flags=re.S)
    assert sorted(re.findall(r"^int (sea_\w+)\(", code, re.M)) == sorted(NAMES) == sorted(_lib._TRAIN_SIGNATURES)
    for name in NAMES:
        decl = re.search(r"^int %s\((.*?)\);" % name, train, re.M | re.S)
        assert decl, name
        assert hasattr(lib, name)
        argtypes, restype = _lib._TRAIN_SIGNATURES[name]
        assert getattr(lib, name).argtypes == argtypes and restype is ctypes.c_int
        want = []                                                              # the binding matches the declaration, argument by argument
        for arg in decl.group(1).replace("\n", " ").split(","):
            arg = arg.strip()
            if arg != "void":
                want.append(_lib._i64p if arg.startswith("const int64_t*")
                            else ctypes.c_void_p if "*" in arg or arg.startswith("sea_stream_t")
                            else ctypes.c_int64 if arg.startswith("int64_t") else ctypes.c_int)
        assert list(argtypes) == want, name
        assert name not in _lib.EXPORTED_SYMBOLS and name not in main
    for name in (EST, SCORE, SCORE_BWD):                                       # either form of the teacher, in one order
        args = re.search(r"^int %s\((.*?)\);" % name, train, re.M | re.S).group(1)
        assert re.search(r"truth, int truth_dtype, const int64_t\* truth_strides,\s*const void\* teacher_q, const void\* teacher_k, "
                         r"int teacher_dtype,\s*const int64_t\* teacher_q_strides, const int64_t\* teacher_k_strides,",
                         args), name
    assert "truth" not in re.search(r"^int %s\((.*?)\);" % EST_BWD, train, re.M | re.S).group(1)
    for gone in ("sea_kd_estimator_loss_qk", "sea_kd_score_loss_qk", "sea_kd_score_loss_qk_bwd"):     # no _qk symbol anywhere
        assert gone not in code and gone not in _lib._TRAIN_SIGNATURES and not hasattr(lib, gone)
    declared = sorted(set(re.findall(r"\b(sea_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", main, flags=re.S))))
    assert len(declared) == 37 and sorted(_lib.EXPORTED_SYMBOLS) == declared
    assert any(h.endswith("sea_hip_train.h") for h in _build.HEADERS) and any(h.endswith("sea_kd.hpp") for h in _build.HEADERS)
    assert "sea_kd_loss.hip" in _build.SOURCES and "sea_kd_score_loss.hip" in _build.SOURCES


def _call(lib, name, form, N=1, H=2, T=64, D=64, T_M=32, qd=BF, xd=BF, td=BF, ed=BF, **kw):
    """`name` with good arguments for the teacher's `form` ("tensor" / "factored"; never-dereferenced pointers) except for what
    `kw` replaces"""
    rows = _rows(H, T, D)
    a = dict(q=A, k=B, qs=rows, ks=rows, est=A, es=_rows(H, T, T_M), truth=None, xs=None, tq=None, tk=None, tqs=None, tks=None,
             row_kl=A, row_mse=A, row_q=A, row_stats=A, pix_tgt=A, grad_loss=A, d_q=A, d_k=B, d_est=B)
    a.update(dict(truth=A, xs=_rows(H, T, T)) if form == "tensor" else dict(tq=A, tk=B, tqs=rows, tks=rows))
    a.update(kw)
    teacher = (a["truth"], xd, a["xs"], a["tq"], a["tk"], td, a["tqs"], a["tks"])
    if name == EST:
        return lib.sea_kd_estimator_loss(a["est"], ed, a["es"], *teacher, N, H, T, T_M, D, a["row_kl"], a["row_mse"], a["pix_tgt"],
                                         a["row_stats"], None)
    if name == EST_BWD:
        return lib.sea_kd_estimator_loss_bwd(a["est"], ed, a["es"], a["pix_tgt"], a["row_stats"], a["grad_loss"], N, H, T, T_M,
                                             a["d_est"], None)
    head = (a["q"], a["k"], qd, a["qs"], a["ks"], *teacher)
    if name == SCORE:
        return lib.sea_kd_score_loss(*head, N, H, T, D, a["row_kl"], a["row_mse"], a["row_q"], a["row_stats"], None)
    return lib.sea_kd_score_loss_bwd(*head, a["row_q"], a["row_stats"], a["grad_loss"], N, H, T, D, a["d_q"], a["d_k"], None)


OWN = {EST: ("est", "row_kl", "row_mse", "pix_tgt", "row_stats"), EST_BWD: ("est", "pix_tgt", "row_stats", "grad_loss", "d_est"),
       SCORE: ("q", "k", "row_kl", "row_mse", "row_q", "row_stats"),
       SCORE_BWD: ("q", "k", "row_q", "row_stats", "grad_loss", "d_q", "d_k")}
GARBAGE = ctypes.cast(ODD, _lib._i64p)           # a stride array that must not be looked at


@pytest.mark.parametrize("name,form", [(EST, "tensor"), (EST, "factored"), (EST_BWD, None), (SCORE, "tensor"), (SCORE, "factored"),
                                       (SCORE_BWD, "tensor"), (SCORE_BWD, "factored")])
def test_refusals_before_any_launch(lib, name, form):
    H, T, D, T_M = 2, 64, 64, 32
    score, est = name in (SCORE, SCORE_BWD), name in (EST, EST_BWD)

    def no(code, fragment, **kw):
        rc = _call(lib, name, form, **kw)
        assert rc == code and fragment in _err(lib), (kw, rc, _err(lib))

    # ---- every named null
    strides = [("es", "est_strides")] if est else [("qs", "q_strides"), ("ks", "k_strides")]
    for arg, shown in [*strides, *[(o, o) for o in OWN[name]]]:
        no(EINVAL, f"{name}: {shown} is null", **{arg: None})
    if form == "tensor":
        no(EINVAL, f"{name}: truth_strides is null", xs=None)
        no(EINVAL, f"{name}: teacher_q is null", truth=None)                   # neither form given: truth is named too
        no(EINVAL, "truth is null", truth=None)
        for arg in ("tq", "tk"):                                               # both forms given
            no(EINVAL, f"{name}: the teacher is given twice", **{arg: B})
        for arg in ("tqs", "tks"):
            no(EINVAL, f"{name}: the teacher is given twice", **{arg: _rows(H, T, D)})
    if form == "factored":
        for arg, shown in (("tq", "teacher_q"), ("tk", "teacher_k"), ("tqs", "teacher_q_strides"), ("tks", "teacher_k_strides")):
            no(EINVAL, f"{name}: {shown} is null", **{arg: None})
        no(EINVAL, "truth is null too", tq=None)

    # ---- bases, strides: SEA_EINVAL for every tensor the entry reads
    tensors = [("est", "es", "est", T_M)] if est else [("q", "qs", "q", D), ("k", "ks", "k", D)]
    tensors += {"tensor": [("truth", "xs", "truth", T)], "factored": [("tq", "tqs", "teacher_q", D), ("tk", "tks", "teacher_k", D)],
                None: []}[form]
    for arg, sarg, shown, row in tensors:
        no(EINVAL, f"{name}: {shown} rows must be 16-byte aligned", **{arg: ODD})                           # a misaligned base
        # a stride that breaks 16-byte rows (bf16: 4 elements are 8 bytes)
        no(EINVAL, f"{shown} rows must be 16-byte aligned", **{sarg: _s(H * T * row, T * row, row + 4)})
        no(EINVAL, f"{shown} rows must be 16-byte aligned", **{sarg: _s(H * T * row + 4, T * row, row)})
        # the entries take no innermost stride: it is 1, so rows of `row` elements cannot be closer than that (a view with an
        # innermost stride of 2 would need it), nor may a stride be negative
        no(EINVAL, f"{name}: bad {shown} strides", **{sarg: _s(H * T * row, T * row, row - 8)})
        no(EINVAL, f"{name}: bad {shown} strides", **{sarg: _s(-8, T * row, row)})
    if est:
        no(EINVAL, f"{name}: bad est strides", es=_s(H * T * T_M, T * T_M, 8))

    # ---- shapes and limits
    no(EINVAL, f"{name}: bad shape", T=0)
    T2 = 16385                                                                 # (its truth rows are misaligned too: the limit is first)
    big = dict(T=T2, qs=_rows(H, T2, D), ks=_rows(H, T2, D), es=_rows(H, T2, T_M))
    big.update({"tensor": dict(xs=_rows(H, T2, T2)), "factored": dict(tqs=_rows(H, T2, D), tks=_rows(H, T2, D)), None: {}}[form])
    no(EUNSUPPORTED, f"{name}: T=16385", **big)
    if score and form == "tensor":
        no(EUNSUPPORTED, f"{name}: T=16385", **{**big, "xs": _rows(H, T2, 16392)})
    if score or form == "factored":
        r72 = _rows(H, T, 72)
        no(EUNSUPPORTED, f"{name}: D=72", D=72, qs=r72, ks=r72, **(dict(tqs=r72, tks=r72) if form == "factored" else {}))
    if est:
        no(EUNSUPPORTED, f"{name}: T_m=30", T_M=30, es=_rows(H, T, 30))        # (rows of 30 are misaligned too: the limit is first)
        no(EUNSUPPORTED, f"{name}: T_m=30", T_M=30, es=_rows(H, T, 32))
        no(EUNSUPPORTED, f"{name}: T_m=516", T_M=516, es=_rows(H, T, 516))

    # ---- dtype codes: SEA_EUNSUPPORTED, the student's before the teacher's
    if est:
        for code in (3, 5, 7, -1):
            no(EUNSUPPORTED, f"{name}: unknown est_dtype {code}", ed=code)
        for code in (F32, F16):
            no(EINVAL, f"{name}: row_stats is null", ed=code, row_stats=None)  # taken: the next refusal is another
    if score:
        no(EUNSUPPORTED, "fp32 q / k", qd=F32)
        no(EUNSUPPORTED, "qk_dtype", qd=F32)
        no(EUNSUPPORTED, f"{name}: unknown qk_dtype 7", qd=7)
    if form == "tensor":
        no(EUNSUPPORTED, f"{name}: unknown truth_dtype -1", xd=-1)
        no(EUNSUPPORTED, f"{name}: unknown truth_dtype 7", xd=7)
        # the factored form's arguments are not looked at: a teacher_dtype that is no code (and, for the estimator, a D that is
        # no head size) gets as far as the outputs
        no(EINVAL, f"{name}: row_stats is null", td=99, row_stats=None, **(dict(D=-5) if est else {}))
    if form == "factored":
        no(EUNSUPPORTED, "fp32 teacher q / k", td=F32)
        no(EUNSUPPORTED, "teacher_dtype", td=F32)
        no(EUNSUPPORTED, f"{name}: unknown teacher_dtype 7", td=7)
        if score:                                                              # the teacher must have the student's type
            no(EUNSUPPORTED, "is not qk_dtype", qd=BF, td=F16)
            no(EUNSUPPORTED, "fp32 q / k", qd=F32, td=BF)
        # the tensor form's arguments are not looked at: garbage for truth_strides and truth_dtype gets as far as the outputs,
        # and as far as a shape the kernels do not take
        no(EINVAL, f"{name}: row_stats is null", xs=GARBAGE, xd=99, row_stats=None)
        no(EUNSUPPORTED, f"{name}: D=72", xs=GARBAGE, xd=99, D=72)
