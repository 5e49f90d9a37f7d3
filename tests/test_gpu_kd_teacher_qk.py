"""-m gpu: the distillation losses with the teacher factored -- `ops.kd_score_loss` / `ops.kd_estimator_loss` handed an
`ops.TeacherScores(q_t, k_t)` (include/sea_hip_train.h "the teacher", csrc/sea_kd_score_loss.hip) -- against the fp64 closed forms of
the two existing suites on the fp64 teacher product.

Kernel tier.  References: `KdScoreReference(q, k, q_t k_t^T)` and `KdReference(est, q_t k_t^T)`, the product in fp64 from the
rounded inputs.  Yardsticks: `torch_score_rows` / `torch_rows` on the CPU, fed the product in fp32 (not rounded to 16 bits: the
kernels' semantics), and their autograd with leaves in the inputs' dtypes.  Bars exactly as the existing suites set them:
`bar_of` per quantity, `row_bars` per row for d_q / d_k / d_est -- 4 times the yardstick's largest error, at least 2^-22 of the
magnitude; no bar comes from the kernels' output.  The backward runs with the upstream gradient g = N H T.  Inputs are strided
views inside NaN buffers (NaN rows and columns around q, k, teacher_q, teacher_k and est, NaN past column D).  Two runs are
bitwise equal, pix_tgt and d_est are exactly 0 on empty pixels.  Shapes: the smallest that reach each way the kernels can go
wrong (the tables at SCORE_CASES and EST_CASES).

Exactness.  A teacher that holds the student's own bits gives row_kl = row_mse = row_q = d_q = d_k = 0 exactly and equal halves
of row_stats: the teacher's and the student's tiles are staged, indexed and multiplied by the same code.

Memory.  Forward + backward of either factored op at T = 2048 allocates less than a quarter of ONE (N,H,T,T) 16-bit tensor.

Module tier.  `PerlinAttention` with both switches on and a `TeacherScores` truth: dense mode (head-chunked) against the layer
with the two terms replaced by the fp64 references and by the fp32 yardsticks; sparse mode, whose loss is the two ops' values plus
the context MSE; and the fallbacks (padded batch, fp32 data, switches off), bit for bit what the tensor `.dense()` gives.

[kd-qk-ref] lines print max err / bar per case; the MI355X values are in DESIGN.md 5.9."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from test_gpu_kd_loss import Cfg
from test_gpu_kd_loss import _RefTerm as _RefEstTerm
from test_gpu_kd_score_loss import _RefTerm as _RefScoreTerm
from test_gpu_kd_score_loss import _poisoned
from test_kd_loss_reference import FP_MIN16, KdReference, bar_of, torch_rows
from test_kd_score_loss_reference import KdScoreReference, row_bars, torch_score_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF = torch.float32, torch.float16, torch.bfloat16
# (N, H, T, D), dtype of q / k / teacher                    reaches
SCORE_CASES = [((1, 1, 1, 64), BF),                        # one key: loss and gradients exactly 0
               ((1, 2, 45, 64), F16),                      # one row block, ragged last tile, the diagonal tile only
               ((2, 3, 100, 80), BF),                      # N, H > 1, the zero-fragment k-step of both products
               ((1, 2, 300, 128), F16),                    # several row blocks and key tiles, the largest LDS plan
               ((1, 1, 1100, 64), BF)]                     # many workgroups in both backward passes, heaviest-first dispatch
# (N, H, T, T_M, D), est dtype, teacher dtype               reaches
EST_CASES = [((1, 2, 45, 32, 64), F32, F16),               # the smallest case: one tile, every row with empty pixels
             ((2, 3, 100, 64, 80), BF, BF),                # the zero-fragment k-step
             ((1, 2, 300, 96, 128), F16, BF),              # several key tiles: the carry crosses tiles, T_M no power of two
             ((1, 1, 530, 512, 64), BF, F16)]              # the widest map (8 pixels per lane); rows with empty pixels beside rows without


def _sid(case):
    (N, H, T, D), dt = case
    return f"{N}x{H}x{T}x{D}-{str(dt)[6:]}"


def _eid(case):
    (N, H, T, T_M, D), ed, td = case
    return f"{N}x{H}x{T}x{T_M}x{D}-{str(ed)[6:]}-{str(td)[6:]}"


def _dd(a, b):
    return a.double() @ b.double().transpose(-1, -2)


def _ff(a, b):
    return a.float() @ b.float().transpose(-1, -2)


def _randn(shape, g, dtype, scale=0.6):
    return (torch.randn(shape, generator=g) * scale).to(dtype)


@functools.lru_cache(maxsize=None)
def _score_case(idx):
    """Inputs (rounded to their dtype), the fp64 reference and the fp32 yardstick of SCORE_CASES[idx]; computed once, never changed."""
    (N, H, T, D), dt = SCORE_CASES[idx]
    g = torch.Generator().manual_seed(300 + idx)
    q, k, qt, kt = (_randn((N, H, T, D), g, dt) for _ in range(4))
    up = float(N * H * T)
    ref = KdScoreReference(q, k, _dd(qt, kt), g=up)
    ql, kl = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    row_kl, row_mse, row_q, row_stats, loss = torch_score_rows(ql, kl, _ff(qt, kt), FP_MIN16)
    (loss * up).backward()
    yard = dict(row_kl=row_kl.detach(), row_mse=row_mse.detach(), row_q=row_q, row_stats=row_stats, d_q=ql.grad, d_k=kl.grad)
    return q, k, qt, kt, ref, yard


@functools.lru_cache(maxsize=None)
def _est_case(idx):
    (N, H, T, T_M, D), ed, td = EST_CASES[idx]
    g = torch.Generator().manual_seed(400 + idx)
    est = _randn((N, H, T, T_M), g, ed, 2.0)
    qt, kt = _randn((N, H, T, D), g, td), _randn((N, H, T, D), g, td)
    up = float(N * H * T)
    ref = KdReference(est, _dd(qt, kt))
    leaf = est.clone().requires_grad_(True)
    row_kl, row_mse, pix_tgt, loss = torch_rows(leaf, _ff(qt, kt), fp_min=FP_MIN16)
    (loss * up).backward()
    yard = dict(row_kl=row_kl.detach(), row_mse=row_mse.detach(), pix_tgt=pix_tgt, d_est=leaf.grad)
    return est, qt, kt, ref, ref.d_est * up, yard


def _check(tag, got, yard, ref):
    bar = bar_of(yard, ref)
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"[kd-qk-ref] {tag}: max err {err:.3e} / bar {bar:.3e} = {err / bar if bar else 0.0:.3f}")
    return err <= bar, (tag, err, bar)


def _check_rows(tag, got, yard, ref):
    bars = row_bars(yard, ref)
    err = (got.double().cpu() - ref).abs().amax(-1)
    worst = (err / bars.clamp_min(1e-300)).max().item()
    print(f"[kd-qk-ref] {tag}: max err {err.max().item():.3e}, worst row at {worst:.3f} of its bar "
          f"(bars {bars.min().item():.3e} .. {bars.max().item():.3e})")
    return bool((err <= bars).all()), (tag, err.max().item(), worst)


def _loss_bar(yard, ref, N, H, T):
    """0.1 mean(row_kl) + mean(row_mse) / T: the rows' bars weighted the same way, plus the fp32 reduction of R values (the
    existing suites' bound)"""
    R = N * H * T
    return (0.1 * bar_of(yard["row_kl"], ref.row_kl) + bar_of(yard["row_mse"], ref.row_mse) / T
            + 2.0 ** -24 * (math.log2(R) + 4) * (0.1 * ref.row_kl.abs().mean().item() + ref.row_mse.abs().mean().item() / T))


def _score_twice(q_c, k_c, qt_c, kt_c, up):
    ts = ops.TeacherScores(_poisoned(qt_c), _poisoned(kt_c))
    q = _poisoned(q_c).detach().requires_grad_(True)
    k = _poisoned(k_c).detach().requires_grad_(True)
    assert ops.kd_score_loss_supported(q, k, ts) and ts.q.storage_offset() > 0
    runs = []
    for _ in range(2):
        q.grad = k.grad = None
        parts = ops.kd_score_loss_parts(q.detach(), k.detach(), ts)
        loss = ops.kd_score_loss(q, k, ts)
        assert loss.dim() == 0 and loss.dtype == F32 and loss.requires_grad
        (loss * up).backward()
        assert q.grad.dtype == q_c.dtype and k.grad.dtype == q_c.dtype
        assert q.grad.shape == q_c.shape and k.grad.shape == q_c.shape and q.grad.is_contiguous() and k.grad.is_contiguous()
        runs.append([*parts, loss.detach().clone(), q.grad.clone(), k.grad.clone()])
    torch.cuda.synchronize()
    names = ["row_kl", "row_mse", "row_q", "row_stats", "loss", "d_q", "d_k"]
    for nm, a, b in zip(names, *runs):
        assert torch.isfinite(a).all(), nm                                     # the NaN poison reached nothing
        assert torch.equal(a, b), f"{nm}: two launches differ"
    return dict(zip(names, (t.cpu() for t in runs[0])))


@pytest.mark.parametrize("idx", range(len(SCORE_CASES)), ids=[_sid(c) for c in SCORE_CASES])
def test_score_kernels_against_fp64_reference(idx):
    (N, H, T, D), dt = SCORE_CASES[idx]
    q_c, k_c, qt_c, kt_c, ref, yard = _score_case(idx)
    got = _score_twice(q_c, k_c, qt_c, kt_c, float(N * H * T))
    assert got["row_kl"].shape == (N, H, T) and got["row_stats"].shape == (N, H, T, 4)
    tag = "score " + _sid(SCORE_CASES[idx])
    results = [_check(f"{tag} {nm}", got[nm], yard[nm], getattr(ref, nm)) for nm in ("row_kl", "row_mse", "row_q", "row_stats")]
    results += [_check_rows(f"{tag} {nm}", got[nm], yard[nm], getattr(ref, nm)) for nm in ("d_q", "d_k")]
    bar_loss = _loss_bar(yard, ref, N, H, T)
    err_loss = abs(got["loss"].double().item() - ref.loss.item())
    print(f"[kd-qk-ref] {tag} loss: err {err_loss:.3e} / bar {bar_loss:.3e} = {err_loss / bar_loss if bar_loss else 0.0:.3f}")
    results.append((err_loss <= bar_loss, ("loss", err_loss, bar_loss)))
    assert all(ok for ok, _ in results), [info for ok, info in results if not ok]
    if T == 1:
        assert got["loss"].item() == 0 and torch.all(got["d_q"] == 0) and torch.all(got["d_k"] == 0)
        assert torch.all(got["row_kl"] == 0) and torch.all(got["row_mse"] == 0) and torch.all(got["row_q"] == 0)


@pytest.mark.parametrize("idx", range(len(EST_CASES)), ids=[_eid(c) for c in EST_CASES])
def test_estimator_kernel_against_fp64_reference(idx):
    (N, H, T, T_M, D), ed, td = EST_CASES[idx]
    est_c, qt_c, kt_c, ref, ref_d_est, yard = _est_case(idx)
    up = float(N * H * T)
    ts = ops.TeacherScores(_poisoned(qt_c), _poisoned(kt_c))
    est = _poisoned(est_c).detach().requires_grad_(True)
    assert ops.kd_estimator_loss_supported(est, ts)
    runs = []
    for _ in range(2):
        est.grad = None
        parts = ops.kd_estimator_loss_parts(est.detach(), ts)
        loss = ops.kd_estimator_loss(est, ts)
        assert loss.dim() == 0 and loss.dtype == F32 and loss.requires_grad
        (loss * up).backward()
        assert est.grad.dtype == ed
        runs.append([*parts, loss.detach().clone(), est.grad.clone()])
    torch.cuda.synchronize()
    names = ["row_kl", "row_mse", "pix_tgt", "row_stats", "loss", "d_est"]
    for nm, a, b in zip(names, *runs):
        assert torch.isfinite(a).all(), nm
        assert torch.equal(a, b), f"{nm}: two launches differ"
    row_kl, row_mse, pix_tgt, row_stats, loss, d_est = (t.cpu() for t in runs[0])
    assert row_kl.shape == (N, H, T) and pix_tgt.shape == (N, H, T, T_M) and row_stats.shape == (N, H, T, 2)
    assert torch.all(pix_tgt[..., ~ref.held] == 0) and torch.all(d_est[..., ~ref.held] == 0)     # empty pixels: exactly 0
    assert (~ref.held).any()                                                   # (rows with t + 1 < T_M always have some)
    if T > T_M == 512:
        assert ref.held.all(-1).any()                                          # ... beside rows that hold every pixel
    tag = "est " + _eid(EST_CASES[idx])
    results = [_check(f"{tag} {nm}", g, yard[nm], want) for nm, g, want in
               (("row_kl", row_kl, ref.row_kl), ("row_mse", row_mse, ref.row_mse), ("pix_tgt", pix_tgt, ref.pix_tgt))]
    # row_stats = {m_e, log S} has no yardstick of its own in `torch_rows`: m_e is a maximum of the inputs (exact), log S a sum
    # of at most T_M fp32 terms -- 2^-22 of the magnitude per term of the tree, the floor of `bar_of`, times log2(T_M) + 4
    st_err = (row_stats.double() - ref.row_stats).abs().max().item()
    st_bar = 2.0 ** -22 * ref.row_stats.abs().max().item() * (math.log2(T_M) + 4)
    print(f"[kd-qk-ref] {tag} row_stats: max err {st_err:.3e} / bar {st_bar:.3e} = {st_err / st_bar:.3f}")
    results.append((st_err <= st_bar, ("row_stats", st_err, st_bar)))
    results.append(_check_rows(f"{tag} d_est", d_est, yard["d_est"], ref_d_est))
    bar_loss = _loss_bar(yard, ref, N, H, T)
    err_loss = abs(loss.double().item() - ref.loss.item())
    print(f"[kd-qk-ref] {tag} loss: err {err_loss:.3e} / bar {bar_loss:.3e} = {err_loss / bar_loss:.3f}")
    results.append((err_loss <= bar_loss, ("loss", err_loss, bar_loss)))
    assert all(ok for ok, _ in results), [info for ok, info in results if not ok]


# ---- exactness -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,H,T,D,dt", [(1, 2, 45, 64, F16), (2, 3, 100, 80, BF)])
def test_a_teacher_with_the_students_bits_gives_exact_zeros(N, H, T, D, dt):
    g = torch.Generator().manual_seed(21)
    q, k = _randn((N, H, T, D), g, dt), _randn((N, H, T, D), g, dt)
    got = _score_twice(q, k, q.clone(), k.clone(), float(N * H * T))
    for nm in ("row_kl", "row_mse", "row_q", "loss", "d_q", "d_k"):
        assert torch.all(got[nm] == 0), nm
    st = got["row_stats"]
    assert torch.equal(st[..., :2], st[..., 2:]) and st[..., 1].abs().max().item() > 0


@pytest.mark.parametrize("N,H,T,D,dt", [(1, 2, 45, 64, F16), (2, 3, 100, 80, BF)])
def test_all_inputs_zero_gives_exact_zeros(N, H, T, D, dt):
    z = torch.zeros((N, H, T, D), dtype=dt)
    got = _score_twice(z, z.clone(), z.clone(), z.clone(), float(N * H * T))
    for nm in ("row_kl", "row_mse", "row_q", "loss", "d_q", "d_k"):
        assert torch.all(got[nm] == 0), nm
    want = torch.log(torch.arange(1, T + 1, dtype=F32))
    assert (got["row_stats"][..., 1] - want).abs().max().item() <= 2.0 ** -22 * max(want.max().item(), 1.0)


# ---- memory ----------------------------------------------------------------------------------------------------------------
def test_forward_and_backward_allocate_nothing_t_by_t():
    """(1,2,2048,64) bf16, T_M = 64: one (N,H,T,T) bf16 tensor is 16 MiB.  The peak of forward + backward above what is allocated
    when the op is called (its inputs) stays below a quarter of that; the op's own outputs are about 1 - 1.5 MiB."""
    N, H, T, D, T_M = 1, 2, 2048, 64, 64
    g = torch.Generator().manual_seed(31)
    q, k, qt, kt = (_randn((N, H, T, D), g, BF).to(DEV) for _ in range(4))
    est = _randn((N, H, T, T_M), g, BF, 2.0).to(DEV)
    ts = ops.TeacherScores(qt, kt)
    limit = N * H * T * T * 2 // 4
    for name, run in (("score", lambda: ops.kd_score_loss(q.requires_grad_(True), k.requires_grad_(True), ts)),
                      ("estimator", lambda: ops.kd_estimator_loss(est.requires_grad_(True), ts))):
        run().backward()                                                       # (warm: the first call loads the code object)
        q.grad = k.grad = est.grad = None
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = run()
        loss.backward()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
        print(f"[kd-qk-mem] {name}: peak {peak / 2 ** 20:.2f} MiB above the inputs ({before / 2 ** 20:.2f} MiB), limit {limit / 2 ** 20:.0f} MiB")
        assert torch.isfinite(loss) and 0 < peak < limit, (name, peak, limit)


# ---- refusals --------------------------------------------------------------------------------------------------------------
def test_what_the_factored_kernels_do_not_take_is_refused():
    big = torch.zeros((1, 2, 16, 128), dtype=BF, device=DEV)
    q, k = big[..., :64], big[..., 64:]
    est = torch.zeros((1, 2, 16, 8), dtype=BF, device=DEV)
    good = ops.TeacherScores(q.clone(), k.clone())
    assert ops.kd_score_loss_supported(q, k, good) and ops.kd_estimator_loss_supported(est, good)
    for bad in (ops.TeacherScores(big[..., ::2], big[..., ::2]),               # an innermost stride of 2
                ops.TeacherScores(big[..., :72], big[..., :72]),               # D = 72
                ops.TeacherScores(q.float(), k.float()),                       # fp32
                ops.TeacherScores(big[..., 4:68], big[..., 4:68])):            # rows that start 8 bytes off
        assert not ops.kd_score_loss_supported(q, k, bad) and not ops.kd_estimator_loss_supported(est, bad)
        with pytest.raises(RuntimeError, match="kd_score_loss_supported"):
            ops.kd_score_loss(q, k, bad)
        with pytest.raises(RuntimeError, match="kd_estimator_loss_supported"):
            ops.kd_estimator_loss(est, bad)
    other = ops.TeacherScores(q.half(), k.half())                              # not the student's type: the score term only
    assert not ops.kd_score_loss_supported(q, k, other) and ops.kd_estimator_loss_supported(est, other)
    with pytest.raises(RuntimeError, match="kd_score_loss_supported"):
        ops.kd_score_loss_parts(q, k, other)
    with pytest.raises(RuntimeError, match="kd_estimator_loss_supported"):
        ops.kd_estimator_loss_parts(est[..., :6], good)                        # T_M = 6


# ---- module tier -------------------------------------------------------------------------------------------------------
H_, D_, T_, TM_, K_ = 4, 64, 96, 32, 8


@pytest.fixture(scope="module")
def bundle():
    S.seed(42)
    pc = PerlinAttentionConfig(k=K_, attention_predictor_length=TM_, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix')
    layer32 = PerlinSelfAttention(Cfg(H_ * D_, H_, T_), pc).to(DEV).eval()     # eval(): the torch form draws no rank jitter
    layer16 = copy.deepcopy(layer32).to(BF)
    S.seed(1)
    x = torch.randn((1, H_, T_, D_), device=DEV)
    idx = torch.arange(T_, device=DEV)
    mask = ((idx.view(1, T_) > idx.view(T_, 1)) * FP_MIN16).view(1, 1, T_, T_)
    qt, kt = torch.randn((1, H_, T_, D_), device=DEV) * 0.5, torch.randn((1, H_, T_, D_), device=DEV) * 0.5
    context_truth = torch.randn((1, T_, H_ * D_), device=DEV)
    return {BF: layer16, F32: layer32}, x, mask, qt, kt, context_truth


def _run(bundle, dtype=BF, benchmarking=False, on=True, chunk=None, mask=None, dense_truth=False):
    """`PerlinAttention.forward` called directly with leaf q_for_score / k_for_score and a `TeacherScores` truth (or, with
    `dense_truth`, the tensor its `.dense()` gives); returns (output, q_for_score, k_for_score)"""
    layers, x, causal, qt, kt, context_truth = bundle
    layer = layers[dtype]
    att = layer.attention
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = benchmarking
    x = x.to(dtype)
    q, k, v = x * D_ ** -0.5, x.clone(), x.clone()
    qs, ks = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    ts = ops.TeacherScores(qt.to(dtype), kt.to(dtype))
    att.fused_kd_score_loss, att.fused_kd_loss, att.dense_head_chunk = on, on, chunk
    layer.zero_grad()
    try:
        out = att(q, k, v, q, k, v, qs, ks, (causal if mask is None else mask).to(dtype), ts.dense() if dense_truth else ts,
                  context_truth.to(F32 if benchmarking else dtype))
    finally:
        att.fused_kd_score_loss, att.fused_kd_loss, att.dense_head_chunk = False, False, None
    return out, qs, ks


def _check_bf16_grad(tag, got, yard, ref):
    """A gradient the bf16 layer delivers: `bar_of`, but no less than two bf16 steps at the gradient's largest magnitude.  In all
    three runs the value passes two roundings to bf16 -- the term's own gradient, then autograd's sum of it and the layer's other
    contributions -- and the runs differ only in the term: two values that agree far below a bf16 step before a rounding can
    still land on neighbouring bf16 numbers, once per rounding.  Which elements do so is chance (the yardstick, at fp32
    accuracy, flips fewer of them than 16-bit dS operands do), so `bar_of` alone would hold the kernels to the yardstick's luck.
    A bf16 step at magnitude m is 2^(floor(log2 m) - 7)."""
    top = ref.abs().max().item()
    floor = 2.0 * 2.0 ** (math.floor(math.log2(top)) - 7) if top > 0 else 0.0
    bar = max(bar_of(yard, ref), floor)
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"[kd-qk-ref] {tag}: max err {err:.3e} / bar {bar:.3e} = {err / bar if bar else 0.0:.3f} "
          f"(bar_of {bar_of(yard, ref):.3e}, two bf16 steps at {top:.3e}: {floor:.3e})")
    return err <= bar, (tag, err, bar)


def test_dense_mode_both_terms_against_the_references(bundle, monkeypatch):
    weight = bundle[0][BF].attention.attention_predictor_enc[0].weight

    def run():
        out, qs, ks = _run(bundle, chunk=2)
        out.loss.backward()
        return out.loss.detach().double().cpu(), {"attention_predictor_enc[0].weight": weight.grad.detach().double().cpu().clone(),
                                                  "q_for_score": qs.grad.double().cpu(), "k_for_score": ks.grad.double().cpu()}
    seen = []
    real_s, real_e = ops.kd_score_loss, ops.kd_estimator_loss
    with monkeypatch.context() as m:                                           # the kernels, and that the layer hands them the factored truth
        m.setattr(ops, "kd_score_loss", lambda q, k, t: seen.append(t) or real_s(q, k, t))
        m.setattr(ops, "kd_estimator_loss", lambda e, t: seen.append(t) or real_e(e, t))
        loss_k, g_k = run()
    assert len(seen) == 2 and all(isinstance(t, ops.TeacherScores) for t in seen)
    with monkeypatch.context() as m:                                           # fp32 torch, products not rounded: the yardstick
        m.setattr(ops, "kd_score_loss", lambda q, k, t: torch_score_rows(q, k, _ff(t.q, t.k), FP_MIN16)[-1])
        m.setattr(ops, "kd_estimator_loss", lambda e, t: torch_rows(e.float().cpu(), _ff(t.q, t.k).cpu(), fp_min=FP_MIN16)[-1].to(e.device))
        loss_y, g_y = run()
    with monkeypatch.context() as m:                                           # fp64 closed forms: the reference
        m.setattr(ops, "kd_score_loss", lambda q, k, t: _RefScoreTerm.apply(q, k, _dd(t.q.cpu(), t.k.cpu())))
        m.setattr(ops, "kd_estimator_loss", lambda e, t: _RefEstTerm.apply(e, _dd(t.q.cpu(), t.k.cpu())))
        loss_r, g_r = run()
    results = [_check("dense chunk=2 loss", loss_k, loss_y, loss_r)]
    for nm in g_k:
        results.append(_check_bf16_grad(f"dense chunk=2 d {nm}", g_k[nm], g_y[nm], g_r[nm]))
    assert all(ok for ok, _ in results), [info for ok, info in results if not ok]
    assert all(g_r[nm].abs().max().item() > 0 for nm in g_r)


def test_sparse_mode_loss_is_the_two_terms_and_the_context_term(bundle, monkeypatch):
    seen = {}
    real_s, real_e = ops.kd_score_loss, ops.kd_estimator_loss
    with monkeypatch.context() as m:
        m.setattr(ops, "kd_score_loss", lambda q, k, t: seen.setdefault("score", (q, k, t)) and real_s(q, k, t))
        m.setattr(ops, "kd_estimator_loss", lambda e, t: seen.setdefault("est", (e, t)) and real_e(e, t))
        out, qs, ks = _run(bundle, benchmarking=True)
    assert isinstance(seen["score"][2], ops.TeacherScores) and isinstance(seen["est"][1], ops.TeacherScores)
    with torch.no_grad():
        want = (real_e(seen["est"][0].detach(), seen["est"][1]).item() + real_s(qs.detach(), ks.detach(), seen["score"][2]).item()
                + F.mse_loss(bundle[5].to(out.context_layer.dtype), out.context_layer.detach()).item())
    assert torch.is_tensor(out.loss) and out.loss.requires_grad and out.loss.dim() == 0
    # three fp32 values added in the layer's order: two roundings of a sum
    assert abs(out.loss.item() - want) <= 2.0 ** -22 * max(1.0, abs(want)), (out.loss.item(), want)
    out.loss.backward()
    assert qs.grad is not None and torch.isfinite(qs.grad).all() and ks.grad.abs().max().item() > 0
    g = bundle[0][BF].attention.attention_predictor_enc[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0


@pytest.mark.parametrize("what", ["padded", "fp32", "switches off"])
def test_fallbacks_are_the_dense_tensors_bit_for_bit(bundle, monkeypatch, what):
    causal = bundle[2]
    kw = {}
    if what == "padded":
        padded = causal.clone()
        padded[:, :, T_ - 8:, :] = FP_MIN16                                    # the last 8 query rows are padding
        kw = dict(mask=padded)
    elif what == "fp32":
        kw = dict(dtype=F32)
    else:
        kw = dict(on=False)
    calls = []
    real_s, real_e = ops.kd_score_loss, ops.kd_estimator_loss
    with monkeypatch.context() as m:
        m.setattr(ops, "kd_score_loss", lambda *a: calls.append(a) or real_s(*a))
        m.setattr(ops, "kd_estimator_loss", lambda *a: calls.append(a) or real_e(*a))
        want, _q0, _k0 = _run(bundle, chunk=2, dense_truth=True, **kw)
        got, _q1, _k1 = _run(bundle, chunk=2, **kw)
    if what == "fp32":
        # fp32 data: the score term falls back; the estimator's kernels take an fp32 TENSOR, so the dense run may use them --
        # a TeacherScores of fp32 is outside them and is made dense first, which is the same tensor
        assert all(not isinstance(a[-1], ops.TeacherScores) for a in calls)
    else:
        assert calls == []
    assert torch.isfinite(want.loss) and torch.equal(got.loss, want.loss) and torch.equal(got.context_layer, want.context_layer)
