"""-m gpu: `ops.kd_score_loss` (csrc/sea_kd_score_loss.hip) against the fp64 closed forms of tests/test_kd_score_loss_reference.py.

Kernel tier.  The reference is `KdScoreReference` (fp64, held to fp64 autograd through the module's expression by the CPU suite)
on the same rounded inputs; the yardstick is `torch_score_rows` on the CPU: q k^T in fp32 (not rounded to 16 bits, as in the
kernels), the body of `_kl_and_mse` per row, and its autograd with leaves in q's dtype -- the kernels write d_q and d_k in that
dtype as well.  Per case and quantity the kernels' largest error may be 4 times the yardstick's, at least 2^-22 of the
quantity's largest magnitude (`bar_of`); for d_q and d_k the bar is taken per row (`row_bars`), because the gradient's size
falls with the row length.  No bar comes from the kernels' own output.  The backward runs with the upstream gradient
g = N H T -- `(loss * g).backward()` for kernels and yardstick alike -- which keeps fp16 gradients out of the subnormal range and
checks that g is applied.  Inputs are strided views inside NaN buffers: NaN rows and columns around every tensor, NaN in every
s > t position of the teacher's scores, NaN beyond column D of q and k.  Shapes: the smallest that reach each way the kernels
can go wrong (the table at CASES).

Module tier.  `PerlinAttention.fused_kd_score_loss` in dense mode (head-chunked) against the layer with this one term replaced
by `KdScoreReference` (the reference) and by `torch_score_rows` (the yardstick); in sparse mode, where it adds the term; and its
fallbacks (a padded batch, fp32 data), where it changes nothing.

[kd-score-ref] lines print max err / bar per case; the MI355X values are in DESIGN.md 5.8."""
import copy
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from test_gpu_kd_loss import Cfg
from test_kd_loss_reference import FP_MIN16, bar_of
from test_kd_score_loss_reference import KdScoreReference, row_bars, torch_score_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF = torch.float32, torch.float16, torch.bfloat16
# (N, H, T, D), q / k dtype, truth dtype                     reaches
CASES = [((1, 1, 1, 64), BF, BF),                          # one key: loss and gradients exactly 0
         ((1, 2, 45, 64), F16, F32),                       # one row block, ragged last tile, the diagonal tile only
         ((2, 3, 100, 80), BF, F16),                       # N, H > 1, zero-padded k-step, T no multiple of 16 or of a 16-byte chunk
         ((1, 2, 300, 128), F16, BF),                      # several row blocks and key tiles, several column-pass sweeps
         ((1, 1, 1100, 64), BF, BF)]                       # many workgroups in both backward passes, heaviest-first dispatch


def _poisoned(values, keep=None):
    """`values` (N,H,T,W) as a strided DEVICE view with 16-byte-aligned rows inside a NaN buffer (a NaN row before and after,
    NaN columns left and right); `keep` (T,W) bool: NaN elsewhere inside the view too.  (test_gpu_kd_loss.py's, for T = 1 too.)"""
    N, H, T, W = values.shape
    buf = torch.full((N, H, T + 2, (W + 7) // 8 * 8 + 16), float("nan"), dtype=values.dtype, device=DEV)
    view = buf[:, :, 1:T + 1, 8:8 + W]
    v = values.to(DEV)
    view.copy_(v if keep is None else torch.where(keep.to(DEV), v, torch.full_like(v, float("nan"))))
    assert view.data_ptr() % 16 == 0 and view.stride(2) > W and view.storage_offset() > 0
    return view


def _id(case):
    (N, H, T, D), qd, xd = case
    return f"{N}x{H}x{T}x{D}-{str(qd)[6:]}-{str(xd)[6:]}"


@functools.lru_cache(maxsize=None)
def _case(idx):
    """Inputs (rounded to their dtypes), the fp64 reference and the fp32 yardstick of CASES[idx]; computed once, never changed."""
    (N, H, T, D), qd, xd = CASES[idx]
    g = torch.Generator().manual_seed(200 + idx)
    q = (torch.randn((N, H, T, D), generator=g) * 0.6).to(qd)
    k = (torch.randn((N, H, T, D), generator=g) * 0.6).to(qd)
    truth = (torch.randn((N, H, T, T), generator=g) * 3.0).to(xd)
    up = float(N * H * T)
    ref = KdScoreReference(q, k, truth, g=up)
    ql, kl = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    row_kl, row_mse, row_q, row_stats, loss = torch_score_rows(ql, kl, truth, FP_MIN16)
    (loss * up).backward()
    yard = dict(row_kl=row_kl.detach(), row_mse=row_mse.detach(), row_q=row_q, row_stats=row_stats, d_q=ql.grad, d_k=kl.grad)
    return q, k, truth, ref, yard


def _check(tag, got, yard, ref):
    bar = bar_of(yard, ref)
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"[kd-score-ref] {tag}: max err {err:.3e} / bar {bar:.3e} = {err / bar if bar else 0.0:.3f}")
    return err <= bar, (tag, err, bar)


def _check_rows(tag, got, yard, ref):
    bars = row_bars(yard, ref)
    err = (got.double().cpu() - ref).abs().amax(-1)
    worst = (err / bars.clamp_min(1e-300)).max().item()
    print(f"[kd-score-ref] {tag}: max err {err.max().item():.3e}, worst row at {worst:.3f} of its bar "
          f"(bars {bars.min().item():.3e} .. {bars.max().item():.3e})")
    return bool((err <= bars).all()), (tag, err.max().item(), worst)


def _run_twice(q_c, k_c, truth_c, up):
    T = q_c.shape[2]
    alive = torch.arange(T).view(1, T) <= torch.arange(T).view(T, 1)
    truth = _poisoned(truth_c, keep=alive)
    q = _poisoned(q_c).detach().requires_grad_(True)
    k = _poisoned(k_c).detach().requires_grad_(True)
    assert ops.kd_score_loss_supported(q, k, truth)
    runs = []
    for _ in range(2):
        q.grad = k.grad = None
        parts = ops.kd_score_loss_parts(q.detach(), k.detach(), truth)
        loss = ops.kd_score_loss(q, k, truth)
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


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_kernels_against_fp64_reference(idx):
    (N, H, T, D), qd, xd = CASES[idx]
    q_c, k_c, truth_c, ref, yard = _case(idx)
    got = _run_twice(q_c, k_c, truth_c, float(N * H * T))
    assert got["row_kl"].shape == (N, H, T) and got["row_mse"].shape == (N, H, T) and got["row_q"].shape == (N, H, T)
    assert got["row_stats"].shape == (N, H, T, 4) and all(got[nm].dtype == F32 for nm in ("row_kl", "row_mse", "row_q", "row_stats"))
    tag = _id(CASES[idx])
    results = [_check(f"{tag} {nm}", got[nm], yard[nm], getattr(ref, nm)) for nm in ("row_kl", "row_mse", "row_q", "row_stats")]
    results += [_check_rows(f"{tag} {nm}", got[nm], yard[nm], getattr(ref, nm)) for nm in ("d_q", "d_k")]
    # the loss is 0.1 mean(row_kl) + mean(row_mse) / T: it may miss by the rows' bars weighted the same way, plus the fp32
    # reduction of R values (a tree: log2 R + 4 roundings of partial sums no larger than the sum of magnitudes)
    R = N * H * T
    bar_loss = (0.1 * bar_of(yard["row_kl"], ref.row_kl) + bar_of(yard["row_mse"], ref.row_mse) / T
                + 2.0 ** -24 * (math.log2(R) + 4) * (0.1 * ref.row_kl.abs().mean().item() + ref.row_mse.abs().mean().item() / T))
    err_loss = abs(got["loss"].double().item() - ref.loss.item())
    print(f"[kd-score-ref] {tag} loss: err {err_loss:.3e} / bar {bar_loss:.3e} = {err_loss / bar_loss if bar_loss else 0.0:.3f}")
    results.append((err_loss <= bar_loss, ("loss", err_loss, bar_loss)))
    assert all(ok for ok, _ in results), [info for ok, info in results if not ok]
    if T == 1:
        assert got["loss"].item() == 0 and torch.all(got["d_q"] == 0) and torch.all(got["d_k"] == 0)
        assert torch.all(got["row_kl"] == 0) and torch.all(got["row_mse"] == 0) and torch.all(got["row_q"] == 0)


@pytest.mark.parametrize("N,H,T,D,qd", [(1, 2, 45, 64, F16), (2, 3, 100, 80, BF)])
def test_uniform_rows_are_exactly_zero(N, H, T, D, qd):
    """q = 0 and truth = 0: p = tgt = 1 / (t + 1) in every row, so the three row sums and both gradients are exactly 0 -- diagonal
    masking and tile edges without rounding (k is random: with q = 0 it reaches nothing)."""
    g = torch.Generator().manual_seed(11)
    k = (torch.randn((N, H, T, D), generator=g) * 0.6).to(qd)
    got = _run_twice(torch.zeros((N, H, T, D), dtype=qd), k, torch.zeros((N, H, T, T), dtype=qd), float(N * H * T))
    for nm in ("row_kl", "row_mse", "row_q", "loss", "d_q", "d_k"):
        assert torch.all(got[nm] == 0), nm
    want = torch.log(torch.arange(1, T + 1, dtype=F32))
    st = got["row_stats"]
    assert torch.all(st[..., 0] == 0) and torch.all(st[..., 2] == 0) and torch.equal(st[..., 1], st[..., 3])
    assert (st[..., 1] - want).abs().max().item() <= 2.0 ** -22 * want.max().item()


def test_what_the_kernels_do_not_take_is_refused():
    q = torch.zeros((1, 2, 16, 128), dtype=BF, device=DEV)
    truth = torch.zeros((1, 2, 16, 16), dtype=BF, device=DEV)
    assert ops.kd_score_loss_supported(q[..., :64], q[..., 64:], truth)
    for bad_q, bad_k in ((q[..., ::2], q[..., ::2]),                  # an innermost stride of 2
                         (q[..., :72], q[..., :72]),                  # D = 72
                         (q[..., :64].float(), q[..., :64].float()),  # fp32 q / k
                         (q[..., :64], q[..., :64].half()),           # q and k of two types
                         (q[..., 4:68], q[..., :64])):                # rows that start 8 bytes off
        assert not ops.kd_score_loss_supported(bad_q, bad_k, truth)
        with pytest.raises(RuntimeError, match="kd_score_loss_supported"):
            ops.kd_score_loss(bad_q, bad_k, truth)
    ql = q[..., :64].clone().requires_grad_(True)
    loss = ops.kd_score_loss(ql, q[..., 64:], truth)                 # k needs no gradient: it gets none
    loss.backward()
    assert ql.grad is not None and torch.all(ql.grad == 0)


# ---- module tier -------------------------------------------------------------------------------------------------------
H_, D_, T_, TM_, K_ = 4, 64, 96, 32, 8


@pytest.fixture(scope="module")
def layers_and_inputs():
    S.seed(42)
    pc = PerlinAttentionConfig(k=K_, attention_predictor_length=TM_, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix')
    layer32 = PerlinSelfAttention(Cfg(H_ * D_, H_, T_), pc).to(DEV).eval()     # eval(): the torch form draws no rank jitter
    layer16 = copy.deepcopy(layer32).to(BF)
    S.seed(1)
    x = torch.randn((1, H_, T_, D_), device=DEV)
    fp_min = torch.finfo(torch.float16).min / 2
    idx = torch.arange(T_, device=DEV)
    mask = ((idx.view(1, T_) > idx.view(T_, 1)) * fp_min).view(1, 1, T_, T_)
    scores_truth = torch.randn((1, H_, T_, T_), device=DEV) * 2.0
    context_truth = torch.randn((1, T_, H_ * D_), device=DEV)
    return {BF: layer16, F32: layer32}, x, mask, scores_truth, context_truth


def _run(bundle, dtype=BF, benchmarking=False, score=False, est=False, chunk=None, mask=None):
    """`PerlinAttention.forward` called directly with leaf q_for_score / k_for_score; returns (output, q_for_score, k_for_score)"""
    layers, x, causal, scores_truth, context_truth = bundle
    layer = layers[dtype]
    att = layer.attention
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = benchmarking
    x = x.to(dtype)
    q, k, v = x * D_ ** -0.5, x.clone(), x.clone()
    qs, ks = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    att.fused_kd_score_loss, att.fused_kd_loss, att.dense_head_chunk = score, est, chunk
    layer.zero_grad()
    # (the teacher's context in the dtype of the layer's own: sparse mode's context is fp32, and `F.mse_loss` has no backward
    # across two dtypes)
    try:
        out = att(q, k, v, q, k, v, qs, ks, (causal if mask is None else mask).to(dtype), scores_truth.to(dtype),
                  context_truth.to(F32 if benchmarking else dtype))
    finally:
        att.fused_kd_score_loss, att.fused_kd_loss, att.dense_head_chunk = False, False, None
    return out, qs, ks


class _RefTerm(torch.autograd.Function):
    """The student-score term in fp64 on the CPU (`KdScoreReference`), standing in for `ops.kd_score_loss` in the reference run."""

    @staticmethod
    def forward(ctx, q, k, truth):
        ref = KdScoreReference(q.detach().cpu(), k.detach().cpu(), truth.detach().cpu())
        ctx.d_q, ctx.d_k, ctx.like = ref.d_q, ref.d_k, q
        return ref.loss.to(torch.float32).to(q.device)

    @staticmethod
    def backward(ctx, g):
        g = g.double().cpu()
        return ((ctx.d_q * g).to(ctx.like.dtype).to(ctx.like.device), (ctx.d_k * g).to(ctx.like.dtype).to(ctx.like.device), None)


def _yard_term(q, k, truth):
    return torch_score_rows(q, k, truth, FP_MIN16)[-1]


def test_dense_mode_fused_term_against_the_reference(layers_and_inputs, monkeypatch):
    def run():
        out, qs, ks = _run(layers_and_inputs, chunk=2, score=True)
        out.loss.backward()
        return out.loss.detach().double().cpu(), {"q_for_score": qs.grad.double().cpu(), "k_for_score": ks.grad.double().cpu()}
    loss_k, g_k = run()                                                       # the kernels
    with monkeypatch.context() as m:
        m.setattr(ops, "kd_score_loss", _yard_term)                           # fp32 torch, scores not rounded: the yardstick
        loss_y, g_y = run()
    with monkeypatch.context() as m:
        m.setattr(ops, "kd_score_loss", _RefTerm.apply)                       # fp64 closed forms: the reference
        loss_r, g_r = run()
    results = [_check("dense chunk=2 loss", loss_k, loss_y, loss_r)]
    for nm in g_k:
        results.append(_check(f"dense chunk=2 d {nm}", g_k[nm], g_y[nm], g_r[nm]))
    assert all(ok for ok, _ in results), [info for ok, info in results if not ok]
    assert g_r["k_for_score"].abs().max().item() > 0


def test_sparse_mode_gains_the_term(layers_and_inputs, monkeypatch):
    _layers, _x, _mask, scores_truth, context_truth = layers_and_inputs
    seen = {"score": [], "est": []}
    real, real_est = ops.kd_score_loss, ops.kd_estimator_loss

    def spy(q, k, truth):
        seen["score"].append((q, k, truth))
        return real(q, k, truth)

    def spy_est(est, truth):
        seen["est"].append(est)
        return real_est(est, truth)
    with monkeypatch.context() as m:
        m.setattr(ops, "kd_score_loss", spy)
        m.setattr(ops, "kd_estimator_loss", spy_est)
        off, _qs, _ks = _run(layers_and_inputs, benchmarking=True)
        assert seen["score"] == [] and isinstance(off.loss, int) and off.loss == 0       # switch off: never called
        est_only, qs_a, ks_a = _run(layers_and_inputs, benchmarking=True, est=True)
        assert seen["score"] == [] and len(seen["est"]) == 1
        est_only.loss.backward()
        on, qs, ks = _run(layers_and_inputs, benchmarking=True, score=True)
        assert len(seen["score"]) == 1 and seen["score"][0][0] is qs and seen["score"][0][1] is ks  # the layer's own tensors
        assert seen["score"][0][2].shape == scores_truth.shape
        both, qs_b, ks_b = _run(layers_and_inputs, benchmarking=True, score=True, est=True)
        assert len(seen["score"]) == 2 and len(seen["est"]) == 2
    with torch.no_grad():
        term = real(qs.detach(), ks.detach(), scores_truth.to(BF))
        ctx = F.mse_loss(context_truth.to(on.context_layer.dtype), on.context_layer.detach())
    assert torch.is_tensor(on.loss) and on.loss.requires_grad and on.loss.dim() == 0
    # switch alone: the term and the context term, two fp32 additions
    assert abs(on.loss.item() - (term.item() + ctx.item())) <= 2.0 ** -22 * max(1.0, abs(on.loss.item()))
    # both switches: what the estimator switch alone gives, plus the term
    assert abs(both.loss.item() - (est_only.loss.item() + term.item())) <= 2.0 ** -22 * max(1.0, abs(both.loss.item()))
    assert math.isfinite(both.loss.item()) and both.loss.item() != 0 and term.item() > 0 and est_only.loss.item() > ctx.item() > 0
    both.loss.backward()
    g_a = ks_a.grad if ks_a.grad is not None else torch.zeros_like(ks_a)
    assert ks_b.grad is not None and torch.isfinite(ks_b.grad).all() and not torch.equal(ks_b.grad, g_a)
    assert qs_b.grad is not None and torch.isfinite(qs_b.grad).all()
    assert torch.equal(on.context_layer, off.context_layer)                   # the switch does not touch the attention itself


@pytest.mark.parametrize("what", ["padded", "fp32"])
def test_fallbacks_change_nothing(layers_and_inputs, monkeypatch, what):
    _layers, _x, causal, _st, _ct = layers_and_inputs
    kw = {}
    if what == "padded":
        padded = causal.clone()
        padded[:, :, T_ - 8:, :] = torch.finfo(torch.float16).min / 2          # the last 8 query rows are padding
        kw = dict(mask=padded)
    else:
        kw = dict(dtype=F32)
    calls = []
    real = ops.kd_score_loss
    with monkeypatch.context() as m:
        m.setattr(ops, "kd_score_loss", lambda *a: calls.append(a) or real(*a))
        off, _q0, _k0 = _run(layers_and_inputs, chunk=2, score=False, **kw)
        on, _q1, _k1 = _run(layers_and_inputs, chunk=2, score=True, **kw)
    assert calls == []
    assert torch.equal(on.loss, off.loss) and torch.equal(on.context_layer, off.context_layer)
    assert torch.isfinite(off.loss)
