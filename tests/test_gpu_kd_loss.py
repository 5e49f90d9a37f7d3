"""-m gpu: `ops.kd_estimator_loss` (csrc/sea_kd_loss.hip) against the fp64 closed forms of tests/test_kd_loss_reference.py.

Kernel tier.  The reference is `KdReference` (fp64, held to fp64 autograd through the module's expression by the CPU suite) on
the same rounded inputs; the yardstick is the module's torch expression in fp32 on the CPU (`torch_rows`, per row, and its
autograd with the leaf in est's dtype -- the kernel writes d_est in est's dtype as well).  Per case and quantity the kernel's
largest error may be 4 times the yardstick's, at least 2^-22 of the quantity's largest magnitude (`bar_of`): the bar never
comes from the kernel's own output.  Inputs are strided views with NaN around every row and in every s > t position of the
teacher's scores.  Shapes: the smallest that reach each way the kernel can go wrong -- T no multiple of 64 or of a 16-byte
chunk, empty pixels (t + 1 < T_M), N, H > 1, T_M no power of two, more than one vector per lane.  The kernel keeps every row it
accepts (T <= 16384) in LDS, so it has no on-chip boundary; the one other path is the launch that asks for more than 48 KB of
LDS, with fp32 scores from T = 10909 on (16-bit rows stay below it), and that is the last case (rows sampled: its reference is
T wide per row).

Module tier.  `PerlinAttention.fused_kd_loss` in dense mode (head-chunked) against the torch form, and in sparse mode, where it
is what makes the loss non-zero.  The layer has no fp64 mode (its Performer runs in fp32), so the fp64 run of the dense check is
the layer with the estimator term -- the only thing the switch touches -- replaced by `KdReference`.

[kd-ref] lines print max err / bar per case; the MI355X values are in DESIGN.md."""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from test_kd_loss_reference import FP_MIN16, FP_MIN32, KdReference, bar_of, pixel_rows, torch_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF = torch.float32, torch.float16, torch.bfloat16
CASES = [((1, 2, 45, 32), F32, F32), ((1, 2, 45, 32), BF, F16), ((1, 2, 45, 32), F16, BF),
         ((2, 3, 100, 64), BF, BF), ((2, 3, 100, 64), F32, BF),
         ((1, 2, 300, 96), F16, F16), ((1, 2, 300, 96), BF, F32),
         ((1, 1, 1100, 256), F32, F16), ((1, 1, 1100, 256), F16, F32), ((1, 1, 1100, 256), BF, BF)]
T_BIG_LDS = 10909                                   # fp32 scores: the first T whose launch opts in to more than 48 KB of LDS


def _id(case):
    (N, H, T, T_M), ed, xd = case
    return f"{N}x{H}x{T}x{T_M}-{str(ed)[6:]}-{str(xd)[6:]}"


def _poisoned(values, keep=None):
    """`values` (N,H,T,W) as a strided DEVICE view with 16-byte-aligned rows inside a NaN buffer (a NaN row before and after,
    NaN columns left and right); `keep` (T,W) bool: NaN elsewhere inside the view too."""
    N, H, T, W = values.shape
    buf = torch.full((N, H, T + 2, (W + 7) // 8 * 8 + 16), float("nan"), dtype=values.dtype, device=DEV)
    view = buf[:, :, 1:T + 1, 8:8 + W]
    v = values.to(DEV)
    view.copy_(v if keep is None else torch.where(keep.to(DEV), v, torch.full_like(v, float("nan"))))
    assert view.data_ptr() % 16 == 0 and not view.is_contiguous()
    return view


@functools.lru_cache(maxsize=None)
def _case(idx):
    """Inputs (rounded to their dtypes), the fp64 reference and the fp32 yardstick of CASES[idx]; computed once, never changed."""
    (N, H, T, T_M), ed, xd = CASES[idx]
    g = torch.Generator().manual_seed(100 + idx)
    est = (torch.randn((N, H, T, T_M), generator=g) * 2.0).to(ed)
    truth = (torch.randn((N, H, T, T), generator=g) * 3.0).to(xd)
    ref = KdReference(est, truth)
    fp_min = FP_MIN32 if ed == xd == F32 else FP_MIN16                         # as the layer picks it
    leaf = est.clone().requires_grad_(True)
    row_kl, row_mse, pix_tgt, loss = torch_rows(leaf, truth, fp_min=fp_min)
    loss.backward()
    yard = dict(row_kl=row_kl.detach(), row_mse=row_mse.detach(), pix_tgt=pix_tgt, d_est=leaf.grad)
    return est, truth, ref, yard


def _check(tag, got, yard, ref):
    bar = bar_of(yard, ref)
    err = (got.double().cpu() - ref).abs().max().item()
    print(f"[kd-ref] {tag}: max err {err:.3e} / bar {bar:.3e} = {err / bar:.3f}")
    return err <= bar, (tag, err, bar)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_kernel_against_fp64_reference(idx):
    (N, H, T, T_M), ed, xd = CASES[idx]
    est_c, truth_c, ref, yard = _case(idx)
    alive = torch.arange(T).view(1, T) <= torch.arange(T).view(T, 1)
    truth = _poisoned(truth_c, keep=alive)
    est = _poisoned(est_c).detach().requires_grad_(True)
    assert ops.kd_estimator_loss_supported(est, truth)
    runs = []
    for _ in range(2):
        est.grad = None
        parts = ops.kd_estimator_loss_parts(est.detach(), truth)
        loss = ops.kd_estimator_loss(est, truth)
        assert loss.dim() == 0 and loss.dtype == F32 and loss.requires_grad
        loss.backward()
        assert est.grad.dtype == ed
        runs.append([*parts, loss.detach().clone(), est.grad.clone()])
    torch.cuda.synchronize()
    names = ["row_kl", "row_mse", "pix_tgt", "row_stats", "loss", "d_est"]
    for nm, a, b in zip(names, *runs):
        assert torch.isfinite(a).all(), nm                                     # the NaN poison reached nothing
        assert torch.equal(a, b), f"{nm}: two launches differ"
    row_kl, row_mse, pix_tgt, row_stats, loss, d_est = (t.cpu() for t in runs[0])
    assert row_kl.shape == (N, H, T) and pix_tgt.shape == (N, H, T, T_M) and row_stats.shape == (N, H, T, 2)
    assert torch.all(pix_tgt[..., ~ref.held] == 0) and torch.all(d_est[..., ~ref.held] == 0)     # empty pixels: exactly 0
    assert (~ref.held).any()                                                   # (rows with t + 1 < T_M always have some)
    results = [_check(f"{_id(CASES[idx])} {nm}", got, yard[nm], want) for nm, got, want in
               (("row_kl", row_kl, ref.row_kl), ("row_mse", row_mse, ref.row_mse), ("pix_tgt", pix_tgt, ref.pix_tgt),
                ("d_est", d_est, ref.d_est))]
    # the loss is 0.1 mean(row_kl) + mean(row_mse) / T: it may miss by the rows' bars weighted the same way, plus the fp32
    # reduction of R values (a tree: log2 R + 4 roundings of partial sums no larger than the sum of magnitudes)
    R = N * H * T
    bar_loss = (0.1 * bar_of(yard["row_kl"], ref.row_kl) + bar_of(yard["row_mse"], ref.row_mse) / T
                + 2.0 ** -24 * (math.log2(R) + 4) * (0.1 * ref.row_kl.abs().mean().item() + ref.row_mse.abs().mean().item() / T))
    err_loss = abs(loss.double().item() - ref.loss.item())
    print(f"[kd-ref] {_id(CASES[idx])} loss: err {err_loss:.3e} / bar {bar_loss:.3e} = {err_loss / bar_loss:.3f}")
    results.append((err_loss <= bar_loss, ("loss", err_loss, bar_loss)))
    assert all(ok for ok, _ in results), [info for ok, info in results if not ok]


@pytest.mark.parametrize("N,H,T,T_M,xd", [(1, 2, 45, 32, F32), (1, 2, 300, 96, F32), (2, 3, 100, 64, BF), (1, 1, 1100, 256, F16)])
def test_uniform_truth_gives_the_key_counts_exactly(N, H, T, T_M, xd):
    """x = 0: tgt_s = 1 / (t + 1), so round(pix_tgt (t + 1)) is c_b -- the kernel's pixel boundaries against the torch formula's,
    every row and pixel."""
    g = torch.Generator().manual_seed(7)
    alive = torch.arange(T).view(1, T) <= torch.arange(T).view(T, 1)
    truth = _poisoned(torch.zeros((N, H, T, T), dtype=xd), keep=alive)
    est = _poisoned(torch.randn((N, H, T, T_M), generator=g))
    _kl, _mse, pix_tgt, _st = ops.kd_estimator_loss_parts(est, truth)
    pix = pixel_rows(torch.arange(T), T, T_M)
    counts = torch.zeros((T, T_M + 1)).scatter_add_(1, torch.where(alive, pix, torch.full_like(pix, T_M)), torch.ones((T, T)))[:, :T_M]
    got = torch.round(pix_tgt.cpu() * torch.arange(1, T + 1, dtype=F32).view(1, 1, T, 1))
    assert torch.equal(got, counts.view(1, 1, T, T_M).expand(N, H, T, T_M))
    assert torch.all(pix_tgt.cpu()[..., counts == 0] == 0)


def test_rows_past_the_default_lds_limit():
    """T = 10909, N = H = 1, fp32 scores: the first T at which the launch asks for more than 48 KB of LDS (and a T that is no
    multiple of a 16-byte chunk: the row tail goes element by element).  Every row is computed; sampled rows are compared."""
    T, T_M = T_BIG_LDS, 64
    g = torch.Generator(device=DEV).manual_seed(5)
    buf = torch.randn((1, 1, T + 2, (T + 7) // 8 * 8 + 16), generator=g, device=DEV) * 3.0
    truth = buf[:, :, 1:T + 1, 8:8 + T]
    clean = truth.clone()
    truth.masked_fill_(torch.ones((T, T), dtype=torch.bool, device=DEV).triu_(1), float("nan"))
    buf[:, :, 0] = float("nan"); buf[:, :, T + 1] = float("nan"); buf[..., :8] = float("nan"); buf[..., 8 + T:] = float("nan")
    est_c = (torch.randn((1, 1, T, T_M), generator=torch.Generator().manual_seed(6)) * 2.0).to(BF)
    est = _poisoned(est_c).detach().requires_grad_(True)
    row_kl, row_mse, pix_tgt, _st = ops.kd_estimator_loss_parts(est.detach(), truth)
    loss = ops.kd_estimator_loss(est, truth)
    loss.backward()
    for t in (row_kl, row_mse, pix_tgt, loss, est.grad):
        assert torch.isfinite(t).all()
    rows = torch.tensor([0, 1, 2, 31, 32, 62, 63, 64, 65, 500, 4095, 4096, 8191, T - 3, T - 2, T - 1])
    e_r, x_r = est_c[:, :, rows], clean[:, :, rows.to(DEV)].cpu()
    ref = KdReference(e_r, x_r, t_index=rows)
    leaf = e_r.clone().requires_grad_(True)
    y_kl, y_mse, y_g, y_loss = torch_rows(leaf, x_r, t_index=rows, fp_min=FP_MIN16)
    y_loss.backward()
    results = [_check(f"T={T} {nm}", got[:, :, rows.to(got.device)], yd, want) for nm, got, yd, want in
               (("row_kl", row_kl, y_kl.detach(), ref.row_kl), ("row_mse", row_mse, y_mse.detach(), ref.row_mse),
                ("pix_tgt", pix_tgt, y_g, ref.pix_tgt), ("d_est", est.grad, leaf.grad, ref.d_est))]
    assert all(ok for ok, _ in results), [info for ok, info in results if not ok]
    assert torch.all(pix_tgt[:, :, rows.to(DEV)].cpu()[..., ~ref.held] == 0)


# ---- module tier -------------------------------------------------------------------------------------------------------
class Cfg:
    def __init__(self, hidden, heads, max_pos):
        self.hidden_size, self.num_attention_heads, self.max_position_embeddings = hidden, heads, max_pos


H_, D_, T_, TM_, K_ = 4, 64, 96, 32, 8


@pytest.fixture(scope="module")
def layer_and_inputs():
    S.seed(42)
    pc = PerlinAttentionConfig(k=K_, attention_predictor_length=TM_, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix')
    layer = PerlinSelfAttention(Cfg(H_ * D_, H_, T_), pc).to(DEV).eval()       # eval(): the torch form draws no rank jitter
    S.seed(1)
    x = torch.randn((1, H_, T_, D_), device=DEV)
    fp_min = torch.finfo(torch.float32).min / 2
    mask = ((torch.arange(T_, device=DEV).view(1, T_) > torch.arange(T_, device=DEV).view(T_, 1)) * fp_min).view(1, 1, T_, T_)
    scores_truth = torch.randn((1, H_, T_, T_), device=DEV) * 2.0
    context_truth = torch.randn((1, T_, H_ * D_), device=DEV)
    return layer, x, mask, scores_truth, context_truth


def _run(layer, inputs, benchmarking, fused, chunk=None):
    _layer, x, mask, scores_truth, context_truth = inputs
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = benchmarking
    layer.attention.fused_kd_loss = fused
    layer.attention.dense_head_chunk = chunk
    layer.zero_grad()
    try:
        out = layer(None, None, None, query_layer=x * D_ ** -0.5, key_layer=x.clone(), value_layer=x.clone(), attention_mask=mask,
                    attention_scores_truth=scores_truth, context_layer_truth=context_truth)
    finally:
        layer.attention.fused_kd_loss = False
        layer.attention.dense_head_chunk = None
    return out


class _RefTerm(torch.autograd.Function):
    """The estimator term in fp64 on the CPU (`KdReference`), standing in for `ops.kd_estimator_loss` in the reference run."""

    @staticmethod
    def forward(ctx, est, truth):
        ref = KdReference(est.detach().cpu(), truth.detach().cpu())
        ctx.d_est, ctx.like = ref.d_est, est
        return ref.loss.to(torch.float32).to(est.device)

    @staticmethod
    def backward(ctx, g):
        return (ctx.d_est * g.double().cpu()).to(ctx.like.dtype).to(ctx.like.device), None


def test_dense_mode_fused_term_against_the_torch_form(layer_and_inputs, monkeypatch):
    layer = layer_and_inputs[0]
    att = layer.attention
    weights = {"enc": att.attention_predictor_enc[0].weight, "dec_scaler": att.attention_predictor_dec_scaler[0].weight}

    def run(fused):
        out = _run(layer, layer_and_inputs, False, fused, chunk=2)
        out.loss.backward()
        return out.loss.detach().double().cpu(), {k: w.grad.detach().double().cpu().clone() for k, w in weights.items()}
    loss_y, g_y = run(False)                                                  # the torch form, fp32: the yardstick
    loss_k, g_k = run(True)                                                   # the kernels
    with monkeypatch.context() as m:
        m.setattr(ops, "kd_estimator_loss", _RefTerm.apply)                   # fp64 closed forms: the reference
        loss_r, g_r = run(True)
    results = [_check("dense chunk=2 loss", loss_k, loss_y, loss_r)]
    for k in weights:
        results.append(_check(f"dense chunk=2 d {k}.weight", g_k[k], g_y[k], g_r[k]))
    assert all(ok for ok, _ in results), [info for ok, info in results if not ok]
    assert g_r["enc"].abs().max().item() > 0


def test_sparse_mode_loss_is_zero_without_the_switch(layer_and_inputs):
    out = _run(layer_and_inputs[0], layer_and_inputs, True, False)
    assert isinstance(out.loss, int) and out.loss == 0


def test_sparse_mode_trains_the_predictor_with_the_switch(layer_and_inputs, monkeypatch):
    layer, _x, _mask, scores_truth, context_truth = layer_and_inputs
    off = _run(layer, layer_and_inputs, True, False)
    seen = []
    real = ops.kd_estimator_loss

    def spy(est, truth):
        seen.append((est.detach(), truth))
        return real(est, truth)
    with monkeypatch.context() as m:
        m.setattr(ops, "kd_estimator_loss", spy)
        out = _run(layer, layer_and_inputs, True, True)
    assert len(seen) == 1 and seen[0][0].shape == (1, H_, T_, TM_) and seen[0][1] is scores_truth
    assert torch.is_tensor(out.loss) and out.loss.requires_grad and out.loss.dim() == 0
    want = real(*seen[0]) + F.mse_loss(context_truth, out.context_layer.detach())
    # the same two fp32 values added once: at most the last bit apart
    assert abs(out.loss.item() - want.item()) <= 2.0 ** -23 * abs(want.item()), (out.loss.item(), want.item())
    assert out.loss.item() > 0
    out.loss.backward()
    g = layer.attention.attention_predictor_enc[0].weight.grad
    assert g is not None and torch.isfinite(g).all() and g.abs().max().item() > 0
    assert torch.equal(out.context_layer, off.context_layer)                  # the switch does not touch the attention itself
