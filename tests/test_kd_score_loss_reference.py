"""The student-score distillation loss without a T x T tensor: the closed forms behind `ops.kd_score_loss`
(include/sea_hip_train.h t3 / t4, csrc/sea_kd_score_loss.hip), held to the module's own torch expression.  No GPU.

`KdScoreReference` (CPU, fp64) evaluates the per-row values, the loss and the gradients with respect to q and k from the forms
the header states.  It is held here to fp64 `torch.autograd` through `_kl_and_mse(q @ k^T, truth, mask)`, so that the GPU test's
reference (tests/test_gpu_kd_score_loss.py imports this class and the yardstick below) does not rest on the comments of the
file under test.  Also here: the comparison the GPU test makes can fail (two witnesses: a row that loses its diagonal key, and
the padded k-step of head size 80 forgotten).  The C entries themselves: tests/test_kd_abi.py."""
import inspect

import pytest
import torch
import torch.nn.functional as F

from sea_attention_amd.perlin_attention import PerlinAttention, ops
from sea_attention_amd.perlin_attention.attention import _kl_and_mse
from test_kd_loss_reference import FP_MIN16, FP_MIN32, bar_of, causal_rows_mask

SHAPES = [(1, 2, 45, 64), (2, 3, 100, 80), (1, 1, 1, 64), (1, 2, 130, 128)]          # (N, H, T, D)


class KdScoreReference:
    """fp64 closed forms of include/sea_hip_train.h t3 / t4.  q, k (N,H,T,D), truth (N,H,T,T) (whatever it holds at s > t is
    never used), g the upstream gradient of the loss.  Per row t over the keys s <= t, with S = q k^T:
        p = softmax(S),  tgt = softmax(x)
        row_kl = sum tgt (log tgt - log p)   (tgt == 0 adds 0);   row_mse = sum (p - tgt)^2;   row_q = sum p (p - tgt)
        row_stats = {max S, log sum exp(S - max), max x, log sum exp(x - max)}
        loss = 0.1 sum(row_kl) / R + sum(row_mse) / (R T),  R = N H T
        dS = g (0.1 / R (p - tgt) + 2 / (R T) (p (p - tgt) - p row_q));   d_q = dS k;   d_k = dS^T q
    `alive` (T,T) bool replaces the causal key set s <= t, `scores` replaces q k^T (the witnesses use them)."""

    def __init__(self, q, k, truth, g=1.0, alive=None, scores=None):
        q, k, truth = q.double(), k.double(), truth.double()
        N, H, T, _D = q.shape
        assert k.shape == q.shape and truth.shape == (N, H, T, T)
        alive = torch.ones((T, T), dtype=torch.bool).tril_() if alive is None else alive
        ninf = torch.tensor(float("-inf"), dtype=torch.float64)
        zero = torch.zeros((), dtype=torch.float64)
        S = torch.where(alive, q @ k.transpose(-1, -2) if scores is None else scores.double(), ninf)
        x = torch.where(alive, truth, ninf)
        m_s, m_x = S.amax(-1, keepdim=True), x.amax(-1, keepdim=True)
        l_s = torch.log(torch.exp(S - m_s).sum(-1, keepdim=True))
        l_x = torch.log(torch.exp(x - m_x).sum(-1, keepdim=True))
        logp, logt = S - m_s - l_s, x - m_x - l_x
        self.p, self.tgt = torch.exp(logp), torch.exp(logt)
        self.row_stats = torch.cat([m_s, l_s, m_x, l_x], -1)
        diff = self.p - self.tgt
        self.row_kl = torch.where(self.tgt > 0, self.tgt * (torch.where(alive, logt, zero) - torch.where(alive, logp, zero)), zero).sum(-1)
        self.row_mse = diff.square().sum(-1)
        self.row_q = (self.p * diff).sum(-1)
        R = N * H * T
        self.loss = 0.1 * self.row_kl.sum() / R + self.row_mse.sum() / (R * T)
        self.d_s = g * (0.1 / R * diff + 2.0 / (R * T) * (self.p * diff - self.p * self.row_q.unsqueeze(-1)))
        self.d_q = self.d_s @ k
        self.d_k = self.d_s.transpose(-1, -2) @ q


def torch_score_rows(q, k, truth, fp_min=FP_MIN16):
    """The fp32 yardstick: q k^T in fp32 and NOT rounded to 16 bits (the kernels' semantics), then the body of `_kl_and_mse` per
    row (`reduction='none'`): (row_kl, row_mse, row_q, row_stats, loss).  Differentiable with respect to q and k; leaves of a
    16-bit dtype get their gradients in that dtype, as the kernels write theirs."""
    N, H, T, _D = q.shape
    dead = (causal_rows_mask(torch.arange(T), T, N, fp_min) < -1).to(q.device)
    scores = (q.float() @ k.float().transpose(-1, -2)).masked_fill(dead, fp_min)
    x = truth.masked_fill(dead, fp_min).float()
    logp = F.log_softmax(scores, dim=-1)
    tgt = F.softmax(x, dim=-1)
    p = F.softmax(scores, dim=-1)
    row_kl = F.kl_div(logp, tgt, reduction='none').sum(-1)
    row_mse = F.mse_loss(p, tgt, reduction='none').sum(-1)
    with torch.no_grad():
        row_q = (p * (p - tgt)).sum(-1)
        m_s, m_x = scores.amax(-1, keepdim=True), x.amax(-1, keepdim=True)
        row_stats = torch.cat([m_s, torch.log(torch.exp(scores - m_s).sum(-1, keepdim=True)),
                               m_x, torch.log(torch.exp(x - m_x).sum(-1, keepdim=True))], -1)
    R = N * H * T
    loss = 0.1 * row_kl.sum() / R + row_mse.sum() / (R * T)
    return row_kl, row_mse, row_q, row_stats, loss


def row_bars(yardstick, reference):
    """`bar_of` per row (over the last dimension) for d_q / d_k, whose size falls with the row length: 4 times the yardstick's
    largest error in that row, at least 2^-22 of the tensor's largest magnitude."""
    per_row = 4.0 * (yardstick.double() - reference).abs().amax(-1)
    return per_row.clamp_min(2.0 ** -22 * reference.abs().max().item())


def _inputs(N, H, T, D, seed=0, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    q = (torch.randn((N, H, T, D), generator=g, dtype=torch.float64) * 0.6).to(dtype)
    k = (torch.randn((N, H, T, D), generator=g, dtype=torch.float64) * 0.6).to(dtype)
    truth = (torch.randn((N, H, T, T), generator=g, dtype=torch.float64) * 3.0).to(dtype)
    return q, k, truth


@pytest.mark.parametrize("N,H,T,D", SHAPES)
def test_closed_forms_equal_fp64_autograd_through_the_module_expression(N, H, T, D, monkeypatch):
    q, k, truth = _inputs(N, H, T, D)
    ref = KdScoreReference(q, k, truth)
    ql, kl = q.clone().requires_grad_(True), k.clone().requires_grad_(True)
    mask = causal_rows_mask(torch.arange(T), T, N, FP_MIN32)
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "float", lambda self: self.double())                     # `_kl_and_mse` says .float(): run it in fp64
        loss = _kl_and_mse(ql @ kl.transpose(-1, -2), truth, mask, FP_MIN32)
    assert loss.dtype == torch.float64
    loss.backward()
    assert abs(ref.loss.item() - loss.item()) <= 1e-12 * abs(loss.item()), (ref.loss.item(), loss.item())
    assert (ref.d_q - ql.grad).abs().max().item() <= 1e-14 and (ref.d_k - kl.grad).abs().max().item() <= 1e-14
    assert torch.all(ref.d_s.masked_select(torch.ones((T, T), dtype=torch.bool).triu_(1)) == 0)
    if T == 1:                                                                           # one key: p = tgt = 1
        assert ref.loss.item() == 0 and loss.item() == 0
        assert torch.all(ref.d_q == 0) and torch.all(ref.d_k == 0) and torch.all(ql.grad == 0) and torch.all(kl.grad == 0)
    else:
        assert ref.d_q.abs().max().item() > 1e-5 and ref.d_k.abs().max().item() > 1e-5
    # the upstream gradient scales both, and the per-row yardstick adds up to the same loss
    ref3 = KdScoreReference(q, k, truth, g=3.0)
    assert torch.equal(ref3.d_q, (3.0 * ref.d_s) @ k) and ref3.loss == ref.loss
    row_kl, row_mse, row_q, row_stats, loss_rows = torch_score_rows(q, k, truth, FP_MIN32)
    assert row_kl.dtype == torch.float32                                                 # the yardstick computes in fp32
    assert (ref.row_kl - row_kl).abs().max().item() <= 1e-4 and (ref.row_mse - row_mse).abs().max().item() <= 1e-5
    assert (ref.row_stats - row_stats).abs().max().item() <= 1e-4 and (ref.row_q - row_q).abs().max().item() <= 1e-5
    assert abs(loss_rows.item() - loss.item()) <= 1e-5 * max(abs(loss.item()), 1e-30) or T == 1


@pytest.mark.parametrize("shape,dtype", [((1, 2, 300, 80), torch.bfloat16), ((2, 3, 100, 64), torch.float16)])
def test_the_comparison_can_fail(shape, dtype):
    """(a) A row t >= 1 that loses its diagonal key misses row_kl and row_mse by more than 10 bars in at least 90 % of the rows
    whose diagonal key carries tgt >= 1e-3.  (b) At D = 80, columns 64 .. 79 dropped (the zero-padded k-step forgotten) miss
    both by more than 10 bars in every row t >= 8."""
    N, H, T, D = shape
    q, k, truth = _inputs(N, H, T, D, seed=3, dtype=dtype)
    ref = KdScoreReference(q, k, truth)
    y_kl, y_mse, _q, _st, _loss = torch_score_rows(q, k, truth)
    bars = {"row_kl": bar_of(y_kl, ref.row_kl), "row_mse": bar_of(y_mse, ref.row_mse)}
    tril = torch.ones((T, T), dtype=torch.bool).tril_()
    no_diag = tril & ~torch.eye(T, dtype=torch.bool)
    no_diag[0, 0] = True
    wrong = KdScoreReference(q, k, truth, alive=no_diag)
    rows = ref.tgt.diagonal(dim1=-2, dim2=-1) >= 1e-3
    rows[..., 0] = False
    assert rows.sum().item() > 100
    for nm in bars:
        moved = (getattr(wrong, nm) - getattr(ref, nm)).abs()
        frac = (moved[rows] > 10 * bars[nm]).double().mean().item()
        print(f"[kd-score-witness] {shape} {nm} no diagonal: {frac:.3f} of {int(rows.sum())} rows, bar {bars[nm]:.3e}")
        assert frac >= 0.9, (nm, frac, bars[nm])
    if D == 80:
        short = KdScoreReference(q, k, truth, scores=q.double()[..., :64] @ k.double()[..., :64].transpose(-1, -2))
        for nm in bars:
            moved = (getattr(short, nm) - getattr(ref, nm)).abs()[..., 8:]
            frac = (moved > 10 * bars[nm]).double().mean().item()
            print(f"[kd-score-witness] {shape} {nm} columns 64 .. 79 dropped: {frac:.3f} of the rows t >= 8")
            assert frac == 1.0, (nm, frac, bars[nm], moved.min().item())


def test_ops_are_exported_and_refuse_what_the_kernels_do_not_take():
    for name in ("kd_score_loss", "kd_score_loss_supported", "kd_score_loss_parts"):
        assert hasattr(ops, name)
    q, truth = torch.zeros(1, 2, 16, 64, dtype=torch.bfloat16), torch.zeros(1, 2, 16, 16)
    assert not ops.kd_score_loss_supported(q, q, truth)                        # CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kd_score_loss(q, q, truth)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kd_score_loss_parts(q, q, truth)
    src = inspect.getsource(PerlinAttention.__init__)
    assert "self.fused_kd_score_loss = False" in src and "self.fused_kd_loss = False" in src
