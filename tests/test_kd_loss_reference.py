"""The estimator's distillation loss without a T x T tensor: the closed forms behind `ops.kd_estimator_loss`
(include/sea_hip_train.h, csrc/sea_kd_loss.hip), held to the module's own torch expression.  No GPU.

`KdReference` (CPU, fp64) evaluates the loss and its gradient from the per-pixel key counts c_b, the teacher's mass per pixel
G_b and per-row scalars.  It is held here to fp64 `torch.autograd` through `_kl_and_mse` over `resize_from_m_to_t(...,
oversampled=1.0)`, so that the GPU test's reference (tests/test_gpu_kd_loss.py imports this class and the yardstick below) does
not rest on the comments of the file under test.  Also here: pix is non-decreasing along every row, the comparison the GPU test
makes can fail (a witness with one key dropped per pixel).  The C entries themselves: tests/test_kd_abi.py."""
import pytest
import torch
import torch.nn.functional as F

from sea_attention_amd.perlin_attention import ops
from sea_attention_amd.perlin_attention.attention import _kl_and_mse

FP_MIN32 = torch.finfo(torch.float32).min / 2
FP_MIN16 = torch.finfo(torch.float16).min / 2
SHAPES = [(1, 2, 45, 32), (2, 3, 100, 64), (1, 1, 20, 32), (1, 2, 300, 96)]       # (N, H, T, T_M)


def pixel_rows(t_index, T, T_M):
    """pix(t, s) for the rows `t_index` and keys 0 .. T - 1: ops/resize_dense.py's formula in fp32 (rank s + 1 of t + 1 keys).
    Entries with s > t mean nothing."""
    rank = torch.arange(1, T + 1, dtype=torch.float32).view(1, T)
    length = (t_index.to(torch.float32) + 1).view(-1, 1)
    return torch.floor((rank - 0.5) / length * T_M - 1e-4).to(torch.long).clamp(0, T_M)


def causal_rows_mask(t_index, T, N, fp_min, dtype=torch.float32):
    """(N, 1, rows, T) additive mask of the rows `t_index`: 0 on keys s <= t, fp_min beyond"""
    dead = torch.arange(T).view(1, T) > t_index.view(-1, 1)
    return (dead.to(dtype) * fp_min).view(1, 1, -1, T).expand(N, 1, -1, T).contiguous()


class KdReference:
    """fp64 closed forms of include/sea_hip_train.h.  est (N,H,rows,T_M), truth (N,H,rows,T); `t_index` names the rows (default:
    all T of them), R = N H T whatever the rows.  With c_b the keys of pixel b, held = c_b > 0:
        p_b = exp(e_b - m_e) / sum_b c_b exp(e_b - m_e),  m_e = max over held pixels;   tgt = softmax over s <= t of x
        G_b = sum of tgt over the keys of b;   P_b = c_b p_b
        row_kl  = sum_s tgt_s log tgt_s - sum_b G_b log p_b          (tgt_s == 0 adds 0)
        row_mse = sum_b (c_b p_b^2 - 2 p_b G_b) + sum_s tgt_s^2
        loss = 0.1 sum(row_kl) / R + sum(row_mse) / (R T)
        d_est_b = 0.1 / R (P_b - G_b) + 2 / (R T) (p_b (P_b - G_b) - P_b Q),  Q = sum_b p_b (P_b - G_b);  0 where not held"""

    def __init__(self, est, truth, t_index=None):
        est, truth = est.double(), truth.double()
        N, H, rows, T_M = est.shape
        T = truth.shape[-1]
        t_index = torch.arange(T) if t_index is None else t_index
        assert truth.shape == (N, H, rows, T) and t_index.shape == (rows,)
        pix = pixel_rows(t_index, T, T_M)
        alive = torch.arange(T).view(1, T) <= t_index.view(-1, 1)
        self.counts = torch.zeros((rows, T_M + 1), dtype=torch.float64).scatter_add_(
            1, torch.where(alive, pix, torch.full_like(pix, T_M)), torch.ones((rows, T), dtype=torch.float64))[:, :T_M]
        assert torch.equal(self.counts.sum(-1), (t_index + 1).double())          # no key s <= t lands in the fill column
        self.held = self.counts > 0
        ninf = torch.tensor(float("-inf"), dtype=torch.float64)
        self.tgt = torch.softmax(torch.where(alive, truth, ninf), -1)
        idx = torch.where(alive, pix, torch.zeros_like(pix)).expand(N, H, rows, T)
        self.pix_tgt = torch.zeros((N, H, rows, T_M), dtype=torch.float64).scatter_add_(-1, idx, self.tgt)
        m_e = torch.where(self.held, est, ninf).amax(-1, keepdim=True)
        w = torch.where(self.held, torch.exp(torch.where(self.held, est - m_e, ninf)), torch.zeros((), dtype=torch.float64))
        log_s = torch.log((self.counts * w).sum(-1, keepdim=True))
        logp = torch.where(self.held, est - m_e - log_s, torch.zeros((), dtype=torch.float64))
        self.p = torch.where(self.held, torch.exp(logp), torch.zeros((), dtype=torch.float64))
        self.row_stats = torch.cat([m_e, log_s], -1)
        P = self.counts * self.p
        ent = torch.where(self.tgt > 0, self.tgt * torch.log(self.tgt.clamp_min(1e-300)), torch.zeros((), dtype=torch.float64)).sum(-1)
        self.row_kl = ent - (self.pix_tgt * logp).sum(-1)
        self.row_mse = (self.counts * self.p * self.p - 2 * self.p * self.pix_tgt).sum(-1) + self.tgt.square().sum(-1)
        R = N * H * T
        self.loss = 0.1 * self.row_kl.sum() / R + self.row_mse.sum() / (R * T)
        D = P - self.pix_tgt
        Q = (self.p * D).sum(-1, keepdim=True)
        self.d_est = torch.where(self.held, 0.1 / R * D + 2.0 / (R * T) * (self.p * D - P * Q), torch.zeros((), dtype=torch.float64))


def torch_rows(est, truth, t_index=None, compute=torch.float32, fp_min=FP_MIN32):
    """The module's torch expression (`resize_from_m_to_t` + the body of `_kl_and_mse`) for the rows `t_index`, evaluated in
    `compute` per row (`reduction='none'`): (row_kl, row_mse, pix_tgt, loss).  Differentiable with respect to `est`."""
    N, H, rows, T_M = est.shape
    T = truth.shape[-1]
    t_index = torch.arange(T) if t_index is None else t_index
    mask = causal_rows_mask(t_index, T, N, fp_min)
    dead = mask < -1
    resized = ops.resize_from_m_to_t(est, fp_min, mask, T, False, True, 7, 1.0)
    logp = F.log_softmax(resized.masked_fill(dead, fp_min).to(compute), dim=-1)
    tgt = F.softmax(truth.masked_fill(dead, fp_min).to(compute), dim=-1)
    row_kl = F.kl_div(logp, tgt, reduction='none').sum(-1)
    row_mse = F.mse_loss(F.softmax(resized.masked_fill(dead, fp_min).to(compute), dim=-1), tgt, reduction='none').sum(-1)
    pix = pixel_rows(t_index, T, T_M)
    alive = torch.arange(T).view(1, T) <= t_index.view(-1, 1)
    idx = torch.where(alive, pix, torch.zeros_like(pix)).expand(N, H, rows, T)
    pix_tgt = torch.zeros((N, H, rows, T_M), dtype=compute).scatter_add_(-1, idx, (tgt * alive).detach())
    R = N * H * T
    loss = 0.1 * row_kl.sum() / R + row_mse.sum() / (R * T)
    return row_kl, row_mse, pix_tgt, loss


def bar_of(yardstick, reference):
    """What the kernel may miss the fp64 reference by: 4 times what the fp32 torch expression misses it by (another summation
    order, device exp / log at up to 2 ulp against the host's 1), and at least 2^-22 of the quantity's largest magnitude."""
    return max(4.0 * (yardstick.double() - reference).abs().max().item(), 2.0 ** -22 * reference.abs().max().item())


def _inputs(N, H, T, T_M, seed=0):
    g = torch.Generator().manual_seed(seed)
    est = torch.randn((N, H, T, T_M), generator=g, dtype=torch.float64) * 2.0
    truth = torch.randn((N, H, T, T), generator=g, dtype=torch.float64) * 3.0
    return est, truth


@pytest.mark.parametrize("N,H,T,T_M", SHAPES)
def test_closed_forms_equal_fp64_autograd_through_the_module_expression(N, H, T, T_M, monkeypatch):
    est, truth = _inputs(N, H, T, T_M)
    ref = KdReference(est, truth)
    leaf = est.clone().requires_grad_(True)
    mask = causal_rows_mask(torch.arange(T), T, N, FP_MIN32)
    resized = ops.resize_from_m_to_t(leaf, FP_MIN32, mask, T, False, True, 7, 1.0)       # pixels in fp32, values in fp64
    assert resized.dtype == torch.float64
    with monkeypatch.context() as m:
        m.setattr(torch.Tensor, "float", lambda self: self.double())                     # `_kl_and_mse` says .float(): run it in fp64
        loss = _kl_and_mse(resized, truth, mask, FP_MIN32)
    assert loss.dtype == torch.float64
    loss.backward()
    assert abs(ref.loss.item() - loss.item()) <= 1e-12 * abs(loss.item()), (ref.loss.item(), loss.item())
    assert (ref.d_est - leaf.grad).abs().max().item() <= 1e-14
    assert torch.all(ref.d_est[..., ~ref.held] == 0) and torch.all(leaf.grad[..., ~ref.held] == 0)
    # the per-row values add up to the same loss through the per-row torch expression
    row_kl, row_mse, pix_tgt, loss_rows = torch_rows(est, truth, compute=torch.float64)
    assert (ref.row_kl - row_kl).abs().max().item() <= 1e-12 and (ref.row_mse - row_mse).abs().max().item() <= 1e-13
    assert (ref.pix_tgt - pix_tgt).abs().max().item() <= 1e-14
    assert abs(loss_rows.item() - loss.item()) <= 1e-12 * abs(loss.item())


@pytest.mark.parametrize("T,T_M", [(45, 32), (100, 64), (20, 32), (300, 96), (1100, 256), (4096, 256), (777, 512)])
def test_pix_is_monotone_in_every_row(T, T_M):
    pix = pixel_rows(torch.arange(T), T, T_M)
    alive = torch.arange(T).view(1, T) <= torch.arange(T).view(T, 1)
    step = pix[:, 1:] - pix[:, :-1]
    assert torch.all(step[alive[:, 1:]] >= 0)
    assert torch.all(pix[alive] < T_M) and torch.all(pix[alive] >= 0)
    # and it is the pixel the dense resize reads: an est row holding its own pixel index comes back as pix
    est = torch.arange(T_M, dtype=torch.float32).view(1, 1, 1, T_M).expand(1, 1, T, T_M)
    mask = causal_rows_mask(torch.arange(T), T, 1, FP_MIN32)
    got = ops.resize_from_m_to_t(est, -1.0, mask, T, False, True, 7, 1.0)[0, 0]
    assert torch.equal(got[alive].long(), pix[alive])


def test_dropping_one_key_per_pixel_is_seen():
    """The GPU comparison can fail: G_b without the LAST key of each pixel misses the bar by more than 10 bars in at least
    90 % of the rows whose dropped key carries tgt >= 1e-3."""
    N, H, T, T_M = 1, 2, 300, 96
    est, truth = _inputs(N, H, T, T_M, seed=3)
    est, truth = est.float(), truth.float()
    ref = KdReference(est, truth)
    _kl, _mse, yard, _loss = torch_rows(est, truth)
    bar = bar_of(yard, ref.pix_tgt)
    pix = pixel_rows(torch.arange(T), T, T_M)
    alive = torch.arange(T).view(1, T) <= torch.arange(T).view(T, 1)
    nxt = torch.cat([pix[:, 1:], torch.full((T, 1), -1, dtype=torch.long)], 1)
    nxt_alive = torch.cat([alive[:, 1:], torch.zeros((T, 1), dtype=torch.bool)], 1)
    last = alive & ((nxt != pix) | ~nxt_alive)                                 # the last key of its pixel
    dropped = ref.tgt * last
    wrong = ref.pix_tgt - torch.zeros_like(ref.pix_tgt).scatter_add_(-1, torch.where(alive, pix, torch.zeros_like(pix)).expand(N, H, T, T), dropped)
    moved = (wrong - ref.pix_tgt).abs().amax(-1)                               # per row
    rows = dropped.amax(-1) >= 1e-3
    assert rows.sum().item() > 100
    assert (moved[rows] > 10 * bar).double().mean().item() >= 0.9, (bar, moved[rows].min().item())


def test_ops_are_exported_and_refuse_what_the_kernels_do_not_take():
    for name in ("kd_estimator_loss", "kd_estimator_loss_supported", "kd_estimator_loss_parts"):
        assert hasattr(ops, name)
    est, truth = torch.zeros(1, 2, 16, 8), torch.zeros(1, 2, 16, 16)
    assert not ops.kd_estimator_loss_supported(est, truth)                    # CPU tensors
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.kd_estimator_loss(est, truth)
    from sea_attention_amd.perlin_attention import PerlinAttention
    import inspect
    assert "self.fused_kd_loss = False" in inspect.getsource(PerlinAttention.__init__)
