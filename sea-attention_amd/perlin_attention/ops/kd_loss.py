"""Distillation loss of the estimator on the HIP kernels (include/sea_hip_train.h, csrc/sea_kd_loss.hip).

`kd_estimator_loss(est_scores, truth_scores)` is the estimator term of `PerlinAttention.forward` -- `_kl_and_mse` over
`resize_from_m_to_t(est_scores)` -- for a causal, unpadded batch, without the (N,H,T,T) resize or any fp32 copy of the
teacher's scores: the forward reads the causal half of `truth_scores` once, the backward is T_M wide.

`truth_scores` may be an `ops.TeacherScores(q_t, k_t)` instead of the tensor: the forward then recomputes the teacher's product
tile by tile on the matrix cores (t5, csrc/sea_kd_score_loss.hip's tile body) and nothing T x T exists anywhere; the backward is
the same launch either way."""
import torch

from ... import _lib
from .flat_csr import _p
from .teacher_scores import TeacherScores, qk_supported

KD_MAX_T_M, KD_MAX_T = 512, 16384
KD_QK_HEAD_SIZES = (64, 80, 128)
_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _rows_aligned(t):
    vec = 4 if t.dtype == torch.float32 else 8
    return (t.stride(-1) == 1 and t.stride(2) >= t.shape[-1] and all(s >= 0 and s % vec == 0 for s in t.stride()[:3])
            and t.data_ptr() % 16 == 0)


def kd_estimator_loss_supported(est, truth) -> bool:
    """What the kernels take: device tensors est (N,H,T,T_M) and truth (N,H,T,T) of fp32 / fp16 / bf16 (independently) with an
    innermost stride of 1 and 16-byte-aligned rows, T_M % 4 == 0, T_M <= 512, T <= 16384.  Or truth an `ops.TeacherScores` on
    est's device: 16-bit q / k (N,H,T,D) with D in {64, 80, 128} and aligned rows."""
    if isinstance(truth, TeacherScores):
        if not (isinstance(est, torch.Tensor) and est.is_cuda and est.dim() == 4 and est.device == truth.device):
            return False
        N, H, T, T_M = est.shape
        if est.dtype not in _DTYPES or min(N, H, T, T_M) < 1 or T_M % 4 or T_M > KD_MAX_T_M:
            return False
        if N * H * ((T + 63) // 64) >= 1 << 31:
            return False
        return _rows_aligned(est) and qk_supported(truth, N, H, T, KD_QK_HEAD_SIZES, KD_MAX_T)
    if not (isinstance(est, torch.Tensor) and isinstance(truth, torch.Tensor) and est.is_cuda and truth.is_cuda
            and est.device == truth.device and est.dim() == 4 and truth.dim() == 4):
        return False
    N, H, T, T_M = est.shape
    if tuple(truth.shape) != (N, H, T, T) or min(N, H, T, T_M) < 1:
        return False
    if est.dtype not in _DTYPES or truth.dtype not in _DTYPES:
        return False
    if T_M % 4 or T_M > KD_MAX_T_M or T > KD_MAX_T or N * H * ((T + 1) // 2) >= 1 << 31:
        return False
    return _rows_aligned(est) and _rows_aligned(truth)


@_lib.device_guarded
def kd_estimator_loss_parts(est, truth):
    """The forward launch alone: (row_kl (N,H,T), row_mse (N,H,T), pix_tgt (N,H,T,T_M), row_stats (N,H,T,2)), all fp32."""
    if isinstance(truth, TeacherScores):
        _lib.require_gpu(est, truth.q, truth.k)
        if not kd_estimator_loss_supported(est, truth):
            raise RuntimeError(f"kd_estimator_loss: est {tuple(est.shape)} {est.dtype} strides {est.stride()} / teacher q "
                               f"{tuple(truth.q.shape)} {truth.q.dtype} strides {truth.q.stride()}, k strides {truth.k.stride()} "
                               "is outside the kernel (ops.kd_estimator_loss_supported)")
        lib = _lib.load()
        N, H, T, T_M = est.shape
        tq, tk = truth.q, truth.k
        dev = est.device
        row_kl = torch.empty((N, H, T), dtype=torch.float32, device=dev)
        row_mse = torch.empty((N, H, T), dtype=torch.float32, device=dev)
        pix_tgt = torch.empty((N, H, T, T_M), dtype=torch.float32, device=dev)
        row_stats = torch.empty((N, H, T, 2), dtype=torch.float32, device=dev)
        _lib.check(lib.sea_kd_estimator_loss_qk(_p(est), _lib.dtype_code(est.dtype), _lib.strides3(est),
                                                _p(tq), _p(tk), _lib.dtype_code(tq.dtype), _lib.strides3(tq), _lib.strides3(tk),
                                                N, H, T, T_M, tq.shape[-1], _p(row_kl), _p(row_mse), _p(pix_tgt), _p(row_stats),
                                                _lib.stream_ptr()),
                   "sea_kd_estimator_loss_qk")
        return row_kl, row_mse, pix_tgt, row_stats
    _lib.require_gpu(est, truth)
    if not kd_estimator_loss_supported(est, truth):
        raise RuntimeError(f"kd_estimator_loss: est {tuple(est.shape)} {est.dtype} strides {est.stride()} / truth "
                           f"{tuple(truth.shape)} {truth.dtype} strides {truth.stride()} is outside the kernel "
                           "(ops.kd_estimator_loss_supported)")
    lib = _lib.load()
    N, H, T, T_M = est.shape
    dev = est.device
    row_kl = torch.empty((N, H, T), dtype=torch.float32, device=dev)
    row_mse = torch.empty((N, H, T), dtype=torch.float32, device=dev)
    pix_tgt = torch.empty((N, H, T, T_M), dtype=torch.float32, device=dev)
    row_stats = torch.empty((N, H, T, 2), dtype=torch.float32, device=dev)
    _lib.check(lib.sea_kd_estimator_loss(_p(est), _lib.dtype_code(est.dtype), _lib.strides3(est),
                                         _p(truth), _lib.dtype_code(truth.dtype), _lib.strides3(truth), N, H, T, T_M,
                                         _p(row_kl), _p(row_mse), _p(pix_tgt), _p(row_stats), _lib.stream_ptr()),
               "sea_kd_estimator_loss")
    return row_kl, row_mse, pix_tgt, row_stats


class _KdEstimatorLossFn(torch.autograd.Function):
    """loss = 0.1 sum(row_kl) / R + sum(row_mse) / (R T), R = N H T.  Saved for the backward: est, the teacher's mass per pixel
    (N,H,T,T_M) and two scalars per row -- not the teacher's scores.  The gradient goes to `est` only, in est's dtype."""

    @staticmethod
    def forward(ctx, est, truth, tq=None, tk=None):
        with torch.no_grad():
            est_d, truth_d = est.detach(), (TeacherScores(tq, tk) if truth is None else truth.detach())
            row_kl, row_mse, pix_tgt, row_stats = kd_estimator_loss_parts(est_d, truth_d)
            N, H, T, _ = est.shape
            R = N * H * T
            # torch.sum of a contiguous fp32 tensor: a fixed reduction tree for a fixed shape, no atomics, no host read-back
            loss = row_kl.sum() * (0.1 / R) + row_mse.sum() * (1.0 / (R * T))
        ctx.save_for_backward(est_d, pix_tgt, row_stats)
        return loss

    @staticmethod
    @_lib.device_guarded
    def backward(ctx, grad_loss):
        est, pix_tgt, row_stats = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        lib = _lib.load()
        N, H, T, T_M = est.shape
        g = grad_loss.detach().to(torch.float32).reshape(1).contiguous()
        d_est = torch.empty((N, H, T, T_M), dtype=est.dtype, device=est.device)
        _lib.check(lib.sea_kd_estimator_loss_bwd(_p(est), _lib.dtype_code(est.dtype), _lib.strides3(est), _p(pix_tgt), _p(row_stats),
                                                 _p(g), N, H, T, T_M, _p(d_est), _lib.stream_ptr()),
                   "sea_kd_estimator_loss_bwd")
        return d_est, None, None, None


def kd_estimator_loss(est_scores, truth_scores) -> torch.Tensor:
    """0.1 KL(batchmean) + MSE between softmax over the causal keys of the T_M-wide `est_scores` (N,H,T,T_M) stretched to each
    row's keys (`resize_from_m_to_t`, no oversampling, no rank jitter) and softmax of `truth_scores` (N,H,T,T): a 0-dim fp32
    tensor, differentiable with respect to `est_scores`.  Causal and unpadded: row t sees keys 0 .. t, whatever `truth_scores`
    holds beyond them.  `truth_scores` may be an `ops.TeacherScores`: the teacher's q k^T is then recomputed tile by tile (fp32
    accumulator, not rounded to the data type) and no (N,H,T,T) tensor is read."""
    if isinstance(truth_scores, TeacherScores):
        return _KdEstimatorLossFn.apply(est_scores, None, truth_scores.q, truth_scores.k)
    return _KdEstimatorLossFn.apply(est_scores, truth_scores, None, None)
