"""Distillation loss of the estimator on the HIP kernels (include/sea_hip_train.h, csrc/sea_kd_loss.hip).

`kd_estimator_loss(est_scores, truth_scores)` is the estimator term of `PerlinAttention.forward` -- `_kl_and_mse` over
`resize_from_m_to_t(est_scores)` -- for a causal, unpadded batch, without the (N,H,T,T) resize or any fp32 copy of the
teacher's scores: the forward reads the causal half of `truth_scores` once, the backward is T_M wide.

`truth_scores` may be an `ops.TeacherScores(q_t, k_t)` instead of the tensor: the forward then recomputes the teacher's product
tile by tile on the matrix cores (the same entry, csrc/sea_kd_score_loss.hip's tile body) and nothing T x T exists anywhere; the
backward is the same launch either way."""
import torch

from ... import _lib
from .flat_csr import _p
from .teacher_scores import TeacherScores, _DTYPES, _rows_aligned, teacher_args, teacher_supported, teacher_tensors

KD_MAX_T_M, KD_MAX_T = 512, 16384
KD_QK_HEAD_SIZES = (64, 80, 128)


def kd_estimator_loss_supported(est, truth) -> bool:
    """What the kernels take: device tensors est (N,H,T,T_M) and truth (N,H,T,T) of fp32 / fp16 / bf16 (independently) with an
    innermost stride of 1 and 16-byte-aligned rows, T_M % 4 == 0, T_M <= 512, T <= 16384.  Or truth an `ops.TeacherScores` on
    est's device: 16-bit q / k (N,H,T,D) with D in {64, 80, 128} and aligned rows."""
    if not (isinstance(est, torch.Tensor) and est.is_cuda and est.dim() == 4):
        return False
    N, H, T, T_M = est.shape
    if est.dtype not in _DTYPES or min(N, H, T, T_M) < 1 or T_M % 4 or T_M > KD_MAX_T_M:
        return False
    block_rows = 64 if isinstance(truth, TeacherScores) else 2         # per workgroup of the kernel that runs: tile or row pair
    if N * H * ((T + block_rows - 1) // block_rows) >= 1 << 31:
        return False
    return _rows_aligned(est) and teacher_supported(truth, est.device, N, H, T, KD_QK_HEAD_SIZES, KD_MAX_T)


@_lib.device_guarded
def kd_estimator_loss_parts(est, truth):
    """The forward launch alone: (row_kl (N,H,T), row_mse (N,H,T), pix_tgt (N,H,T,T_M), row_stats (N,H,T,2)), all fp32."""
    tensors, shown = teacher_tensors(truth)
    _lib.require_gpu(est, *tensors)
    if not kd_estimator_loss_supported(est, truth):
        raise RuntimeError(f"kd_estimator_loss: est {tuple(est.shape)} {est.dtype} strides {est.stride()} / {shown} "
                           "is outside the kernel (ops.kd_estimator_loss_supported)")
    lib = _lib.load()
    N, H, T, T_M = est.shape
    D = tensors[0].shape[-1] if isinstance(truth, TeacherScores) else 0
    dev = est.device
    row_kl = torch.empty((N, H, T), dtype=torch.float32, device=dev)
    row_mse = torch.empty((N, H, T), dtype=torch.float32, device=dev)
    pix_tgt = torch.empty((N, H, T, T_M), dtype=torch.float32, device=dev)
    row_stats = torch.empty((N, H, T, 2), dtype=torch.float32, device=dev)
    _lib.check(lib.sea_kd_estimator_loss(_p(est), _lib.dtype_code(est.dtype), _lib.strides3(est), *teacher_args(truth),
                                         N, H, T, T_M, D, _p(row_kl), _p(row_mse), _p(pix_tgt), _p(row_stats), _lib.stream_ptr()),
               "sea_kd_estimator_loss")
    return row_kl, row_mse, pix_tgt, row_stats


class _KdEstimatorLossFn(torch.autograd.Function):
    """loss = 0.1 sum(row_kl) / R + sum(row_mse) / (R T), R = N H T.  Saved for the backward: est, the teacher's mass per pixel
    (N,H,T,T_M) and two scalars per row -- not the teacher's scores, which come as the tensor or as an `ops.TeacherScores`.  The
    gradient goes to `est` only, in est's dtype."""

    @staticmethod
    def forward(ctx, est, truth):
        with torch.no_grad():
            est_d, truth_d = est.detach(), (truth if isinstance(truth, TeacherScores) else truth.detach())
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
            return None, None
        lib = _lib.load()
        N, H, T, T_M = est.shape
        g = grad_loss.detach().to(torch.float32).reshape(1).contiguous()
        d_est = torch.empty((N, H, T, T_M), dtype=est.dtype, device=est.device)
        _lib.check(lib.sea_kd_estimator_loss_bwd(_p(est), _lib.dtype_code(est.dtype), _lib.strides3(est), _p(pix_tgt), _p(row_stats),
                                                 _p(g), N, H, T, T_M, _p(d_est), _lib.stream_ptr()),
                   "sea_kd_estimator_loss_bwd")
        return d_est, None


def kd_estimator_loss(est_scores, truth_scores) -> torch.Tensor:
    """0.1 KL(batchmean) + MSE between softmax over the causal keys of the T_M-wide `est_scores` (N,H,T,T_M) stretched to each
    row's keys (`resize_from_m_to_t`, no oversampling, no rank jitter) and softmax of `truth_scores` (N,H,T,T): a 0-dim fp32
    tensor, differentiable with respect to `est_scores`.  Causal and unpadded: row t sees keys 0 .. t, whatever `truth_scores`
    holds beyond them.  `truth_scores` may be an `ops.TeacherScores`: the teacher's q k^T is then recomputed tile by tile (fp32
    accumulator, not rounded to the data type) and no (N,H,T,T) tensor is read."""
    return _KdEstimatorLossFn.apply(est_scores, truth_scores)
