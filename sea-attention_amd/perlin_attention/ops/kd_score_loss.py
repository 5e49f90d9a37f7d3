"""Distillation loss of the student's own scores on the HIP kernels (include/sea_hip_train.h, csrc/sea_kd_score_loss.hip).

`kd_score_loss(q, k, truth_scores)` is the student-score term of `PerlinAttention` -- `_kl_and_mse` over
`q_for_score @ k_for_score^T` -- for a causal, unpadded batch, without the (N,H,T,T) score tensor, its fp32 softmaxes or anything
autograd would save of them: the forward recomputes q k^T tile by tile on the matrix cores and reads the causal half of
`truth_scores` twice, the backward (two launches) twice more.  The scores keep their fp32 accumulator (the torch form rounds
q k^T to the data type before the softmaxes).

`truth_scores` may be an `ops.TeacherScores(q_t, k_t)` instead of the tensor: then the teacher's product is recomputed beside the
student's (the same entries, fp32 accumulator, not rounded either) and nothing T x T exists anywhere."""
import torch

from ... import _lib
from .flat_csr import _p
from .teacher_scores import TeacherScores, _rows_aligned, teacher_args, teacher_supported, teacher_tensors

KD_SCORE_HEAD_SIZES, KD_SCORE_MAX_T = (64, 80, 128), 16384
_QK_DTYPES = (torch.float16, torch.bfloat16)


def kd_score_loss_supported(q, k, truth) -> bool:
    """What the kernels take: device tensors q, k (N,H,T,D) of one 16-bit dtype and truth (N,H,T,T) of fp32 / fp16 / bf16, each
    with an innermost stride of 1 and 16-byte-aligned rows, D in {64, 80, 128}, T <= 16384.  Or truth an `ops.TeacherScores` on
    the device whose q / k have the student's shape and dtype and aligned rows."""
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.dim() == 4 for t in (q, k)):
        return False
    if not (q.device == k.device and q.shape == k.shape and q.dtype == k.dtype):
        return False
    N, H, T, D = q.shape
    if q.dtype not in _QK_DTYPES or D not in KD_SCORE_HEAD_SIZES or N * H * ((T + 63) // 64) >= 1 << 31:
        return False
    return _rows_aligned(q) and _rows_aligned(k) and teacher_supported(truth, q.device, N, H, T, (D,), KD_SCORE_MAX_T, q.dtype)


def _require(q, k, truth):
    tensors, shown = teacher_tensors(truth)
    _lib.require_gpu(q, k, *tensors)
    if not kd_score_loss_supported(q, k, truth):
        raise RuntimeError(f"kd_score_loss: q {tuple(q.shape)} {q.dtype} strides {q.stride()} / k {tuple(k.shape)} {k.dtype} "
                           f"strides {k.stride()} / {shown} is outside the kernels (ops.kd_score_loss_supported)")


@_lib.device_guarded
def kd_score_loss_parts(q, k, truth):
    """The forward launch alone: (row_kl (N,H,T), row_mse (N,H,T), row_q (N,H,T), row_stats (N,H,T,4)), all fp32;
    row_stats = {max S, log sum exp, max x, log sum exp} of the student's and the teacher's row."""
    _require(q, k, truth)
    lib = _lib.load()
    N, H, T, D = q.shape
    dev = q.device
    row_kl = torch.empty((N, H, T), dtype=torch.float32, device=dev)
    row_mse = torch.empty((N, H, T), dtype=torch.float32, device=dev)
    row_q = torch.empty((N, H, T), dtype=torch.float32, device=dev)
    row_stats = torch.empty((N, H, T, 4), dtype=torch.float32, device=dev)
    _lib.check(lib.sea_kd_score_loss(_p(q), _p(k), _lib.dtype_code(q.dtype), _lib.strides3(q), _lib.strides3(k), *teacher_args(truth),
                                     N, H, T, D, _p(row_kl), _p(row_mse), _p(row_q), _p(row_stats), _lib.stream_ptr()),
               "sea_kd_score_loss")
    return row_kl, row_mse, row_q, row_stats


class _KdScoreLossFn(torch.autograd.Function):
    """loss = 0.1 sum(row_kl) / R + sum(row_mse) / (R T), R = N H T.  Saved for the backward: q, k and the teacher as it came in
    (the score tensor, or the q / k of an `ops.TeacherScores`: references, no copies) and five scalars per row.  The gradient
    goes to q and k, in their dtype."""

    @staticmethod
    def forward(ctx, q, k, truth):
        ctx.factored = isinstance(truth, TeacherScores)
        with torch.no_grad():
            q_d, k_d = q.detach(), k.detach()
            truth_d = truth if ctx.factored else truth.detach()
            row_kl, row_mse, row_q, row_stats = kd_score_loss_parts(q_d, k_d, truth_d)
            N, H, T, _ = q.shape
            R = N * H * T
            # torch.sum of a contiguous fp32 tensor: a fixed reduction tree for a fixed shape, no atomics, no host read-back
            loss = row_kl.sum() * (0.1 / R) + row_mse.sum() * (1.0 / (R * T))
        ctx.save_for_backward(q_d, k_d, row_q, row_stats, *teacher_tensors(truth_d)[0])
        return loss

    @staticmethod
    @_lib.device_guarded
    def backward(ctx, grad_loss):
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None
        q, k, row_q, row_stats, *teacher = ctx.saved_tensors
        truth = TeacherScores(*teacher) if ctx.factored else teacher[0]
        lib = _lib.load()
        N, H, T, D = q.shape
        g = grad_loss.detach().to(torch.float32).reshape(1).contiguous()
        d_q = torch.empty((N, H, T, D), dtype=q.dtype, device=q.device)
        d_k = torch.empty((N, H, T, D), dtype=q.dtype, device=q.device)
        _lib.check(lib.sea_kd_score_loss_bwd(_p(q), _p(k), _lib.dtype_code(q.dtype), _lib.strides3(q), _lib.strides3(k),
                                             *teacher_args(truth), _p(row_q), _p(row_stats), _p(g), N, H, T, D, _p(d_q), _p(d_k),
                                             _lib.stream_ptr()),
                   "sea_kd_score_loss_bwd")
        return (d_q if ctx.needs_input_grad[0] else None), (d_k if ctx.needs_input_grad[1] else None), None


def kd_score_loss(q, k, truth_scores) -> torch.Tensor:
    """0.1 KL(batchmean) + MSE between softmax over the causal keys of q k^T (q, k (N,H,T,D), 16-bit) and softmax of
    `truth_scores` (N,H,T,T): a 0-dim fp32 tensor, differentiable with respect to q and k.  Causal and unpadded: row t sees keys
    0 .. t, whatever `truth_scores` holds beyond them.  `truth_scores` may be an `ops.TeacherScores`: the teacher's q k^T is then
    recomputed tile by tile (fp32 accumulator, not rounded to the data type) and no (N,H,T,T) tensor is read."""
    _require(q, k, truth_scores)
    return _KdScoreLossFn.apply(q, k, truth_scores)
