"""The teacher's attention scores in factored form: `TeacherScores(q, k)` stands for the (N,H,T,T) tensor q k^T without holding it.

`ops.kd_estimator_loss` and `ops.kd_score_loss` (and their `_parts` / `_supported`) take it wherever they take the score tensor
and then recompute the teacher's product tile by tile on the matrix cores (include/sea_hip_train.h t5 - t7); `PerlinAttention`
takes it as `attention_scores_truth` and calls `.dense()` once on every path the factored kernels do not serve."""
import torch


class TeacherScores:
    """q, k (N,H,T,D) of one dtype, held detached (the teacher gets no gradient); q already carries the teacher's scaling
    (OPT: `q_proj(h) * scaling`)."""

    def __init__(self, q, k):
        if not (isinstance(q, torch.Tensor) and isinstance(k, torch.Tensor)):
            raise TypeError("TeacherScores: q and k must be tensors")
        if q.dim() != 4 or q.shape != k.shape:
            raise ValueError(f"TeacherScores: q {tuple(q.shape)} and k {tuple(k.shape)} must be (N,H,T,D) of one shape")
        if q.dtype != k.dtype:
            raise ValueError(f"TeacherScores: q is {q.dtype}, k is {k.dtype}; they must share a dtype")
        if q.device != k.device:
            raise ValueError(f"TeacherScores: q is on {q.device}, k is on {k.device}")
        self.q, self.k = q.detach(), k.detach()

    @property
    def shape(self):
        N, H, T, _D = self.q.shape
        return torch.Size((N, H, T, T))

    @property
    def dtype(self):
        return self.q.dtype

    @property
    def device(self):
        return self.q.device

    def to(self, device, non_blocking=False):
        q, k = self.q.to(device, non_blocking=non_blocking), self.k.to(device, non_blocking=non_blocking)
        return self if (q is self.q and k is self.k) else TeacherScores(q, k)

    def dense(self):
        """q @ k^T in q's dtype: what the teacher's own bmm would have handed over"""
        return torch.matmul(self.q, self.k.transpose(-1, -2))

    def __repr__(self):
        return f"TeacherScores(shape={tuple(self.shape)}, dtype={self.dtype}, device={self.device})"


def qk_supported(ts, N, H, T, head_sizes, max_t, dtype=None):
    """A device `TeacherScores` the factored kernels take for a student of (N,H,T): 16-bit (`dtype` if given), D in
    `head_sizes`, rows 16-byte aligned"""
    from .kd_loss import _rows_aligned
    q, k = ts.q, ts.k
    if not (q.is_cuda and k.is_cuda and q.device == k.device):
        return False
    if tuple(q.shape[:3]) != (N, H, T) or q.shape[-1] not in head_sizes or T > max_t or min(N, H, T) < 1:
        return False
    if q.dtype not in (torch.float16, torch.bfloat16) or (dtype is not None and q.dtype != dtype):
        return False
    return _rows_aligned(q) and _rows_aligned(k)
