"""The teacher's attention scores in factored form: `TeacherScores(q, k)` stands for the (N,H,T,T) tensor q k^T without holding it.

`ops.kd_estimator_loss` and `ops.kd_score_loss` (and their `_parts` / `_supported`) take it wherever they take the score tensor
and then recompute the teacher's product tile by tile on the matrix cores (include/sea_hip_train.h, "the teacher");
`PerlinAttention` takes it as `attention_scores_truth` and calls `.dense()` once on every path the factored kernels do not serve.

The module is also the one place that knows both forms of the teacher: what either is to the `*_supported` predicates
(`teacher_supported`), to the C entries (`teacher_args`) and to an error message (`teacher_tensors`)."""
import torch

from ... import _lib
from .flat_csr import _p

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


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


def _rows_aligned(t):
    vec = 4 if t.dtype == torch.float32 else 8
    return (t.stride(-1) == 1 and t.stride(2) >= t.shape[-1] and all(s >= 0 and s % vec == 0 for s in t.stride()[:3])
            and t.data_ptr() % 16 == 0)


def teacher_supported(truth, device, N, H, T, head_sizes, max_t, dtype=None):
    """The teacher's half of the `*_supported` predicates, for a student of (N,H,T) on `device`: the score tensor (N,H,T,T) of
    fp32 / fp16 / bf16, or a `TeacherScores` whose q / k are 16-bit (`dtype` if given) with D in `head_sizes`; either way on
    the device, with an innermost stride of 1 and 16-byte-aligned rows."""
    factored = isinstance(truth, TeacherScores)
    tensors = (truth.q, truth.k) if factored else (truth,)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda and t.device == device and t.dim() == 4 for t in tensors):
        return False
    if T > max_t or min(N, H, T) < 1:
        return False
    if factored:
        q = truth.q
        if tuple(q.shape[:3]) != (N, H, T) or q.shape[-1] not in head_sizes:
            return False
        if q.dtype not in (torch.float16, torch.bfloat16) or (dtype is not None and q.dtype != dtype):
            return False
    elif tuple(truth.shape) != (N, H, T, T) or truth.dtype not in _DTYPES:
        return False
    return all(_rows_aligned(t) for t in tensors)


def teacher_tensors(truth):
    """(the device tensors of either form, how an error message shows them)"""
    if isinstance(truth, TeacherScores):
        q, k = truth.q, truth.k
        return (q, k), f"teacher q {tuple(q.shape)} {q.dtype} strides {q.stride()}, k strides {k.stride()}"
    return (truth,), f"truth {tuple(truth.shape)} {truth.dtype} strides {truth.stride()}"


def teacher_args(truth):
    """The eight teacher arguments of the C entries: truth, its dtype and strides, teacher_q, teacher_k, their dtype and strides,
    None / 0 for the form that is not given."""
    if isinstance(truth, TeacherScores):
        q, k = truth.q, truth.k
        return None, 0, None, _p(q), _p(k), _lib.dtype_code(q.dtype), _lib.strides3(q), _lib.strides3(k)
    return _p(truth), _lib.dtype_code(truth.dtype), _lib.strides3(truth), None, None, 0, None, None
