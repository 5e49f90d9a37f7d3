"""The causal Performer under autograd on the HIP kernels (include/sea_hip_estimator_grad.h, csrc/sea_performer_bwd.hip).

`performer_value_autograd(q, k, v, pos, projection)` is `ops.performer_value` with a backward: the forward is the same launch,
the backward recomputes the feature maps, the running state and the denominators chunk by chunk in two sweeps and one fixed-order
reduction.  Saved between the two: q, k, v, pos and the fp32 projection the forward used -- no feature map, no (C x C) product,
no state.  Gradients go to q, k, v (their dtype) and pos (its dtype and shape; rows at or beyond T get exactly 0); the projection
is a buffer and gets none."""
import torch
from torch.autograd.function import once_differentiable

from ... import _lib
from .flat_csr import _p
from .predictor import _cached, performer_value

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _aligned(t) -> bool:
    vec = 16 // t.element_size()
    return t.stride(-1) == 1 and t.data_ptr() % 16 == 0 and all(s % vec == 0 and s >= 0 for s in t.stride()[:-1])


def performer_value_grad_supported(q, k, v, pos, projection) -> bool:
    """What the backward kernels take (one predicate on both sides of the ABI, `sea_performer_causal_bwd_supported`): device
    tensors q, k, v (N,H,T,D) of one dtype among fp32 / fp16 / bf16 with an innermost stride of 1 and 16-byte-aligned rows,
    pos (>= T, D), projection (nb, D), and a (D, nb) the library has a form for."""
    ts = (q, k, v, pos, projection)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts) or q.dim() != 4 or pos.dim() != 2 or projection.dim() != 2:
        return False
    N, H, T, D = q.shape
    if q.dtype not in _DTYPES or not (k.dtype == v.dtype == q.dtype) or k.shape != q.shape or v.shape != q.shape:
        return False
    if min(N, H, T) < 1 or pos.shape[0] < T or pos.shape[1] != D or projection.shape[1] != D or T >= 1 << 24:
        return False
    if not _lib.load().sea_performer_causal_bwd_supported(D, projection.shape[0], _lib.dtype_code(q.dtype)):
        return False
    return all(_aligned(t) for t in (q, k, v)) and (pos.dtype != q.dtype or _aligned(pos))


class _PerformerValueFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, q, k, v, pos, projection, n_segments):
        with torch.no_grad():
            q_d, k_d, v_d, pos_d = q.detach(), k.detach(), v.detach(), pos.detach()
            out = performer_value(q_d, k_d, v_d, pos_d, projection, n_segments=n_segments)
            # the very tensor the forward launch read (ops.predictor's cache): the projection rounded to the data type, as fp32
            proj = _cached("proj", (projection,), q.dtype, lambda: projection.to(q.dtype).float().contiguous())
        ctx.save_for_backward(q_d, k_d, v_d, pos_d, proj)
        return out

    @staticmethod
    @once_differentiable
    @_lib.device_guarded
    def backward(ctx, grad_out):
        q, k, v, pos, proj = ctx.saved_tensors
        if not any(ctx.needs_input_grad[:4]):
            return None, None, None, None, None, None
        lib = _lib.load()
        N, H, T, D = q.shape
        nb = proj.shape[0]
        code = _lib.dtype_code(q.dtype)
        g = grad_out if grad_out.dtype == q.dtype else grad_out.to(q.dtype)
        g = g.contiguous()
        pos_in = pos if pos.dtype == q.dtype else pos.to(q.dtype)
        pos_in = pos_in if pos_in.stride(-1) == 1 else pos_in.contiguous()
        d_q, d_k, d_v = (torch.empty((N, H, T, D), dtype=q.dtype, device=q.device) for _ in range(3))
        d_pos = torch.empty((T, D), dtype=torch.float32, device=q.device)
        ws_bytes = lib.sea_performer_causal_bwd_workspace_bytes(N, H, T, D, nb, code)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=q.device)
        _lib.check(lib.sea_performer_causal_bwd(
            _p(q), _p(k), _p(v), _p(pos_in), code, _p(proj), N, H, T, D, nb, _lib.strides3(q), _lib.strides3(k), _lib.strides3(v),
            pos_in.stride(0), _p(g), _p(d_q), _p(d_k), _p(d_v), _p(d_pos), _p(ws), ws_bytes, _lib.stream_ptr()),
            "sea_performer_causal_bwd")
        need = ctx.needs_input_grad
        g_pos = None
        if need[3]:
            g_pos = torch.zeros(pos.shape, dtype=pos.dtype, device=pos.device)
            g_pos[:T] = d_pos
        return (d_q if need[0] else None, d_k if need[1] else None, d_v if need[2] else None, g_pos, None, None)


def performer_value_autograd(q, k, v, pos, projection, n_segments=None):
    """`ops.performer_value(q, k, v, pos, projection)` (no cumulative average), differentiable with respect to q, k, v and pos.
    Raises where `performer_value_grad_supported` does not hold: there is no other path behind this name."""
    if not performer_value_grad_supported(q, k, v, pos, projection):
        raise RuntimeError(f"performer_value_autograd: q {tuple(q.shape)} {q.dtype} strides {q.stride()}, nb={projection.shape[0]} "
                           "is outside the backward kernels (ops.performer_value_grad_supported)")
    return _PerformerValueFn.apply(q, k, v, pos, projection, n_segments)
