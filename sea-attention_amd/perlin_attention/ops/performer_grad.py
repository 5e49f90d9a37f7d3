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


def _forward(ctx, q, k, v, pos, projection, n_segments):
    with torch.no_grad():
        q_d, k_d, v_d, pos_d = q.detach(), k.detach(), v.detach(), pos.detach()
        out = performer_value(q_d, k_d, v_d, pos_d, projection, n_segments=n_segments)
        # the very tensor the forward launch read (ops.predictor's cache): the projection rounded to the data type, as fp32
        proj = _cached("proj", (projection,), q.dtype, lambda: projection.to(q.dtype).float().contiguous())
    ctx.save_for_backward(q_d, k_d, v_d, pos_d, proj)
    return out


@_lib.device_guarded
def _backward(grad_out, saved, need, segments=None, entry="sea_performer_causal_bwd"):
    """(dq, dk, dv, dpos), None where `need` is False.  `segments` None: `entry` (`sea_performer_causal_bwd`, or
    `sea_performer_causal_bwd_wide` with the same argument list); an int: that many row segments requested of
    `sea_performer_causal_bwd_seg`."""
    q, k, v, pos, proj = saved
    if not any(need[:4]):
        return None, None, None, None
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
    if segments is None:
        name, seg = entry, ()
        ws_bytes = getattr(lib, entry + "_workspace_bytes")(N, H, T, D, nb, code)
    else:
        name, seg = "sea_performer_causal_bwd_seg", (segments,)
        ws_bytes = lib.sea_performer_causal_bwd_seg_workspace_bytes(N, H, T, D, nb, code, segments)
    ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=q.device)
    _lib.check(getattr(lib, name)(
        _p(q), _p(k), _p(v), _p(pos_in), code, _p(proj), N, H, T, D, nb, _lib.strides3(q), _lib.strides3(k), _lib.strides3(v),
        pos_in.stride(0), _p(g), _p(d_q), _p(d_k), _p(d_v), _p(d_pos), *seg, _p(ws), ws_bytes, _lib.stream_ptr()), name)
    g_pos = None
    if need[3]:
        g_pos = torch.zeros(pos.shape, dtype=pos.dtype, device=pos.device)
        g_pos[:T] = d_pos
    return d_q if need[0] else None, d_k if need[1] else None, d_v if need[2] else None, g_pos


class _PerformerValueFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, q, k, v, pos, projection, n_segments):
        return _forward(ctx, q, k, v, pos, projection, n_segments)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        return (*_backward(grad_out, ctx.saved_tensors, ctx.needs_input_grad), None, None)


class _PerformerValueSegFn(torch.autograd.Function):
    """The same op with the backward cut into row segments (`grad_segments`, an int >= 1)"""

    @staticmethod
    def forward(ctx, q, k, v, pos, projection, n_segments, grad_segments):
        ctx.grad_segments = grad_segments
        return _forward(ctx, q, k, v, pos, projection, n_segments)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        return (*_backward(grad_out, ctx.saved_tensors, ctx.needs_input_grad, ctx.grad_segments), None, None, None)


class _PerformerValueWideFn(torch.autograd.Function):
    """The same op for the head sizes 80 and 128: the backward of csrc/sea_performer_bwd_wide.hip"""

    @staticmethod
    def forward(ctx, q, k, v, pos, projection, n_segments):
        return _forward(ctx, q, k, v, pos, projection, n_segments)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        return (*_backward(grad_out, ctx.saved_tensors, ctx.needs_input_grad, entry="sea_performer_causal_bwd_wide"), None, None)


def grad_segments_for(q, grad_segments):
    """The count `performer_value_autograd` requests for `grad_segments`: an int >= 1 as it is, "auto" one segment per
    ceil(CUs / (N H)) -- enough workgroups per sweep to give every CU of q's device one."""
    if grad_segments == "auto":
        cus = torch.cuda.get_device_properties(q.device).multi_processor_count
        return -(-cus // (q.shape[0] * q.shape[1]))
    if isinstance(grad_segments, bool) or not isinstance(grad_segments, int) or grad_segments < 1:
        raise ValueError(f"grad_segments must be None, an int >= 1 or 'auto', got {grad_segments!r}")
    return grad_segments


def performer_value_autograd(q, k, v, pos, projection, n_segments=None, grad_segments=None):
    """`ops.performer_value(q, k, v, pos, projection)` (no cumulative average), differentiable with respect to q, k, v and pos.
    `grad_segments`: None runs the backward as one workgroup per (n, h) and sweep; an int >= 1 or "auto" asks for that many row
    segments per (n, h) (`sea_performer_causal_bwd_seg`: one sequence per GPU leaves most CUs idle otherwise; 1 gives the bits
    of None).  Raises where `performer_value_grad_supported` does not hold: there is no other path behind this name."""
    if not performer_value_grad_supported(q, k, v, pos, projection):
        raise RuntimeError(f"performer_value_autograd: q {tuple(q.shape)} {q.dtype} strides {q.stride()}, nb={projection.shape[0]} "
                           "is outside the backward kernels (ops.performer_value_grad_supported)")
    if grad_segments is None:
        return _PerformerValueFn.apply(q, k, v, pos, projection, n_segments)
    return _PerformerValueSegFn.apply(q, k, v, pos, projection, n_segments, grad_segments_for(q, grad_segments))


def performer_value_grad_wide_supported(q, k, v, pos, projection) -> bool:
    """`performer_value_grad_supported` for the head sizes it refuses (`sea_performer_causal_bwd_wide_supported`: D = 80 / 128, up
    to 80 features): the same conditions on the tensors, the other predicate of the library.  False at D = 64."""
    ts = (q, k, v, pos, projection)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts) or q.dim() != 4 or pos.dim() != 2 or projection.dim() != 2:
        return False
    N, H, T, D = q.shape
    if q.dtype not in _DTYPES or not (k.dtype == v.dtype == q.dtype) or k.shape != q.shape or v.shape != q.shape:
        return False
    if min(N, H, T) < 1 or pos.shape[0] < T or pos.shape[1] != D or projection.shape[1] != D or T >= 1 << 24:
        return False
    if not _lib.load().sea_performer_causal_bwd_wide_supported(D, projection.shape[0], _lib.dtype_code(q.dtype)):
        return False
    return all(_aligned(t) for t in (q, k, v)) and (pos.dtype != q.dtype or _aligned(pos))


def performer_value_autograd_wide(q, k, v, pos, projection, n_segments=None):
    """`performer_value_autograd` for the head sizes 80 and 128 (`sea_performer_causal_bwd_wide`: the value columns split over two
    workgroups per (n, h); no row segments).  The forward is `ops.performer_value`; saved are q, k, v, pos and the rounded
    projection.  Raises where `performer_value_grad_wide_supported` does not hold: there is no other path behind this name."""
    if not performer_value_grad_wide_supported(q, k, v, pos, projection):
        raise RuntimeError(f"performer_value_autograd_wide: q {tuple(q.shape)} {q.dtype} strides {q.stride()}, "
                           f"nb={projection.shape[0]} is outside the wide-head backward kernels "
                           "(ops.performer_value_grad_wide_supported)")
    return _PerformerValueWideFn.apply(q, k, v, pos, projection, n_segments)
