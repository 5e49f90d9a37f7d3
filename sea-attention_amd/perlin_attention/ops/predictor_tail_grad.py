"""The predictor tail under autograd on the HIP kernels (include/sea_hip_predictor_grad.h, csrc/sea_tail_bwd.hip).

`predictor_tail_autograd(y, conv_w, conv_b, ln_w, ln_b, up, T_m, eps)` is `ops.predictor_tail(..., want_scores=True)` with a
backward: the forward is the same launch, the backward recomputes z, the resize, the LayerNorm statistics and (when the
probabilities carry a gradient) the softmax row by row.  Saved between the two: y -- the very tensor, with its strides -- and the
four parameter tensors; nothing of the size of the (N,H,T,T_m) map.  Gradients go to y (its dtype, contiguous), conv_w, ln_w and
ln_b (their dtypes, cast from fp32 sums in a fixed order) and conv_b, which gets exact zeros: the bias shifts every pixel of a row
alike and the LayerNorm removes the shift."""
import torch
from torch.autograd.function import once_differentiable

from ... import _lib
from .flat_csr import _p
from .predictor import predictor_tail

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def predictor_tail_grad_supported(y, conv_w, conv_b, ln_w, ln_b, up, T_m) -> bool:
    """What the backward kernel takes (one predicate on both sides of the ABI, `sea_predictor_tail_bwd_supported`): device tensors,
    y (N,C,T,W4) of fp32 / fp16 / bf16 with the width or the channels innermost, 16-byte-aligned rows and no two elements at one
    address, conv_w (H,C), conv_b (H), ln_w and ln_b (T_m), and a (C, H, W4, up, T_m) the library has a form for."""
    ts = (y, conv_w, conv_b, ln_w, ln_b)
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts) or y.dim() != 4 or conv_w.dim() != 2:
        return False
    N, C, T, W4 = y.shape
    H = conv_w.shape[0]
    if y.dtype not in _DTYPES or min(N, C, T, W4, H) < 1 or N * T >= 1 << 31:
        return False
    if conv_w.shape != (H, C) or conv_b.shape != (H,) or ln_w.shape != (T_m,) or ln_b.shape != (T_m,):
        return False
    if not _lib.load().sea_predictor_tail_bwd_supported(C, H, W4, int(up), int(T_m), _lib.dtype_code(y.dtype)):
        return False
    vec = 16 // y.element_size()
    sn, sc, st, sw = y.stride()
    if not (sw == 1 or sc == 1) or y.data_ptr() % 16:
        return False
    if any(s % vec for s in (sn, st, sc if sw == 1 else sw)):
        return False
    span = 1                                                 # each stride at least the extent of the smaller ones: nothing overlaps
    for s, e in sorted(zip(y.stride(), y.shape)):
        if e > 1 and s < span:
            return False
        span += (e - 1) * s
    return True


class _PredictorTailFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, y, conv_w, conv_b, ln_w, ln_b, up, T_m, eps):
        with torch.no_grad():
            y_d = y.detach()
            probs, scores = predictor_tail(y_d, conv_w.detach(), conv_b.detach(), ln_w.detach(), ln_b.detach(), up=up, T_m=T_m,
                                           eps=eps, want_scores=True)
        ctx.save_for_backward(y_d, conv_w, conv_b, ln_w, ln_b)
        ctx.up, ctx.T_m, ctx.eps = int(up), int(T_m), float(eps)
        ctx.set_materialize_grads(False)                     # an output nobody differentiates arrives as None, not as zeros
        return probs, scores

    @staticmethod
    @once_differentiable
    @_lib.device_guarded
    def backward(ctx, g_probs, g_scores):
        y, conv_w, conv_b, ln_w, ln_b = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:5]) or (g_probs is None and g_scores is None):
            return (None,) * 8
        lib = _lib.load()
        N, C, T, W4 = y.shape
        H, T_m, dt = conv_w.shape[0], ctx.T_m, y.dtype
        code = _lib.dtype_code(dt)
        # the parameters as the forward launch saw them: rounded to the data type (ops.predictor._tail_pack)
        w = conv_w.detach().to(dt).float().contiguous()
        gamma, beta = ln_w.detach().to(dt).contiguous(), ln_b.detach().to(dt).contiguous()
        g_s = None if g_scores is None else g_scores.to(dt).contiguous()
        g_p = None if g_probs is None else g_probs.to(dt).contiguous()
        d_y = torch.empty((N, C, T, W4), dtype=dt, device=y.device)
        d_w = torch.empty((H, C), dtype=torch.float32, device=y.device)
        d_gamma, d_beta = (torch.empty((T_m,), dtype=torch.float32, device=y.device) for _ in range(2))
        ws_bytes = lib.sea_predictor_tail_bwd_workspace_bytes(N, C, H, T, W4, ctx.up, T_m, code)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=y.device)
        _lib.check(lib.sea_predictor_tail_bwd(
            _p(y), code, N, C, H, T, W4, ctx.up, T_m, _lib.strides4(y), _p(w), _p(gamma), _p(beta), ctx.eps, _p(g_s), _p(g_p),
            _p(d_y), _p(d_w), _p(d_gamma), _p(d_beta), _p(ws), ws_bytes, _lib.stream_ptr()), "sea_predictor_tail_bwd")
        return (d_y if need[0] else None,
                d_w.to(conv_w.dtype) if need[1] else None,
                torch.zeros_like(conv_b) if need[2] else None,
                d_gamma.to(ln_w.dtype) if need[3] else None,
                d_beta.to(ln_b.dtype) if need[4] else None, None, None, None)


def predictor_tail_autograd(y, conv_w, conv_b, ln_w, ln_b, up, T_m, eps=1e-5):
    """`ops.predictor_tail(y, conv_w, conv_b, ln_w, ln_b, up, T_m, eps, want_scores=True)` -> (probs, scores), differentiable with
    respect to y, conv_w, conv_b, ln_w and ln_b.  Raises where `predictor_tail_grad_supported` does not hold: there is no other path
    behind this name."""
    if not predictor_tail_grad_supported(y, conv_w, conv_b, ln_w, ln_b, up, T_m):
        raise RuntimeError(f"predictor_tail_autograd: y {tuple(y.shape)} {y.dtype} strides {y.stride()}, H={conv_w.shape[0]}, up={up}, "
                           f"T_m={T_m} is outside the backward kernel (ops.predictor_tail_grad_supported)")
    return _PredictorTailFn.apply(y, conv_w, conv_b, ln_w, ln_b, up, T_m, eps)
