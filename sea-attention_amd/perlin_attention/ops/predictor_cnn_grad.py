"""The predictor CNN's (convolution, ReLU) pairs under autograd on the HIP kernels (include/sea_hip_predictor_cnn_grad.h,
csrc/sea_conv_bwd.hip).

`causal_conv_relu_autograd(x, weight, bias, ksize, dilation, pad_w)` is `ops.causal_conv_c8(..., relu=True)` with a backward: the
forward is the same launch, the backward masks the incoming gradient with y > 0 as it stages it and runs the data- and
weight-gradient kernels.  Saved between the two: x and y -- the very tensors -- and the two parameters.  Gradients go to x (C8, its
dtype), to weight in the module's (C, C, 2k-1, k) shape with exact zeros in the dead rows, and to bias; both parameter gradients
are fp32 sums in a fixed order, cast once."""
import torch
from torch.autograd.function import once_differentiable

from ... import _lib
from .flat_csr import _p
from .predictor import _cached, causal_conv_c8, pack_conv_weight

_DTYPES = (torch.float16, torch.bfloat16)


def causal_conv_relu_grad_supported(x, weight, bias, ksize, dilation, pad_w) -> bool:
    """What the backward kernels take (one predicate on both sides of the ABI, `sea_causal_conv_relu_bwd_supported`): a dense C8
    device tensor x (N, T, C/8, W, 8) of fp16 / bf16, weight (C, C, 2k-1, k), bias (C), and a (C, W, ksize, dilation, pad_w) the
    library has a form for.  fp32 data is refused: the layer keeps its torch path there."""
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in (x, weight, bias)) or x.dim() != 5 or weight.dim() != 4:
        return False
    N, T, C8, W, e = x.shape
    C = C8 * 8
    if e != 8 or x.dtype not in _DTYPES or not x.is_contiguous() or min(N, T, C8, W) < 1 or N * T >= 1 << 30 or x.data_ptr() % 16:
        return False
    if weight.shape != (C, C, 2 * ksize - 1, ksize) or bias.shape != (C,):
        return False
    return bool(_lib.load().sea_causal_conv_relu_bwd_supported(C, W, int(ksize), int(dilation), int(pad_w), _lib.dtype_code(x.dtype)))


class _ConvReluFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, weight, bias, ksize, dilation, pad_w):
        with torch.no_grad():
            x_d = x.detach()
            y = causal_conv_c8(x_d, weight, bias, ksize, dilation, pad_w, relu=True)   # (the parameters themselves: one cached image)
        ctx.save_for_backward(x_d, y, weight, bias)
        ctx.ksize, ctx.dilation, ctx.pad_w = int(ksize), int(dilation), int(pad_w)
        return y

    @staticmethod
    @once_differentiable
    @_lib.device_guarded
    def backward(ctx, g):
        x, y, weight, bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:3]):
            return (None,) * 6
        lib = _lib.load()
        N, T, C8, W, _e = x.shape
        C, dt, k = C8 * 8, x.dtype, ctx.ksize
        code = _lib.dtype_code(dt)
        # the forward's own image: the cache misses when the parameter has changed since (`_version`), as it does for the forward
        (wp, CinP), _bf = _cached("conv", (weight, bias), dt,
                                  lambda: (pack_conv_weight(weight, k, dt), bias.to(dt).float().contiguous()))
        g = g.to(dt).contiguous()
        d_x = torch.empty_like(x) if need[0] else None
        d_w = torch.empty((C, C, k, k), dtype=torch.float32, device=x.device)
        d_b = torch.empty((C,), dtype=torch.float32, device=x.device)
        ws_bytes = lib.sea_causal_conv_relu_bwd_workspace_bytes(N, T, W, C, ctx.dilation, code)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=x.device)
        _lib.check(lib.sea_causal_conv_relu_bwd(_p(x), _p(y), _p(g), code, N, T, W, C, _p(wp), CinP, ctx.dilation, ctx.pad_w,
                                                _p(d_x), _p(d_w), _p(d_b), _p(ws), ws_bytes, _lib.stream_ptr()),
                   "sea_causal_conv_relu_bwd")
        g_w = None
        if need[1]:
            g_w = torch.zeros_like(weight)                   # the dead rows k .. 2k-2: exact zeros
            g_w[:, :, :k, :] = d_w
        return d_x, g_w, (d_b.to(bias.dtype) if need[2] else None), None, None, None


def causal_conv_relu_autograd(x, weight, bias, ksize, dilation, pad_w):
    """`ops.causal_conv_c8(x, weight, bias, ksize, dilation, pad_w, relu=True)` -> y, differentiable with respect to x, weight and
    bias.  Raises where `causal_conv_relu_grad_supported` does not hold: there is no other path behind this name."""
    if not causal_conv_relu_grad_supported(x, weight, bias, ksize, dilation, pad_w):
        raise RuntimeError(f"causal_conv_relu_autograd: x {tuple(x.shape)} {x.dtype}, weight {tuple(weight.shape)}, ksize={ksize}, "
                           f"dilation={dilation}, pad_w={pad_w} is outside the backward kernels (ops.causal_conv_relu_grad_supported)")
    return _ConvReluFn.apply(x, weight, bias, ksize, dilation, pad_w)
