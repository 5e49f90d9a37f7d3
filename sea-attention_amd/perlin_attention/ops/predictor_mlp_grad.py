"""The predictor MLP under autograd on the HIP kernels (include/sea_hip_predictor_mlp_grad.h, csrc/sea_mlp_bwd.hip).

`predictor_mlp_autograd(x, enc_lin, enc_ln, dec_lin, ln1, scaler_lin)` is `ops.predictor_mlp` without its gates and with a backward:
the forward is the same launch, the backward recomputes the chain from x and runs the row, d_x, weight-gradient and reduce kernels.
Saved between the two: x and the eight parameters of enc_lin, enc_ln, dec_lin and ln1.  The two gates stay out of the op: in training
`attention_predictor_dec_scaler` is the torch Linear on tpred, whose gradient comes back as the gradient of tpred.  Parameter
gradients are fp32 sums in a fixed order, cast once."""
import torch
from torch.autograd.function import once_differentiable

from ... import _lib
from .flat_csr import _p
from .predictor import mlp_images, predictor_mlp

_DTYPES = (torch.float16, torch.bfloat16)


def predictor_mlp_grad_supported(x, enc_lin, enc_ln, dec_lin, ln1, scaler_lin) -> bool:
    """What the backward kernels take (one predicate on both sides of the ABI, `sea_predictor_mlp_bwd_supported`): a device tensor
    x (N, H, T, Din) of fp16 / bf16 with a contiguous last axis and 16-byte aligned rows, affine modules with biases, and a
    (D1, D2, H, Din) the library has a form for.  fp32 data is refused: the layer keeps its torch path there."""
    if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() == 4 and x.dtype in _DTYPES):
        return False
    N, H, T, Din = x.shape
    if min(N, H, T, Din) < 1 or N * H * T >= 1 << 30 or x.stride(-1) != 1 or any(s % 8 for s in x.stride()[:3]) or x.data_ptr() % 16:
        return False
    if any(m.bias is None for m in (enc_lin, dec_lin, scaler_lin)) or not (enc_ln.elementwise_affine and ln1.elementwise_affine):
        return False
    D1, D2 = enc_lin.out_features, dec_lin.out_features
    if (enc_lin.in_features != Din or dec_lin.in_features != D1 or tuple(enc_ln.normalized_shape) != (D1,)
            or tuple(ln1.normalized_shape) != (D2 // 2,) or scaler_lin.in_features != D1 or scaler_lin.out_features != 2):
        return False
    return bool(_lib.load().sea_predictor_mlp_bwd_supported(D1, D2, H, Din, _lib.dtype_code(x.dtype)))


class _PredictorMlpFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, w1, b1, g1, be1, w2, b2, g2, be2, mods, want_tpred):
        with torch.no_grad():
            x_d = x.detach()
            x_c8, tpred, _row_scale, _avg_scale = predictor_mlp(x_d, *mods, want_tpred=want_tpred)   # (the gates: discarded)
        ctx.save_for_backward(x_d, w1, b1, g1, be1, w2, b2, g2, be2)
        ctx.mods = mods
        ctx.set_materialize_grads(False)                     # an output nobody differentiates hands the backward None, not zeros
        if tpred is None:
            return x_c8, None
        return x_c8, tpred

    @staticmethod
    @once_differentiable
    @_lib.device_guarded
    def backward(ctx, g_y, g_tpred):
        x = ctx.saved_tensors[0]
        params = ctx.saved_tensors[1:]
        need = ctx.needs_input_grad
        if not any(need[:9]):
            return (None,) * 11
        enc_lin, enc_ln, dec_lin, ln1, scaler_lin = ctx.mods
        lib = _lib.load()
        N, H, T, Din = x.shape
        D1, D2, dt = enc_lin.out_features, dec_lin.out_features, x.dtype
        code = _lib.dtype_code(dt)
        # the forward's own images: the same cache entry, which misses when a parameter has changed since (`_version`)
        w1p, w2p, vec = mlp_images(dt, x.device, *ctx.mods)
        Wd = D2 // 2
        g_y = torch.zeros((N, T, H // 4, Wd, 8), dtype=dt, device=x.device) if g_y is None else g_y.to(dt).contiguous()
        g_tpred = None if g_tpred is None else g_tpred.to(dt).contiguous()
        d_x = torch.empty_strided(x.shape, x.stride(), dtype=dt, device=x.device) if need[0] else None
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=x.device)
        outs = (f32(D1, Din), f32(D1), f32(D1), f32(D1), f32(D2, D1), f32(D2), f32(D2 // 2), f32(D2 // 2))
        ws_bytes = lib.sea_predictor_mlp_bwd_workspace_bytes(N, H, T, Din, D1, D2, code)
        ws = torch.empty((max(ws_bytes, 16),), dtype=torch.uint8, device=x.device)
        _lib.check(lib.sea_predictor_mlp_bwd(_p(x), _lib.strides3(x), _p(g_y), _p(g_tpred), code, N, H, T, Din, D1, D2, _p(w1p), _p(w2p),
                                             _p(vec), float(enc_ln.eps), float(ln1.eps), _p(d_x), *[_p(o) for o in outs], _p(ws),
                                             ws_bytes, _lib.stream_ptr()), "sea_predictor_mlp_bwd")
        grads = [o.to(q.dtype).view_as(q) if nd else None for o, q, nd in zip(outs, params, need[1:9])]
        return (d_x, *grads, None, None)


def predictor_mlp_autograd(x, enc_lin, enc_ln, dec_lin, ln1, scaler_lin, want_tpred: bool = True):
    """`ops.predictor_mlp(x, ...)` -> (x_c8, tpred or None), differentiable with respect to x and the parameters of enc_lin, enc_ln,
    dec_lin and ln1 (not scaler_lin: the gates are not outputs).  Raises where `predictor_mlp_grad_supported` does not hold: there
    is no other path behind this name."""
    if not predictor_mlp_grad_supported(x, enc_lin, enc_ln, dec_lin, ln1, scaler_lin):
        raise RuntimeError(f"predictor_mlp_autograd: x {tuple(x.shape) if isinstance(x, torch.Tensor) else x} "
                           f"{getattr(x, 'dtype', None)}, D1={enc_lin.out_features}, D2={dec_lin.out_features} is outside the backward "
                           "kernels (ops.predictor_mlp_grad_supported)")
    return _PredictorMlpFn.apply(x, enc_lin.weight, enc_lin.bias, enc_ln.weight, enc_ln.bias, dec_lin.weight, dec_lin.bias,
                                 ln1.weight, ln1.bias, (enc_lin, enc_ln, dec_lin, ln1, scaler_lin), bool(want_tpred))
