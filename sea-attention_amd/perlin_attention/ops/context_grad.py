"""The sparse context branch under autograd on the HIP kernels (include/sea_hip_context_grad.h, csrc/sea_context_grad.hip).

`sparse_context_autograd(q, k, v, csr, row_scale, mix, out_dtype)` is the training branch of `PerlinAttention._forward_sparse` from
q, k, v to the (N, T, H D) context as one op:

    ctx[n, t, h D:(h + 1) D] = a rs o + (1 - a) round_dt(cumavg(v)[t])

with o the sparse product over `csr`, rs = row_scale (or None), a = mix and the average rounded to the data type as every other
path of the layer hands it to the mix (the gradient passes through that rounding as the identity, as autograd's `.to` does).
Forward: the gather attention launch `_SparseAttentionFn.forward` runs (probabilities kept, no epilogue, fp32 o), then
`sea_context_mix_fwd`.  Backward: `sea_context_mix_bwd` (dO, d row_scale, d mix), the unchanged `sea_sparse_attention_bwd` (form
AUTO, the per-stream workspace of `flat_csr`), `sea_context_dv_finish` (dv = dv_attn + the average's part, in v's dtype).
Saved: q, k, v, row_scale, mix, the per-entry probabilities and the unscaled fp32 o -- not the average, the scaled or the mixed
product or the permuted copy, in any dtype."""
import torch
from torch.autograd.function import once_differentiable

from ... import _lib
from . import flat_csr
from .flat_csr import _p

_DTYPES = (torch.float32, torch.float16, torch.bfloat16)
_CONTEXT_WS = {}          # per (device, stream): the chunk sums, kept like flat_csr's backward scratch and apart from it


def sparse_context_grad_supported(q, k, v, csr, row_scale, mix, out_dtype=torch.float32) -> bool:
    """What the kernels take (one predicate on both sides of the ABI, `sea_context_grad_supported`): device tensors, q, k, v
    (N,H,T,D) of one dtype (fp32 / fp16 / bf16) and ONE length (T_dst == T_src), D in {64, 80, 128}, v with unit feature stride and
    16-byte-aligned rows, mix (and row_scale, unless None) fp32 (N,H,T), out_dtype one of the three."""
    ts = (q, k, v, mix) + (() if row_scale is None else (row_scale,))
    if not all(isinstance(t, torch.Tensor) and t.is_cuda for t in ts) or not (q.dim() == k.dim() == v.dim() == 4):
        return False
    N, H, T, D = q.shape
    if q.dtype not in _DTYPES or out_dtype not in _DTYPES or k.dtype != q.dtype or v.dtype != q.dtype:
        return False
    if k.shape != (N, H, k.shape[2], D) or v.shape != k.shape or min(N, H, T, D) < 1:
        return False
    if not _lib.load().sea_context_grad_supported(T, k.shape[2], D, _lib.dtype_code(q.dtype), _lib.dtype_code(out_dtype)):
        return False
    if not isinstance(csr, flat_csr.FlatCSR) or (csr.N, csr.T_dst, csr.T_src, csr.H) != (N, T, T, H):
        return False
    if q.stride(-1) != 1 or k.stride(-1) != 1:
        return False
    if any(t.shape != (N, H, T) or t.dtype != torch.float32 for t in ts[3:]):
        return False
    vec = 16 // v.element_size()
    return v.stride(-1) == 1 and v.data_ptr() % 16 == 0 and all(s % vec == 0 and s >= 0 for s in v.stride()[:3]) and v.stride(2) >= D


class _SparseContextFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, q, k, v, csr, row_scale, mix, out_dtype):
        lib = _lib.load()
        N, H, T, D = q.shape
        with torch.no_grad():
            vd = v.detach()
            o, probs = flat_csr.sparse_attention(q.detach(), k.detach(), vd, csr, want_probs=True, path="gather")
            rs = None if row_scale is None else row_scale.detach().contiguous()
            a = mix.detach().contiguous()
            out = torch.empty((N, T, H * D), dtype=out_dtype, device=q.device)
            code, ocode = _lib.dtype_code(q.dtype), _lib.dtype_code(out_dtype)
            with torch.cuda.device(q.device):
                nb = int(lib.sea_context_grad_workspace_bytes(N, H, T, D, 0))
                ws = flat_csr._stream_workspace(_CONTEXT_WS, nb, q.device)
                _lib.check(lib.sea_context_mix_fwd(_p(vd), _lib.strides3(vd), _p(o), _p(rs), _p(a), code, ocode, N, H, T, D, _p(out),
                                                   _p(ws), nb, _lib.stream_ptr()), "sea_context_mix_fwd")
        ctx.save_for_backward(q, k, v, rs, a, probs, o)
        ctx.csr, ctx.out_dtype = csr, out_dtype
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, k, v, rs, a, probs, o = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need):
            return (None,) * 7
        csr, lib = ctx.csr, _lib.load()
        N, H, T, D = q.shape
        dev = q.device
        code, ocode = _lib.dtype_code(q.dtype), _lib.dtype_code(ctx.out_dtype)
        g = g.to(ctx.out_dtype).contiguous()
        qd, kd, vd = (t.detach() if t.stride(-1) == 1 else t.detach().contiguous() for t in (q, k, v))
        v0 = v.detach()
        d_o = torch.empty((N, H, T, D), dtype=torch.float32, device=dev)
        d_rs = torch.empty((N, H, T), dtype=torch.float32, device=dev) if need[4] and rs is not None else None
        d_a = torch.empty((N, H, T), dtype=torch.float32, device=dev) if need[5] else None
        dq = dk = dv = None
        with torch.cuda.device(dev):
            nb = int(lib.sea_context_grad_workspace_bytes(N, H, T, D, 1))
            ws = flat_csr._stream_workspace(_CONTEXT_WS, nb, dev)
            _lib.check(lib.sea_context_mix_bwd(_p(v0), _lib.strides3(v0), _p(o), _p(g), _p(rs), _p(a), code, ocode, N, H, T, D, _p(d_o),
                                               _p(d_rs), _p(d_a), _p(ws), nb, _lib.stream_ptr()), "sea_context_mix_bwd")
            if any(need[:3]):
                dq, dk, dv_attn = (torch.empty((N, H, T, D), dtype=torch.float32, device=dev) for _ in range(3))
                form = _lib.SEA_ATTN_BWD_AUTO
                nba = int(lib.sea_sparse_attention_bwd_workspace_bytes(code, N, H, T, D, csr.col.stride(0), form))
                wsa = flat_csr._bwd_workspace(nba, dev) if nba else None
                _lib.check(lib.sea_sparse_attention_bwd(
                    _p(qd), _p(kd), _p(vd), code, N, H, T, T, D, _lib.strides3(qd), _lib.strides3(kd), _lib.strides3(vd),
                    _p(csr.crow), _p(csr.col), csr.col.stride(0), _p(csr.head_off), _p(probs), probs.stride(0), _p(o), _p(d_o),
                    _p(dq), _p(dk), _p(dv_attn), _p(wsa), nba, form, _lib.stream_ptr()), "sea_sparse_attention_bwd")
                if need[2]:
                    dv = torch.empty((N, H, T, D), dtype=v.dtype, device=dev)
                    _lib.check(lib.sea_context_dv_finish(_p(g), _p(a), _p(dv_attn), code, ocode, N, H, T, D, _p(dv), _p(ws), nb,
                                                         _lib.stream_ptr()), "sea_context_dv_finish")
        return (dq.to(q.dtype) if need[0] else None, dk.to(k.dtype) if need[1] else None, dv, None, d_rs, d_a, None)


def clear_context_workspace():
    """Release the cached chunk-sum workspaces (4 - 8 MB per device and stream at 8 x 32 x 4096 x 64)."""
    _CONTEXT_WS.clear()


@_lib.device_guarded
def sparse_context_autograd(q, k, v, csr, row_scale, mix, out_dtype=torch.float32) -> torch.Tensor:
    """(N, T, H D) context of the sparse branch in `out_dtype`, differentiable with respect to q, k, v, row_scale and mix (d row_scale
    and d mix come back fp32, dq / dk / dv in the inputs' dtype; a gradient nobody wants comes back as None).  Raises where
    `sparse_context_grad_supported` does not hold: there is no other path behind this name."""
    _lib.require_gpu(q, k, v, row_scale, mix)
    if not sparse_context_grad_supported(q, k, v, csr, row_scale, mix, out_dtype):
        raise RuntimeError(f"sparse_context_autograd: q {tuple(q.shape)} {q.dtype}, k {tuple(k.shape)}, v {tuple(v.shape)} strides "
                           f"{v.stride()}, out_dtype {out_dtype} is outside the kernels (ops.sparse_context_grad_supported)")
    return _SparseContextFn.apply(q, k, v, csr, row_scale, mix, out_dtype)
