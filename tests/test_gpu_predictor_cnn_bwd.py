"""The (convolution, ReLU) backward on the HIP kernels (csrc/sea_conv_bwd.hip, ops.causal_conv_relu_autograd) and the layer switch
`PerlinAttention.fused_cnn_grad`, DESIGN 5.12.

Op tier.  Reference: fp64 autograd of the linear F.conv2d on the rounded, top-padded input with grad_outputs dp = g (.) (y > 0), y
the op's own output (no element is excluded for a sign flip near zero).  Yardstick: the same expression in fp32 on the CPU, its
gradients cast to the data type.  Bar per quantity: 4 x the yardstick's largest error, at least 2^-22 of the reference's largest
magnitude (5.7's rule).  Module tier: 5.11's layer; reference an fp64 stand-in for the op, yardstick the switch-off run."""
import functools

import pytest
import torch
import torch.nn.functional as F

from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import ops
from sea_attention_amd.perlin_attention.ops import predictor_cnn_grad
from test_predictor_tail_bwd_reference import bar_of

DEV = "cuda"
F16, BF, F64 = torch.float16, torch.bfloat16, torch.float64


def rows_per_block(N, C, W, d, dt):
    """from the workspace arithmetic: the first T at which a sequence needs a second block"""
    size = lambda T: _lib.load().sea_causal_conv_relu_bwd_workspace_bytes(N, T, W, C, d, _lib.dtype_code(dt))
    return next(T for T in range(1, 256) if size(T + 1) > size(T))


#        N  C   T     W   d  dtype
CASES = [(2, 8, 1, 16, 2, BF),          # one row, W below a k-step, C below a tile
         (2, 24, 3, 24, 2, F16),        # T < 2d, W % 16 != 0
         (3, 40, 5, 32, 1, BF),         # dilation 1, C % 16 != 0
         (2, 64, None, 64, 2, BF),      # rows_per_block + 1: a block boundary with both halos
         (2, 80, 70, 64, 2, F16)]       # the split output, several blocks per sequence


def _grads(x, w3, dp, d):
    """(dx, dW, db) of sum(dp (.) conv(x)) in the precision of the arguments: the linear expression, top-padded"""
    with torch.enable_grad():
        x, w3 = x.clone().requires_grad_(True), w3.clone().requires_grad_(True)
        out = F.conv2d(F.pad(x, (0, 0, 2 * d, 0)), w3, None, 1, (0, d), d)
        return (*torch.autograd.grad(out, [x, w3], grad_outputs=dp), dp.sum((0, 2, 3)))


@functools.lru_cache(maxsize=None)
def _inputs(idx):
    N, C, T, W, d, dt = CASES[idx]
    T = T or rows_per_block(N, C, W, d, dt) + 1
    gen = torch.Generator().manual_seed(50 + idx)
    x = torch.randn((N, C, T, W), generator=gen).to(dt)
    w = torch.zeros((C, C, 5, 3))
    w[:, :, :3] = torch.randn((C, C, 3, 3), generator=gen) / (9 * C) ** 0.5
    g = torch.randn((N, C, T, W), generator=gen).to(dt)
    return x, w.to(dt), torch.zeros(C, dtype=dt), g


def _run(idx, need_x=True):
    d = CASES[idx][4]
    x, w, b, g = _inputs(idx)
    x8 = ops.to_c8(x.to(DEV)).requires_grad_(need_x)
    w, b = w.to(DEV).requires_grad_(True), b.to(DEV).requires_grad_(True)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y = ops.causal_conv_relu_autograd(x8, w, b, 3, d, d)
    grads = torch.autograd.grad(y, [x8, w, b] if need_x else [w, b], grad_outputs=ops.to_c8(g.to(DEV)), retain_graph=True)
    again = torch.autograd.grad(y, [x8, w, b] if need_x else [w, b], grad_outputs=ops.to_c8(g.to(DEV)))
    torch.cuda.synchronize()
    return (x8, w, b, y), saved, grads, again


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=["N%d-C%d-T%s-W%d-d%d-%s" % (*c[:5], str(c[5]).split(".")[1]) for c in CASES])
def test_kernels_against_fp64_reference(idx):
    N, C, _T, W, d, dt = CASES[idx]
    x, w, _b, g = _inputs(idx)
    (x8, wd, bd, y), saved, got, again = _run(idx)
    assert torch.equal(y, ops.causal_conv_c8(x8.detach(), wd.detach(), bd.detach(), 3, d, d, relu=True))   # the inference launch
    assert [t.data_ptr() for t in saved] == [t.data_ptr() for t in (x8, y, wd, bd)]       # x, y, weight, bias: the very tensors
    y4 = ops.from_c8(y.detach()).cpu()
    assert 0.25 <= (y4 == 0).float().mean().item() <= 0.75
    dp = g.double() * (y4 > 0)
    ref = _grads(x.double(), w[:, :, :3].double(), dp, d)
    yard = [t.to(dt) for t in _grads(x.float(), w[:, :, :3].float(), dp.float(), d)]
    dx, dW, db = got
    assert dx.dtype == dW.dtype == db.dtype == dt and dW.shape == (C, C, 5, 3) and (dW[:, :, 3:] == 0).all()   # dead rows: exact zeros
    failures = []
    for name, v, r, yd in zip(("dx", "dW", "db"), (ops.from_c8(dx), dW[:, :, :3], db), ref, yard):
        bar, err = bar_of(yd, r), (v.double().cpu() - r).abs().max().item()
        print(f"[cnn-bwd] {tuple(x.shape)} d={d} {dt} {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f} (max |ref| {r.abs().max().item():.3e})")
        if not (torch.isfinite(v).all() and err <= bar):
            failures.append((name, err, bar))
    assert not failures, failures
    assert all(torch.equal(a, b) for a, b in zip(got, again))                              # no atomics, one order: the same bits

    class Ctx:                                                                             # d_x = None when x needs no gradient
        saved_tensors, needs_input_grad, ksize, dilation, pad_w = tuple(saved), (False, True, True, False, False, False), 3, d, d
    res = predictor_cnn_grad._ConvReluFn.backward(Ctx, ops.to_c8(g.to(DEV)))
    assert res[0] is None and torch.equal(res[1], dW) and torch.equal(res[2], db) and res[3:] == (None,) * 3


@pytest.mark.gpu
def test_fp32_parameters_under_bf16_data():
    """fp32 master weights: weight and bias are fp32 leaves whose values bf16 cannot hold -- every live value (1 + 2^-10) times a bf16
    number, which rounds back to that number.  The forward is bitwise the forward on the rounded parameters, both gradients come back
    fp32, and every gradient is held to this file's fp64 reference on the rounded weight under this file's bar."""
    idx = 0
    N, C, _T, W, d, dt = CASES[idx]
    x, w, _b, g = _inputs(idx)
    b = (0.1 * torch.randn(C, generator=torch.Generator().manual_seed(58))).to(dt)          # (the case's own bias is zero)
    w32, b32 = (t.float() * (1 + 2.0 ** -10) for t in (w, b))
    assert dt == BF and torch.equal(w32.to(BF), w) and torch.equal(b32.to(BF), b)
    assert (w32[:, :, :3] != w[:, :, :3].float()).float().mean().item() > 0.99 and (b32 != b.float()).all() and (w32[:, :, 3:] == 0).all()
    x8 = ops.to_c8(x.to(DEV)).requires_grad_(True)
    wd, bd = w32.to(DEV).requires_grad_(True), b32.to(DEV).requires_grad_(True)
    y = ops.causal_conv_relu_autograd(x8, wd, bd, 3, d, d)
    dx, dW, db = torch.autograd.grad(y, [x8, wd, bd], grad_outputs=ops.to_c8(g.to(DEV)))
    torch.cuda.synchronize()
    assert torch.equal(y, ops.causal_conv_c8(x8.detach(), w.to(DEV), b.to(DEV), 3, d, d, relu=True))
    assert (dx.dtype, dW.dtype, db.dtype) == (BF, torch.float32, torch.float32) and dW.shape == (C, C, 5, 3) and (dW[:, :, 3:] == 0).all()
    y4 = ops.from_c8(y.detach()).cpu()
    assert 0.25 <= (y4 == 0).float().mean().item() <= 0.75
    dp = g.double() * (y4 > 0)
    ref = _grads(x.double(), w[:, :, :3].double(), dp, d)
    yard = [t.to(dt) for t in _grads(x.float(), w[:, :, :3].float(), dp.float(), d)]
    failures = []
    for name, v, r, yd in zip(("dx", "dW", "db"), (ops.from_c8(dx), dW[:, :, :3], db), ref, yard):
        bar, err = bar_of(yd, r), (v.double().cpu() - r).abs().max().item()
        print(f"[cnn-bwd] {tuple(x.shape)} d={d} fp32 parameters {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
        if not (torch.isfinite(v).all() and err <= bar):
            failures.append((name, err, bar))
    assert not failures, failures


@pytest.mark.gpu
def test_outside_the_predicate_the_op_raises():
    x8 = torch.zeros((1, 2, 1, 8, 8), device=DEV)                                          # fp32 data: the layer keeps its torch path
    w, b = torch.zeros((8, 8, 5, 3), device=DEV), torch.zeros(8, device=DEV)
    assert not ops.causal_conv_relu_grad_supported(x8, w, b, 3, 2, 2) and not ops.causal_conv_relu_grad_supported(x8.to(BF), w, b, 3, 3, 3)
    with pytest.raises(RuntimeError, match="causal_conv_relu_grad_supported"):
        ops.causal_conv_relu_autograd(x8, w, b, 3, 2, 2)


# ---- module tier: 5.11's layer (H = 4, d = 64, T = 96, T_M = 32, bf16, sparse mode, fused_kd_loss, fused_tail_grad) ----------------
class _RefConvRelu(torch.autograd.Function):
    """the op in fp64 on the CPU, rounded to the data type at its edges"""

    @staticmethod
    def forward(ctx, x8, w, b, d):
        x, w3 = ops.from_c8(x8.detach()).double().cpu(), w.detach()[:, :, :3].double().cpu()
        y = torch.relu(F.conv2d(F.pad(x, (0, 0, 2 * d, 0)), w3, b.detach().double().cpu(), 1, (0, d), d))
        ctx.args, ctx.like = (x, w3, y, d), (x8, w, b)
        return ops.to_c8(y.to(x8.dtype).to(x8.device))

    @staticmethod
    def backward(ctx, g8):
        x, w3, y, d = ctx.args
        dx, dW3, db = _grads(x, w3, ops.from_c8(g8).double().cpu() * (y > 0), d)
        x8, w, b = ctx.like
        dW = torch.zeros_like(w)
        dW[:, :, :3] = dW3.to(w.dtype)
        return ops.to_c8(dx.to(x8.dtype).to(x8.device)), dW, db.to(b.dtype).to(b.device), None


@pytest.mark.gpu
def test_layer_switch_against_the_fp64_stand_in(monkeypatch):
    from test_gpu_predictor_tail_bwd import D_, _layer_and_inputs
    layer, x, mask, scores_truth = _layer_and_inputs(BF)
    att, lib, calls = layer.attention, _lib.load(), []
    assert att.fused_cnn_grad is False                                                     # off by default
    real = lib.sea_causal_conv_relu_bwd
    monkeypatch.setattr(lib, "sea_causal_conv_relu_bwd", lambda *a: calls.append(1) or real(*a))

    def step(cnn):
        att.fused_kd_loss, att.fused_tail_grad, att.fused_cnn_grad = True, True, cnn
        layer.zero_grad()
        try:
            q = x * D_ ** -0.5
            out = att(q, x.clone(), x.clone(), q, x.clone(), x.clone(), q, x.clone(), mask, scores_truth, None)
            out.loss.backward()
        finally:
            att.fused_kd_loss, att.fused_tail_grad, att.fused_cnn_grad = False, False, False
        torch.cuda.synchronize()
        return {"loss": out.loss.detach().clone(), **{n: p.grad.detach().clone() for n, p in att.named_parameters() if p.grad is not None}}
    yard = step(False)
    assert calls == []                                                                     # never with the switch off
    got = step(True)
    assert len(calls) == 2                                                                 # once per (conv, ReLU) pair per step
    with monkeypatch.context() as m:
        m.setattr(ops, "causal_conv_relu_autograd", lambda x8, w, b, k, d, pad: _RefConvRelu.apply(x8, w, b, d))
        ref = step(True)
    assert len(calls) == 2 and sorted(got) == sorted(yard) == sorted(ref)
    failures = []
    for n in got:
        r = ref[n].double().cpu()
        bar, err = bar_of(yard[n].double().cpu(), r), (got[n].double().cpu() - r).abs().max().item()
        print(f"[cnn-bwd] layer {n}: max err {err:.3e} bar {bar:.3e} ratio {err / max(bar, 1e-300):.3f} (max |ref| {r.abs().max().item():.3e})")
        if not (torch.isfinite(got[n]).all() and err <= bar):
            failures.append((n, err, bar))
    assert not failures, failures
