"""The predictor MLP's backward on the HIP kernels (csrc/sea_mlp_bwd.hip, ops.predictor_mlp_autograd) and the layer switch
`PerlinAttention.fused_mlp_grad`, DESIGN 5.13.

Op tier.  Reference: fp64 autograd on the CPU of the plain chain (linear, layer_norm, gelu, linear, halves, layer_norm) on the rounded
inputs and parameters, no intermediate rounding.  Yardstick: the same chain in the data type under autograd on the device -- what the
layer runs with the switch off, with the forward's rounding points.  Bar per quantity: 4 x the yardstick's largest error, at least
2^-22 of the reference's largest magnitude (5.7's rule).  Module tier: 5.11's layer; reference an fp64 stand-in for the op, yardstick
the switch-off run."""
import functools
from types import SimpleNamespace

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import ops
from sea_attention_amd.perlin_attention.ops import predictor_mlp_grad
from test_predictor_tail_bwd_reference import bar_of

DEV = "cuda"
F16, BF, F64 = torch.float16, torch.bfloat16, torch.float64
EPS = 1e-5
NAMES = ("dx", "dW1", "db1", "dg1", "dbe1", "dW2", "db2", "dg2", "dbe2")


def wgrad_rows(rows):
    """rows of one weight-gradient block (csrc/sea_mlp_bwd.hip, mlp_bwd_wgrad_rows)"""
    return max(256, 32 * -(-rows // 8192))


#        N  H   T     Din  D2   dtype
CASES = [(1, 4, 1, 192, 16, BF),           # four rows in one partly empty tile; Wd = 8 inside a padded tile
         (2, 12, 3, 192, 48, F16),         # Wd = 24; 72 rows: tiles straddle tokens and batch items, a ragged last slab
         (2, 16, 5, 192, 128, BF),         # H % 16 == 0, Wd = 64; x a permuted view of (N, T, H, Din); no gradient of tpred
         (2, 8, None, 192, 64, BF),        # a second weight-gradient block of one token's rows: two parts, one ragged
         (1, 4, 2, 64, 32, F16)]           # Din = 64: two k-steps
STRIDED, NO_GTPRED = 2, 2


def _chain(x, p):
    """(y (N, 2H, T, Wd), tpred) of the module chain in the precision of the arguments"""
    N, H, T, _ = x.shape
    enc = F.gelu(F.layer_norm(F.linear(x, p[0], p[1]), (p[0].shape[0],), p[2], p[3], EPS))
    dec = F.linear(enc, p[4], p[5])
    Wd = dec.shape[-1] // 2
    y = F.layer_norm(dec.view(N, H, T, 2, Wd), (Wd,), p[6], p[7], EPS)
    return y.permute(0, 1, 3, 2, 4).reshape(N, 2 * H, T, Wd), enc


def _chain_grads(x, p, g_y, g_tp):
    with torch.enable_grad():
        x, p = x.detach().clone().requires_grad_(True), [t.detach().clone().requires_grad_(True) for t in p]
        y, enc = _chain(x, p)
        outs, gs = ([y], [g_y]) if g_tp is None else ([y, enc], [g_y, g_tp])
        return torch.autograd.grad(outs, [x, *p], grad_outputs=gs)


@functools.lru_cache(maxsize=None)
def _inputs(idx):
    N, H, T, Din, D2, dt = CASES[idx]
    T = T or next(t for t in range(1, 4096) if N * H * t > wgrad_rows(N * H * t))
    assert N * H * T >= 4
    gen = torch.Generator().manual_seed(70 + idx)
    rn = lambda *s: torch.randn(s, generator=gen)
    x = rn(N, T, H, Din).to(dt)                                                            # (case STRIDED hands this memory order over)
    p = [rn(128, Din) / Din ** 0.5, 0.1 * rn(128), 1 + 0.1 * rn(128), 0.1 * rn(128),
         rn(D2, 128) / 128 ** 0.5, 0.1 * rn(D2), 1 + 0.1 * rn(D2 // 2), 0.1 * rn(D2 // 2)]
    return x.permute(0, 2, 1, 3), [t.to(dt) for t in p], rn(N, 2 * H, T, D2 // 2).to(dt), rn(N, H, T, 128).to(dt)


def _modules(p, dt):
    Din, D2 = p[0].shape[1], p[4].shape[0]
    mods = (nn.Linear(Din, 128), nn.LayerNorm(128, eps=EPS), nn.Linear(128, D2), nn.LayerNorm(D2 // 2, eps=EPS), nn.Linear(128, 2))
    mods = [m.to(DEV).to(dt) for m in mods]
    with torch.no_grad():
        for q, v in zip([q for m in mods[:4] for q in (m.weight, m.bias)], p):
            q.copy_(v)
    return mods


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=["N%d-H%d-T%s-Din%d-D2_%d-%s" % (*c[:5], str(c[5]).split(".")[1]) for c in CASES])
def test_kernels_against_fp64_reference(idx):
    dt = CASES[idx][5]
    x, p, g_y, g_tp = _inputs(idx)
    g_tp = None if idx == NO_GTPRED else g_tp
    mods = _modules(p, dt)
    params = [q for m in mods[:4] for q in (m.weight, m.bias)]
    xd = (x.permute(0, 2, 1, 3).to(DEV).permute(0, 2, 1, 3) if idx == STRIDED else x.contiguous().to(DEV)).requires_grad_(True)
    assert xd.is_contiguous() == (idx != STRIDED)
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        y8, tpred = ops.predictor_mlp_autograd(xd, *mods)
    want8, want_tp = ops.predictor_mlp(xd.detach(), *mods, want_tpred=True)[:2]
    assert torch.equal(y8, want8) and torch.equal(tpred, want_tp)                          # the inference launch
    assert [t.data_ptr() for t in saved] == [t.data_ptr() for t in (xd, *params)]          # x and the eight parameters: nothing else
    outs, gs = ([y8], [ops.to_c8(g_y.to(DEV))]) if g_tp is None else ([y8, tpred], [ops.to_c8(g_y.to(DEV)), g_tp.to(DEV)])
    got = torch.autograd.grad(outs, [xd, *params], grad_outputs=gs, retain_graph=True)
    again = torch.autograd.grad(outs, [xd, *params], grad_outputs=gs, retain_graph=True)
    no_x = torch.autograd.grad(outs, params, grad_outputs=gs)
    torch.cuda.synchronize()
    ref = _chain_grads(x.double(), [t.double() for t in p], g_y.double(), None if g_tp is None else g_tp.double())
    yard = _chain_grads(xd, params, g_y.to(DEV), None if g_tp is None else g_tp.to(DEV))
    failures = []
    for name, v, r, yd in zip(NAMES, got, ref, yard):
        bar, err = bar_of(yd.cpu(), r), (v.double().cpu() - r).abs().max().item()
        print(f"[mlp-bwd] {tuple(x.shape)} D2={CASES[idx][4]} {dt} {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f} "
              f"(max |ref| {r.abs().max().item():.3e})")
        if not (v.dtype == dt and v.shape == r.shape and torch.isfinite(v).all() and err <= bar):
            failures.append((name, err, bar))
    assert not failures, failures
    assert all(torch.equal(a, b) for a, b in zip(got, again))                              # no atomics, one order: the same bits
    assert all(torch.equal(a, b) for a, b in zip(got[1:], no_x))
    # d_x = None when x needs no gradient

    ctx = SimpleNamespace(saved_tensors=tuple(saved), needs_input_grad=(False,) + (True,) * 8 + (False, False), mods=tuple(mods))
    res = predictor_mlp_grad._PredictorMlpFn.backward(ctx, gs[0], gs[1] if len(gs) > 1 else None)
    assert res[0] is None and res[9:] == (None, None) and all(torch.equal(a, b) for a, b in zip(res[1:9], got[1:]))


@pytest.mark.gpu
def test_fp32_parameters_under_bf16_data():
    """fp32 master weights: the modules stay fp32 and their values are such as bf16 cannot hold -- every value (1 + 2^-10) times a
    bf16 number, which rounds back to that number.  The forward is bitwise the forward of the rounded modules, the eight parameter
    gradients come back fp32, and every gradient is held to this file's fp64 reference on the rounded parameters under this file's
    bar (the yardstick: the rounded modules' chain in the data type)."""
    idx = 0
    dt = CASES[idx][5]
    x, p, g_y, g_tp = _inputs(idx)
    mods16 = _modules(p, dt)
    mods = _modules([t.float() * (1 + 2.0 ** -10) for t in p], torch.float32)
    params16 = [q for m in mods16[:4] for q in (m.weight, m.bias)]
    params = [q for m in mods[:4] for q in (m.weight, m.bias)]
    with torch.no_grad():
        for m, m16 in zip(mods[4:], mods16[4:]):                                           # (the gates' Linear: the same values)
            m.weight.copy_(m16.weight), m.bias.copy_(m16.bias)
    for q, q16 in zip(params, params16):
        assert dt == BF and q.dtype == torch.float32 and torch.equal(q.detach().to(BF), q16.detach())
        assert (q.detach() != q16.detach().float()).float().mean().item() > 0.99
    xd = x.contiguous().to(DEV).requires_grad_(True)
    y8, tpred = ops.predictor_mlp_autograd(xd, *mods)
    want8, want_tp = ops.predictor_mlp(xd.detach(), *mods16, want_tpred=True)[:2]
    assert torch.equal(y8, want8) and torch.equal(tpred, want_tp)
    got = torch.autograd.grad([y8, tpred], [xd, *params], grad_outputs=[ops.to_c8(g_y.to(DEV)), g_tp.to(DEV)])
    torch.cuda.synchronize()
    assert [v.dtype for v in got] == [BF] + [torch.float32] * 8
    ref = _chain_grads(x.double(), [t.double() for t in p], g_y.double(), g_tp.double())
    yard = _chain_grads(xd, params16, g_y.to(DEV), g_tp.to(DEV))
    failures = []
    for name, v, r, yd in zip(NAMES, got, ref, yard):
        bar, err = bar_of(yd.cpu(), r), (v.double().cpu() - r).abs().max().item()
        print(f"[mlp-bwd] {tuple(x.shape)} D2={CASES[idx][4]} fp32 parameters {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
        if not (v.shape == r.shape and torch.isfinite(v).all() and err <= bar):
            failures.append((name, err, bar))
    assert not failures, failures


@pytest.mark.gpu
def test_outside_the_predicate_the_op_raises():
    mods = _modules(_inputs(4)[1], BF)
    x = torch.zeros((1, 4, 2, 64), device=DEV)                                             # fp32 data: the layer keeps its torch path
    wide = (nn.Linear(64, 160).to(DEV).to(BF), nn.LayerNorm(160).to(DEV).to(BF), nn.Linear(160, 32).to(DEV).to(BF), mods[3],
            nn.Linear(160, 2).to(DEV).to(BF))
    assert not ops.predictor_mlp_grad_supported(x, *mods) and not ops.predictor_mlp_grad_supported(x.to(BF), *wide)
    for args in ((x, *mods), (x.to(BF), *wide)):
        with pytest.raises(RuntimeError, match="predictor_mlp_grad_supported"):
            ops.predictor_mlp_autograd(*args)


# ---- module tier: 5.11's layer (H = 4, d = 64, T = 96, T_M = 32, bf16, sparse mode), fused_kd_loss, fused_tail_grad, fused_cnn_grad ----
class _RefMlp(torch.autograd.Function):
    """the op in fp64 on the CPU, rounded to the data type at its edges"""

    @staticmethod
    def forward(ctx, x, *params):
        ctx.args = (x.detach().double().cpu(), [t.detach().double().cpu() for t in params])
        ctx.like = (x, *params)
        y, enc = _chain(*ctx.args)
        return ops.to_c8(y.to(x.dtype).to(x.device)), enc.to(x.dtype).to(x.device)

    @staticmethod
    def backward(ctx, g8, g_tp):
        grads = _chain_grads(*ctx.args, ops.from_c8(g8).double().cpu(), g_tp.double().cpu())
        return tuple(g.to(q.dtype).to(q.device) for g, q in zip(grads, ctx.like))


@pytest.mark.gpu
def test_layer_switch_against_the_fp64_stand_in(monkeypatch):
    from test_gpu_predictor_tail_bwd import D_, _layer_and_inputs
    layer, x, mask, scores_truth = _layer_and_inputs(BF)
    att, lib, calls = layer.attention, _lib.load(), []
    assert att.fused_mlp_grad is False                                                     # off by default
    real = lib.sea_predictor_mlp_bwd
    monkeypatch.setattr(lib, "sea_predictor_mlp_bwd", lambda *a: calls.append(1) or real(*a))

    def step(mlp):
        att.fused_kd_loss = att.fused_tail_grad = att.fused_cnn_grad = True
        att.fused_mlp_grad = mlp
        layer.zero_grad()
        try:
            q = x * D_ ** -0.5
            out = att(q, x.clone(), x.clone(), q, x.clone(), x.clone(), q, x.clone(), mask, scores_truth, None)
            out.loss.backward()
        finally:
            att.fused_kd_loss = att.fused_tail_grad = att.fused_cnn_grad = att.fused_mlp_grad = False
        torch.cuda.synchronize()
        return {"loss": out.loss.detach().clone(), **{n: p.grad.detach().clone() for n, p in att.named_parameters() if p.grad is not None}}
    yard = step(False)
    assert calls == []                                                                     # never with the switch off
    got = step(True)
    assert len(calls) == 1                                                                 # exactly once per step
    with monkeypatch.context() as m:
        m.setattr(ops, "predictor_mlp_autograd", lambda x_, e, ln, d, l1, sc, want_tpred=True: _RefMlp.apply(
            x_, e.weight, e.bias, ln.weight, ln.bias, d.weight, d.bias, l1.weight, l1.bias))
        ref = step(True)
    assert len(calls) == 1 and sorted(got) == sorted(yard) == sorted(ref)
    failures = []
    for n in got:
        r = ref[n].double().cpu()
        bar, err = bar_of(yard[n].double().cpu(), r), (got[n].double().cpu() - r).abs().max().item()
        print(f"[mlp-bwd] layer {n}: max err {err:.3e} bar {bar:.3e} ratio {err / max(bar, 1e-300):.3f} (max |ref| {r.abs().max().item():.3e})")
        if not (torch.isfinite(got[n]).all() and err <= bar):
            failures.append((n, err, bar))
    assert not failures, failures
