"""-m gpu: `ops.predictor_mlp_f32` (csrc/sea_mlp_f32.hip) and the layer switch `PerlinAttention.fused_mlp_fp32` against an fp64 CPU
evaluation of the same module chain on the fp32 inputs and parameters.  Yardstick: that chain in fp32 on the CPU; bar: `bar_of`."""
import copy
import functools

import pytest
import torch
from torch import nn

import sea_attention_amd as S
from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from test_gpu_context_grad import context_reference
from test_gpu_context_grad_layer import Cfg, H_, D_, T_, TM_, K_
from test_gpu_performer_bwd import _poisoned_rows          # NaN on both sides of every 16-byte aligned row
from test_performer_bwd_reference import bar_of

pytestmark = pytest.mark.gpu
DEV, F32, F64 = "cuda", torch.float32, torch.float64
D1, DIN = 128, 192
#        N  H   T   D2
CASES = [(1, 4, 1, 32),        # one token: a part-filled tile
         (2, 4, 37, 64),       # packed tiles, a tail, two batch items
         (1, 12, 21, 48),      # H % 16 != 0, Wd = 24
         (1, 16, 9, 128),      # whole-token tiles, all eight decoder column blocks
         (2, 32, 5, 128)]
NAMES = ("x_c8", "tpred", "row_scale", "avg_scale")


def _modules(D2, seed, d1=D1, din=DIN):
    """(enc Linear, enc LayerNorm, dec Linear, lnorm1, scaler Linear) on the CPU in fp32, every parameter random"""
    torch.manual_seed(seed)
    mods = (nn.Linear(din, d1), nn.LayerNorm(d1), nn.Linear(d1, D2), nn.LayerNorm(D2 // 2), nn.Linear(d1, 2))
    with torch.no_grad():
        for ln in (mods[1], mods[3]):
            ln.weight.copy_(1.0 + 0.3 * torch.randn_like(ln.weight))
            ln.bias.copy_(0.3 * torch.randn_like(ln.bias))
    return mods


def chain(x, mods, dt):
    """The module chain on the CPU in `dt`: (y (N, 2H, T, Wd) with channel 2 h + split, tpred, row_scale, avg_scale)"""
    enc, ln, dec, ln1, sc = (copy.deepcopy(m).cpu().to(dt) for m in mods)
    with torch.no_grad():
        tp = nn.functional.gelu(ln(enc(x.cpu().to(dt))))
        N, H, T, _ = tp.shape
        y = ln1(dec(tp).view(N, H, T, 2, -1)).permute(0, 1, 3, 2, 4).reshape(N, 2 * H, T, -1)
        g = torch.sigmoid(sc(tp))
    return y, tp, g[..., 0], g[..., 1]


@functools.lru_cache(maxsize=None)
def _case(idx):
    N, H, T, D2 = CASES[idx]
    mods = _modules(D2, 100 + idx)
    x = torch.randn((N, H, T, DIN), generator=torch.Generator().manual_seed(idx))
    return x, mods, [m.to(DEV) for m in copy.deepcopy(mods)], chain(x, mods, F64), chain(x, mods, F32)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["N%d-H%d-T%d-D2_%d" % c for c in CASES])
def test_op_holds_the_fp64_chain(idx):
    x, _mods, dev, ref, yard = _case(idx)
    xd = _poisoned_rows(x)
    assert not xd.is_contiguous() and ops.predictor_mlp_f32_supported(xd, *dev)
    x_c8, tpred, rs, avg = ops.predictor_mlp_f32(xd, *dev, want_tpred=True)
    got = (ops.from_c8(x_c8), tpred, rs, avg)
    for name, g, y, r in zip(NAMES, got, yard, ref):
        bar, err = bar_of(y, r), (g.double().cpu() - r).abs().max().item()
        print(f"[mlp-f32] {CASES[idx]} {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f} (max |ref| {r.abs().max().item():.3e})")
        assert g.shape == r.shape and torch.isfinite(g).all() and err <= bar, (name, err, bar)
    again = ops.predictor_mlp_f32(xd, *dev, want_tpred=True)                   # no atomics: the same bits
    lean = ops.predictor_mlp_f32(xd, *dev)                                     # tpred not stored: the other three unchanged
    assert lean[1] is None and torch.equal(again[1], tpred)
    for i in (0, 2, 3):
        assert torch.equal(again[i], (x_c8, tpred, rs, avg)[i]) and torch.equal(lean[i], (x_c8, tpred, rs, avg)[i])


def test_op_raises_outside_the_predicate():
    dev = [m.to(DEV) for m in _modules(32, 7, d1=160, din=240)]
    x = torch.randn((1, 4, 3, 240), device=DEV)
    assert not ops.predictor_mlp_f32_supported(x, *dev)
    with pytest.raises(RuntimeError, match="predictor_mlp_f32_supported"):
        ops.predictor_mlp_f32(x, *dev)


# ---- the layer: one fp32 PerlinSelfAttention, H = 4, d = 64, T = 96, T_M = 32, sparse mode (the module tier's shape) --------------------
@functools.lru_cache(maxsize=None)
def _layer_runs():
    """(out with the switch off, out with it on, calls of the entry in each, Linear calls in the on run, the MLP's input)"""
    S.seed(42)
    pc = PerlinAttentionConfig(k=K_, attention_predictor_length=TM_, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix')
    layer = PerlinSelfAttention(Cfg(), pc).to(DEV).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = True                                              # sparse mode
    att = layer.attention
    S.seed(1)
    with torch.no_grad():
        for ln in (att.attention_predictor_enc[1], att.attention_predictor_cnn[0].module):
            ln.weight.copy_(1.0 + 0.3 * torch.randn_like(ln.weight))
            ln.bias.copy_(0.3 * torch.randn_like(ln.bias))
    x = torch.randn((1, H_, T_, D_), device=DEV)
    idx = torch.arange(T_, device=DEV)
    mask = ((idx.view(1, T_) > idx.view(T_, 1)) * (torch.finfo(torch.float16).min / 2)).view(1, 1, T_, T_).float()
    q, k, v = x * D_ ** -0.5, x.clone(), 1.0 + 0.5 * torch.randn((1, H_, T_, D_), device=DEV)
    assert att.fused_mlp_fp32 is False                                         # off by default
    lib, calls, linears, seen, outs = _lib.load(), [0], [], [], []
    mlp_linears = {id(att.attention_predictor_enc[0]), id(att.attention_predictor_dec_row[0]), id(att.attention_predictor_dec_scaler[0])}
    real_entry, real_op, real_linear = lib.sea_predictor_mlp_f32, ops.predictor_mlp_f32, nn.Linear.forward
    with pytest.MonkeyPatch.context() as m:
        m.setattr(lib, "sea_predictor_mlp_f32", lambda *a: calls.__setitem__(0, calls[0] + 1) or real_entry(*a))
        m.setattr(ops, "predictor_mlp_f32", lambda x_, *a, **kw: seen.append(x_) or real_op(x_, *a, **kw))
        m.setattr(nn.Linear, "forward", lambda self, t: (linears.append(id(self)) if id(self) in mlp_linears else None) or real_linear(self, t))
        for switch in (False, True):
            att.fused_mlp_fp32 = switch
            before = (calls[0], len(linears))
            try:
                with torch.no_grad():
                    out = att(q, k, v, q, k, v, q, k, mask, None, None)
            finally:
                att.fused_mlp_fp32 = False
            torch.cuda.synchronize()
            outs.append((out, calls[0] - before[0], len(linears) - before[1]))
    return att, (q, k, v), outs[0], outs[1], seen


def test_layer_takes_the_launch_and_holds_the_fp64_chain():
    """Switch off: the entry never runs.  Switch on: once, and none of the MLP's torch Linears.  The fp64 chain: the MLP's input as the
    layer handed it over (the Performer's output, the same bits in both runs), the torch modules of the MLP and the CNN in fp64 on
    the CPU, softmax; the context branch in fp64 (`context_reference`) on the selection, with the gates of that chain.  The selection
    of the two runs must be EQUAL (stricter than a count of near-tie pixels)."""
    att, (q, k, v), (off, entry_off, lin_off), (on, entry_on, lin_on), seen = _layer_runs()
    assert entry_off == 0 and lin_off >= 2                                     # today's path: the torch Linears
    assert (entry_on, lin_on) == (1, 0) and len(seen) == 1 and seen[0].dtype == F32
    mods = (att.attention_predictor_enc[0], att.attention_predictor_enc[1], att.attention_predictor_dec_row[0],
            att.attention_predictor_cnn[0].module, att.attention_predictor_dec_scaler[0])
    _y, tp64, rs64, mix64 = chain(seen[0], mods, F64)
    with torch.no_grad():
        cnn64 = copy.deepcopy(att.attention_predictor_cnn).cpu().double()
        dec64 = copy.deepcopy(att.attention_predictor_dec_row).cpu().double()
        probs64 = torch.softmax(cnn64(dec64(tp64)), -1)
    dense, dense_off = ((ops.flat_csr_to_dense(o.partial_attention_mask, T_, H_) > 0).cpu() for o in (on, off))
    assert torch.equal(dense, dense_off) and dense.any()
    ctx64 = context_reference(q.double().cpu(), k.double().cpu(), v.double().cpu(), dense, rs64, mix64, F32)[0]
    for name, g, y, r in (("estimated_attention_probs", on.estimated_attention_probs, off.estimated_attention_probs, probs64),
                          ("context_layer", on.context_layer, off.context_layer, ctx64)):
        g, y = ops.realize(g).double().cpu(), ops.realize(y).double().cpu()
        bar, err = bar_of(y, r), (g - r).abs().max().item()
        print(f"[mlp-f32] layer {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f} (max |ref| {r.abs().max().item():.3e})")
        assert g.shape == r.shape and torch.isfinite(g).all() and err <= bar, (name, err, bar)
