"""The causal Performer's backward for the head sizes 80 and 128 (csrc/sea_performer_bwd_wide.hip,
ops.performer_value_autograd_wide, and `PerlinAttention.fused_performer_grad` at those head sizes), DESIGN 5.10b.

Reference, yardstick, bar and the rule for rows at the ReLU's kink are those of test_gpu_performer_bwd.py: fp64
`PerformerReference` on the rounded inputs; `performer.py` under fp32 autograd on the CPU (`chunk=T`) cast to the data type;
`bar_of` = 4 x the yardstick's largest error, at least 2^-22 of the reference's largest magnitude; none comes from the kernel."""
import functools

import pytest
import torch

import sea_attention_amd as S
import test_gpu_performer_bwd as B
from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from test_performer_bwd_reference import PerformerReference, ambiguous_rows, bar_of, make_inputs, performer_py

DEV = "cuda"
F32, F16, BF = torch.float32, torch.float16, torch.bfloat16
QK_SCALE = 0.05
#        N  H  T    D    nb  dtype seed      one chunk + one row; a partial last chunk after 2, 4 and 9 boundaries; padded features at
CASES = [(1, 2, 97, 80, 43, F16, 17), (1, 2, 70, 128, 77, BF, 18), (2, 2, 33, 128, 77, F32, 19), (1, 1, 130, 80, 43, F32, 20),
         (1, 1, 300, 128, 33, F16, 22)]     # NBT 3 and 5; N H > 1 for the dpos order; the three dtypes and both head sizes
NAMES = ("dq", "dk", "dv", "dpos")
_id = B._id


@functools.lru_cache(maxsize=None)
def _case(idx):
    """Inputs (dtype values on the CPU), the fp64 reference, the rows left out of dq / dk, the bars"""
    N, H, T, D, nb, dt, seed = CASES[idx]
    inp = make_inputs(N, H, T, D, nb, seed, dtype=dt, qk_scale=QK_SCALE)
    ref = PerformerReference(32).backward(*inp)
    yard = [y.to(dt) for y in performer_py(*(t.float() for t in inp), F32)[1:]]
    amb = (ambiguous_rows(inp[0], inp[4]), ambiguous_rows(inp[1], inp[4]))
    for a in amb:                                                              # on the reference side, before any kernel
        assert a.float().mean().item() <= 0.03, a.float().mean().item()
    return inp, ref, amb, [bar_of(B._kept(y, i, amb), B._kept(r, i, amb)) for i, (y, r) in enumerate(zip(yard, ref))]


def _kernel_grads(inp):
    qd, kd, vd, pd, Wd, gd = B._device_inputs(inp)
    assert ops.performer_value_grad_wide_supported(qd, kd, vd, pd, Wd)
    out = ops.performer_value_autograd_wide(qd, kd, vd, pd, Wd)
    grads = torch.autograd.grad(out, [qd, kd, vd, pd], grad_outputs=gd)
    torch.cuda.synchronize()
    return out.detach(), grads


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_kernel_against_fp64_reference(idx):
    N, H, T, D, nb, dt, _seed = CASES[idx]
    inp, ref, amb, bars = _case(idx)
    out, got = _kernel_grads(inp)
    ref_out = PerformerReference(32).forward(*inp[:5])
    assert (out.double().cpu() - ref_out).abs().max() <= 2.0 ** -7 * ref_out.abs().max()        # the forward launch, loosely
    failures = []
    for i, name in enumerate(NAMES):
        x = got[i].cpu()
        assert x.dtype == dt and x.shape == inp[i].shape and torch.isfinite(x).all(), name
        err = (B._kept(x, i, amb) - B._kept(ref[i], i, amb)).abs().max().item()
        print(f"[perf-bwd-wide] {_id(CASES[idx])} {name}: max err {err:.3e} bar {bars[i]:.3e} ratio {err / bars[i]:.3f}"
              f" (max |ref| {ref[i].abs().max().item():.3e}, left out {int(amb[i].sum()) if i < 2 else 0} rows)")
        if not err <= bars[i]:
            failures.append((name, err, bars[i]))
    assert not failures, failures
    assert (got[3][T:] == 0).all() and got[3].shape[0] == T + 3                # rows of pos the forward never read
    _out2, again = _kernel_grads(inp)                                         # no atomics, one order: the same bits
    for a, b in zip(got, again):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_one_row():
    """T = 1: ctx = V_0 whatever q and k are (up to the 1e-6 of the denominator), so dv = g[D:2D] + g[2D:], dpos = sum over the heads
    of g[:D], both to one unit of bf16, and dq = dk = 0 up to fp32 cancellation (DESIGN 5.10's closed form).

    Where the terms of the closed form cancel (this seed has g[D + j] = -g[2D + j] exactly for one j: the closed form says 0, the
    exact gradient is -6e-7 g) one bf16 unit of the closed form is smaller than the closed form's own error.  So on top of the unit
    stand that error, |fp64 reference - closed form|, and the fp32 worst case of the ctx part, (a . b) (g / den): two nb-term dot
    products and two roundings, (nb + 2) 2^-23 of the terms' magnitude.  Both are 1e-5 of |g| and vanish beside the unit elsewhere."""
    D, nb = 128, 77
    inp = make_inputs(1, 3, 1, D, nb, seed=21, dtype=BF)
    g = inp[5].double()
    ref = PerformerReference(32).backward(*inp)
    _out, (dq, dk, dv, dpos) = _kernel_grads(inp)
    want_v = g[..., D:2 * D] + g[..., 2 * D:]
    want_p = g[..., :D].sum((0, 1))
    fp32 = (nb + 2) * 2.0 ** -23
    tol_v = 2.0 ** -8 * want_v.abs() + (ref[2] - want_v).abs() + fp32 * g[..., D:2 * D].abs()
    tol_p = 2.0 ** -8 * want_p.abs() + (ref[3][:1] - want_p).abs() + fp32 * g[..., :D].abs().sum((0, 1))
    assert ((dv.double().cpu() - want_v).abs() <= tol_v).all()
    assert ((dpos[:1].double().cpu() - want_p).abs() <= tol_p).all() and (dpos[1:] == 0).all()
    lim = 1e-4 * g.abs().max().item()
    assert dq.abs().max().item() <= lim and dk.abs().max().item() <= lim, (dq.abs().max().item(), dk.abs().max().item(), lim)


@pytest.mark.gpu
def test_layer_takes_the_wide_op_under_the_switch_and_only_there(monkeypatch):
    """d = 128, bf16, sparse mode, `fused_kd_loss`, a teacher: the module tier of test_gpu_performer_bwd.py at a wide head"""
    H_, D_, T_, TM_ = 4, 128, 96, 32
    S.seed(42)
    pc = PerlinAttentionConfig(k=8, attention_predictor_length=TM_, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix')
    layer = PerlinSelfAttention(B.Cfg(H_ * D_, H_, T_), pc).to(DEV).to(BF).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = True                                              # sparse mode
    S.seed(1)
    x = torch.randn((1, H_, T_, D_), device=DEV).to(BF)
    idx = torch.arange(T_, device=DEV)
    mask = ((idx.view(1, T_) > idx.view(T_, 1)) * (torch.finfo(torch.float16).min / 2)).view(1, 1, T_, T_).to(BF)
    setup = (layer, x, mask, (torch.randn((1, H_, T_, T_), device=DEV) * 2.0).to(BF))
    att, lib, calls = layer.attention, _lib.load(), []
    real = lib.sea_performer_causal_bwd_wide
    monkeypatch.setattr(lib, "sea_performer_causal_bwd_wide", lambda *a: calls.append(1) or real(*a))

    loss_y, g_y = B._step(setup, False)                                        # the torch modules: the yardstick
    assert calls == [] and loss_y.item() > 0
    with monkeypatch.context() as m:                                           # switch off: bitwise the torch modules behind the op's name
        m.setattr(ops, "performer_value_autograd_wide", B._torch_stand_in(att))
        loss_s, g_s = B._step(setup, True)
    assert calls == [] and torch.equal(loss_s, loss_y) and all(torch.equal(g_s[n], g_y[n]) for n in g_y)
    loss_k, g_k = B._step(setup, True)                                         # the kernels
    assert len(calls) == 1                                                     # one HIP backward per step
    with monkeypatch.context() as m:                                           # fp64: the reference
        m.setattr(ops, "performer_value_autograd_wide",
                  lambda q, k, v, pos, projection, n_segments=None: B._RefPerformer.apply(q, k, v, pos, projection))
        loss_r, g_r = B._step(setup, True)
    assert len(calls) == 1
    failures = []
    for name, got, yard, ref in [("loss", loss_k, loss_y, loss_r)] + [
            (f"d {n}", g_k[n], g_y[n], g_r[n]) for n in ("v_eye_learned_causal", "attention_predictor_enc.0.weight")]:
        ref = ref.double().cpu()
        bar = bar_of(yard.double().cpu(), ref)
        err = (got.double().cpu() - ref).abs().max().item()
        print(f"[perf-bwd-wide] layer {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f} (max |ref| {ref.abs().max().item():.3e})")
        assert torch.isfinite(got).all() and ref.abs().max().item() > 0
        if not err <= bar:
            failures.append((name, err, bar))
    assert not failures, failures
