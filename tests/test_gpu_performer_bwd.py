"""The causal Performer's backward on the HIP kernels (csrc/sea_performer_bwd.hip, ops.performer_value_autograd) and the layer
switch `PerlinAttention.fused_performer_grad`, DESIGN 5.10.

Op tier.  Reference: `PerformerReference` (test_performer_bwd_reference.py) in fp64 on the rounded inputs.  Yardstick: `performer.py`
under fp32 autograd on the CPU (`chunk=T`), its gradients cast to the output dtype.  Bar per case and quantity: 4 x the yardstick's
largest error, at least 2^-22 of the reference's largest magnitude (5.7's rule); it never comes from the kernel's output.  Rows of
q (k) with a feature inside four fp32 worst-case errors of the ReLU's kink are left out of the dq (dk) comparison, for the yardstick
as for the kernel; at most 3 % of a case's rows, asserted before the kernel is looked at.  q and k are drawn at 0.05 of unit scale:
the ReLU part of a feature is then of the order of 1e-2 and the 1e-3 every feature carries -- what a padded feature or a padded
row must NOT carry -- weighs in every sum.

Module tier.  One bf16 layer (projection buffer included), sparse mode, `fused_kd_loss`, a teacher score tensor and no context
truth: the loss is the estimator term, a continuous function of the Performer's output."""
import functools

import pytest
import torch

import sea_attention_amd as S
from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from sea_attention_amd.perlin_attention.ops import performer_grad
from test_performer_bwd_reference import PerformerReference, ambiguous_rows, bar_of, make_inputs, performer_py

DEV = "cuda"
F32, F16, BF = torch.float32, torch.float16, torch.bfloat16
F64 = torch.float64
QK_SCALE = 0.05
#        N  H  T     D   nb  dtype seed
CASES = [(1, 2, 65, 64, 33, BF, 11), (2, 3, 200, 64, 33, BF, 12), (1, 2, 130, 64, 80, BF, 13), (1, 1, 300, 64, 17, F16, 14),
         (1, 1, 150, 64, 33, F32, 15), (1, 1, 1100, 64, 33, F32, 16)]
WIDE = [(1, 2, 97, 80, 43, F16, 17), (1, 2, 70, 128, 77, BF, 18)]         # in the cases where the predicate allows: it does not yet
NAMES = ("dq", "dk", "dv", "dpos")


def _id(c):
    return "N%d-H%d-T%d-D%d-nb%d-%s" % (*c[:5], str(c[5]).split(".")[1])


@functools.lru_cache(maxsize=None)
def _case(idx, cases="CASES"):
    """Inputs (dtype values on the CPU), the fp64 reference, the fp32 yardstick, the rows left out of dq / dk, the bars."""
    N, H, T, D, nb, dt, seed = (CASES if cases == "CASES" else WIDE)[idx]
    inp = make_inputs(N, H, T, D, nb, seed, dtype=dt, qk_scale=QK_SCALE)
    q, k, v, pos, W, g = inp
    ref = PerformerReference(64).backward(*inp)
    yard = [y.to(dt) for y in performer_py(*(t.float() for t in inp), F32)[1:]]
    amb = (ambiguous_rows(q, W), ambiguous_rows(k, W))
    for a in amb:                                                              # on the reference side, before any kernel
        assert a.float().mean().item() <= 0.03, a.float().mean().item()
    bars = [bar_of(_kept(y, i, amb), _kept(r, i, amb)) for i, (y, r) in enumerate(zip(yard, ref))]
    return inp, ref, yard, amb, bars


def _kept(x, i, amb):
    """x without the rows whose ReLU side fp32 cannot tell (dq: i = 0, dk: i = 1), as fp64"""
    x = x.to(F64)
    return x[~amb[i]] if i < 2 else x


def _poisoned_rows(x):
    """an (N,H,T,D) view of an (N,T,H,D + 16) buffer: NaN on both sides of every row, rows 16-byte aligned"""
    N, H, T, D = x.shape
    buf = torch.full((N, T, H, D + 16), float("nan"), dtype=x.dtype, device=DEV)
    buf[..., 8:8 + D] = x.permute(0, 2, 1, 3).to(DEV)
    return buf[..., 8:8 + D].permute(0, 2, 1, 3).detach()


def _device_inputs(inp, need=(True, True, True, True)):
    q, k, v, pos, W, g = inp
    qd, kd, vd = (_poisoned_rows(t).requires_grad_(n) for t, n in zip((q, k, v), need))
    pbuf = torch.full((pos.shape[0], pos.shape[1] + 16), float("nan"), dtype=pos.dtype, device=DEV)
    pbuf[:, 8:8 + pos.shape[1]] = pos.to(DEV)
    pd = pbuf[:, 8:8 + pos.shape[1]].detach().requires_grad_(need[3])
    assert not qd.is_contiguous() and qd.stride(-1) == 1 and pd.stride(0) == pos.shape[1] + 16
    return qd, kd, vd, pd, W.float().to(DEV), g.to(DEV)


def _kernel_grads(inp, g_dev=None):
    qd, kd, vd, pd, Wd, gd = _device_inputs(inp)
    out = ops.performer_value_autograd(qd, kd, vd, pd, Wd)
    grads = torch.autograd.grad(out, [qd, kd, vd, pd], grad_outputs=gd if g_dev is None else g_dev)
    torch.cuda.synchronize()
    return out.detach(), grads


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_kernel_against_fp64_reference(idx):
    N, H, T, D, nb, dt, _seed = CASES[idx]
    inp, ref, yard, amb, bars = _case(idx)
    out, got = _kernel_grads(inp)
    ref_out = PerformerReference(64).forward(*inp[:5])
    assert (out.double().cpu() - ref_out).abs().max() <= 2.0 ** -7 * ref_out.abs().max()        # the forward launch, loosely
    failures = []
    for i, name in enumerate(NAMES):
        x = got[i].cpu()
        assert x.dtype == dt and x.shape == inp[(0, 1, 2, 3)[i]].shape and torch.isfinite(x).all(), name
        err = (_kept(x, i, amb) - _kept(ref[i], i, amb)).abs().max().item()
        print(f"[perf-bwd] {_id(CASES[idx])} {name}: max err {err:.3e} bar {bars[i]:.3e} ratio {err / bars[i]:.3f}"
              f" (max |ref| {ref[i].abs().max().item():.3e}, left out {int(amb[i].sum()) if i < 2 else 0} rows)")
        if not err <= bars[i]:
            failures.append((name, err, bars[i]))
    assert not failures, failures
    assert (got[3][T:] == 0).all() and got[3].shape[0] == T + 3                # rows of pos the forward never read
    _out2, again = _kernel_grads(inp)                                         # no atomics, one order: the same bits
    for a, b in zip(got, again):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(WIDE)), ids=[_id(c) for c in WIDE])
def test_head_sizes_without_a_backward_kernel_are_refused_not_emulated(idx):
    """D = 80 / 128: the state does not fit the LDS beside the chunk tiles in this plan; the predicate says so on
    both sides of the ABI, the op raises, and the layer keeps its torch path."""
    N, H, T, D, nb, dt, seed = WIDE[idx]
    qd, kd, vd, pd, Wd, _gd = _device_inputs(make_inputs(N, H, T, D, nb, seed, dtype=dt, qk_scale=QK_SCALE))
    assert _lib.load().sea_performer_causal_bwd_supported(D, nb, _lib.dtype_code(dt)) == 0
    assert not ops.performer_value_grad_supported(qd, kd, vd, pd, Wd)
    with pytest.raises(RuntimeError, match="performer_value_grad_supported"):
        ops.performer_value_autograd(qd, kd, vd, pd, Wd)


@pytest.mark.gpu
def test_saves_the_five_inputs_returns_none_where_no_gradient_is_wanted_and_takes_any_grad_layout():
    inp = _case(0)[0]
    N, H, T, D = inp[0].shape
    qd, kd, vd, pd, Wd, gd = _device_inputs(inp)
    packed = []

    def pack(t):
        packed.append(t)
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = ops.performer_value_autograd(qd, kd, vd, pd, Wd)
    assert len(packed) == 5
    for t, src in zip(packed[:4], (qd, kd, vd, pd)):
        assert t.data_ptr() == src.data_ptr() and t.shape == src.shape and t.stride() == src.stride()
    assert packed[4].dtype == F32 and packed[4].shape == Wd.shape and torch.equal(packed[4], Wd.to(inp[0].dtype).float())
    base = torch.autograd.grad(out, [qd, kd, vd, pd], grad_outputs=gd)

    # a grad_out that is a permuted view: made contiguous inside, the same bits
    g_view = gd.permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not g_view.is_contiguous()
    _o, strided = _kernel_grads(inp, g_dev=g_view)
    for a, b in zip(base, strided):
        assert torch.equal(a, b)

    # the Function's own return values: None for every input that wants no gradient
    class Ctx:
        saved_tensors = tuple(packed)
    for need in ((True, False, False, False), (False, True, False, True), (False, False, True, False)):
        Ctx.needs_input_grad = (*need, False, False)
        res = performer_grad._PerformerValueFn.backward(Ctx, gd)
        assert len(res) == 6 and res[4] is None and res[5] is None
        for r, n, b in zip(res[:4], need, base):
            assert (r is None) == (not n) and (r is None or torch.equal(r, b))
    Ctx.needs_input_grad = (False,) * 6
    assert all(r is None for r in performer_grad._PerformerValueFn.backward(Ctx, gd))
    # and through autograd: only q wants one
    q1, k1, v1, p1, _W, _g = _device_inputs(inp, need=(True, False, False, False))
    ops.performer_value_autograd(q1, k1, v1, p1, Wd).backward(gd)
    assert torch.equal(q1.grad, base[0]) and k1.grad is None and v1.grad is None and p1.grad is None


@pytest.mark.gpu
def test_one_row():
    """T = 1: ctx = V_0 whatever q and k are (up to the 1e-6 of the denominator), so dv = g[D:2D] + g[2D:], dpos = sum over the heads
    of g[:D], both to the rounding of the output type, and dq = dk = 0: fp32 cancellation of O(|g|) terms leaves about 1e-7 |g|, a
    missing denominator term about 0.1 |g|."""
    D = 64
    inp = make_inputs(1, 2, 1, D, 33, seed=21, dtype=BF)                       # unit scale: 1e-6 sum(a) / (a . b) is below 1e-6
    g = inp[5].double()
    _out, (dq, dk, dv, dpos) = _kernel_grads(inp)
    want_v = g[..., D:2 * D] + g[..., 2 * D:]
    want_p = g[..., :D].sum((0, 1))
    assert ((dv.double().cpu() - want_v).abs() <= 2.0 ** -8 * want_v.abs() + 1e-30).all()
    assert ((dpos[:1].double().cpu() - want_p).abs() <= 2.0 ** -8 * want_p.abs() + 1e-30).all() and (dpos[1:] == 0).all()
    lim = 1e-4 * g.abs().max().item()
    assert dq.abs().max().item() <= lim and dk.abs().max().item() <= lim, (dq.abs().max().item(), dk.abs().max().item(), lim)


@pytest.mark.parametrize("fault", ("carry", "padded-feature"))
def test_witnesses_exceed_ten_bars(fault):
    """On the CPU: a reference with one of the two faults the kernels must not have, held to the same bars as the kernels."""
    idx = 4                                                                    # (1,1,150,64,33,fp32): 3 chunks, 15 padded features
    inp, ref, _yard, amb, bars = _case(idx)
    bad = PerformerReference(64, drop_carry_at=1) if fault == "carry" else PerformerReference(64, leak_padded_features=True)
    got = bad.backward(*inp)
    ratios = [(_kept(x, i, amb) - _kept(r, i, amb)).abs().max().item() / bars[i] for i, (x, r) in enumerate(zip(got, ref))]
    print(f"[perf-bwd] witness {fault}: err / bar " + " ".join(f"{n} {r:.1f}" for n, r in zip(NAMES, ratios)))
    assert max(ratios) > 10, ratios


# ---- module tier -------------------------------------------------------------------------------------------------------
class Cfg:
    def __init__(self, hidden, heads, max_pos):
        self.hidden_size, self.num_attention_heads, self.max_position_embeddings = hidden, heads, max_pos


H_, D_, T_, TM_, K_ = 4, 64, 96, 32, 8


@pytest.fixture(scope="module")
def layer_and_inputs():
    S.seed(42)
    pc = PerlinAttentionConfig(k=K_, attention_predictor_length=TM_, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix')
    # .to(bf16) rounds the projection buffer as well: the torch path and the kernels then see the same projection
    layer = PerlinSelfAttention(Cfg(H_ * D_, H_, T_), pc).to(DEV).to(BF).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = True                                              # sparse mode
    S.seed(1)
    x = torch.randn((1, H_, T_, D_), device=DEV).to(BF)
    fp_min = torch.finfo(torch.float16).min / 2
    idx = torch.arange(T_, device=DEV)
    mask = ((idx.view(1, T_) > idx.view(T_, 1)) * fp_min).view(1, 1, T_, T_).to(BF)
    scores_truth = (torch.randn((1, H_, T_, T_), device=DEV) * 2.0).to(BF)
    return layer, x, mask, scores_truth


def _step(layer_and_inputs, switch):
    """One training step of `PerlinAttention.forward`, called directly: (loss, {parameter name: gradient})"""
    layer, x, mask, scores_truth = layer_and_inputs
    att = layer.attention
    q, k, v = x * D_ ** -0.5, x.clone(), x.clone()
    att.fused_kd_loss, att.fused_performer_grad = True, switch
    layer.zero_grad()
    try:
        out = att(q, k, v, q, k, v, q, k, mask, scores_truth, None)
        out.loss.backward()
    finally:
        att.fused_kd_loss, att.fused_performer_grad = False, False
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in att.named_parameters() if p.grad is not None}
    return out.loss.detach().clone(), grads


def _counting(monkeypatch):
    lib, calls = _lib.load(), []
    real = lib.sea_performer_causal_bwd

    def spy(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(lib, "sea_performer_causal_bwd", spy)
    return calls


def _torch_stand_in(att):
    """What `_estimate` does with the switch off, behind the new op's name: the module's own FastAttention and the two
    concatenations"""
    def f(q, k, v, pos, projection, n_segments=None):
        vfa = torch.cat([pos.view(1, 1, *pos.shape).expand(v.shape).to(v.dtype), v], dim=-1)
        ctx = att.performer(q.float(), k.float(), vfa.float()).to(q.dtype)
        return torch.cat([ctx, v], dim=-1)
    return f


class _RefPerformer(torch.autograd.Function):
    """`PerformerReference`: fp64 inside, rounded to the data type at its edges"""

    @staticmethod
    def forward(ctx, q, k, v, pos, projection):
        args = tuple(t.detach().cpu() for t in (q, k, v, pos, projection.to(q.dtype)))
        ctx.args, ctx.like, ctx.pos_like = args, q, pos
        return PerformerReference(64).forward(*args).to(q.dtype).to(q.device)

    @staticmethod
    def backward(ctx, g):
        dq, dk, dv, dpos = PerformerReference(64).backward(*ctx.args, g.detach().cpu())
        to = lambda t, like: t.to(like.dtype).to(like.device)
        return to(dq, ctx.like), to(dk, ctx.like), to(dv, ctx.like), to(dpos, ctx.pos_like), None


@pytest.mark.gpu
def test_layer_wiring_is_bitwise_the_torch_path_behind_the_switch(layer_and_inputs, monkeypatch):
    att = layer_and_inputs[0].attention
    assert att.fused_performer_grad is False                                   # off by default
    calls = _counting(monkeypatch)
    loss_off, g_off = _step(layer_and_inputs, False)
    assert calls == [] and loss_off.item() > 0                                 # with the switch off the HIP backward never runs
    seen = []
    stand_in = _torch_stand_in(att)

    def spy(*a, **kw):
        seen.append(a)
        return stand_in(*a, **kw)
    with monkeypatch.context() as m:
        m.setattr(ops, "performer_value_autograd", spy)
        loss_on, g_on = _step(layer_and_inputs, True)
    assert len(seen) == 1 and seen[0][0].shape == (1, H_, T_, D_) and seen[0][3].shape == (T_, D_) and calls == []
    assert torch.equal(loss_on, loss_off) and sorted(g_on) == sorted(g_off)
    for n in g_off:
        assert torch.equal(g_on[n], g_off[n]), n
    assert "v_eye_learned_causal" in g_off and g_off["v_eye_learned_causal"].abs().max().item() > 0


@pytest.mark.gpu
def test_layer_numbers_against_the_fp64_performer(layer_and_inputs, monkeypatch):
    calls = _counting(monkeypatch)
    loss_y, g_y = _step(layer_and_inputs, False)                               # the torch path: the yardstick
    assert calls == []
    loss_k, g_k = _step(layer_and_inputs, True)                                # the kernels
    assert len(calls) == 1                                                     # one HIP backward per step
    with monkeypatch.context() as m:
        m.setattr(ops, "performer_value_autograd",                             # fp64: the reference
                  lambda q, k, v, pos, projection, n_segments=None: _RefPerformer.apply(q, k, v, pos, projection))
        loss_r, g_r = _step(layer_and_inputs, True)
    assert len(calls) == 1
    held = [("loss", loss_k, loss_y, loss_r)]
    for n in ("v_eye_learned_causal", "attention_predictor_enc.0.weight"):
        held.append((f"d {n}", g_k[n], g_y[n], g_r[n]))
    failures = []
    for name, got, yard, ref in held:
        ref = ref.double().cpu()
        bar = bar_of(yard.double().cpu(), ref)
        err = (got.double().cpu() - ref).abs().max().item()
        print(f"[perf-bwd] layer {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f} (max |ref| {ref.abs().max().item():.3e})")
        assert torch.isfinite(got).all() and ref.abs().max().item() > 0
        if not err <= bar:
            failures.append((name, err, bar))
    assert not failures, failures
