"""The predictor tail's backward on the HIP kernel (csrc/sea_tail_bwd.hip, ops.predictor_tail_autograd) and the layer switch
`PerlinAttention.fused_tail_grad`, DESIGN 5.11.

Op tier.  Reference: `TailReference` (test_predictor_tail_bwd_reference.py) in fp64 on the rounded inputs.  Yardstick: the module
chain under fp32 autograd on the CPU, its gradients cast to the output dtype.  Bar per case and quantity: 4 x the yardstick's largest
error, at least 2^-22 of the reference's largest magnitude (5.7's rule); it never comes from the kernel's output.  y = relu(randn),
handed over as a view with NaN on both sides of every row.

Module tier.  One layer, sparse mode, `fused_kd_loss`, a teacher score tensor and no context truth: the loss is the estimator term,
a continuous function of the tail's scores."""
import functools

import pytest
import torch

import sea_attention_amd as S
from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from sea_attention_amd.perlin_attention.modules import interpolate
from sea_attention_amd.perlin_attention.ops import predictor_tail_grad
from test_predictor_tail_bwd_reference import EPS, TailReference, bar_of, block_rows, make_inputs, tail_torch

DEV = "cuda"
F32, F16, BF = torch.float32, torch.float16, torch.bfloat16
F64 = torch.float64
#        N  H   T    T_M  dtype layout  seed
CASES = [(1, 12, 5, 64, BF, "nchw", 31),        # H, C not multiples of 16; fewer rows than a block
         (2, 32, 37, 256, BF, "nhwc", 32),      # channels-last strides
         (1, 16, 130, 96, F16, "nchw", 33),     # W4 = 24, partial lanes
         (1, 40, 9, 128, F32, "nchw", 34),      # C = 80
         (1, 4, 1, 64, F32, "nchw", 35),        # one row
         (3, 8, 700, 64, BF, "nchw", 36)]       # many blocks and a ragged last one
NAMES = ("dy", "dW", "dgamma", "dbeta")
MODES = ("g_s", "g_p", "both")


def _id(c):
    return "N%d-H%d-T%d-TM%d-%s-%s" % (*c[:4], str(c[4]).split(".")[1], c[5])


def _pick(inp, mode):
    return (inp[5] if mode != "g_p" else None), (inp[6] if mode != "g_s" else None)


@functools.lru_cache(maxsize=None)
def _case(idx, mode="both"):
    """Inputs (dtype values on the CPU), the fp64 reference (dy, dW, dgamma, dbeta), the bars from the fp32 yardstick."""
    N, H, T, T_m, dt, _layout, seed = CASES[idx]
    inp = make_inputs(N, H, T, T_m, seed, dtype=dt)
    g_s, g_p = _pick(inp, mode)
    dy, dW, _db, dga, dbe = TailReference().backward(*inp[:5], EPS, g_s, g_p)
    ref = (dy, dW, dga, dbe)
    f = lambda t: None if t is None else t.float()
    yd = tail_torch(*(t.float() for t in inp[:5]), EPS, f(g_s), f(g_p), F32)
    yard = [yd[i].to(dt) for i in (0, 1, 3, 4)]
    bars = [bar_of(y, r) for y, r in zip(yard, ref)]
    return inp, ref, bars


def _poisoned(y, layout):
    """y (N,C,T,W4) as a view of a NaN-filled buffer: NaN on both sides of every row the kernel loads, rows 16-byte aligned"""
    N, C, T, W4 = y.shape
    if layout == "nchw":
        buf = torch.full((N, C, T, W4 + 16), float("nan"), dtype=y.dtype, device=DEV)
        buf[..., 8:8 + W4] = y.to(DEV)
        view = buf[..., 8:8 + W4]
        assert view.stride(-1) == 1 and not view.is_contiguous()
    else:
        buf = torch.full((N, T, W4, C + 16), float("nan"), dtype=y.dtype, device=DEV)
        buf[..., 8:8 + C] = y.permute(0, 2, 3, 1).to(DEV)
        view = buf[..., 8:8 + C].permute(0, 3, 1, 2)
        assert view.stride(1) == 1 and view.stride(-1) == C + 16
    return view.detach()


def _device_inputs(idx, need=(True,) * 5):
    inp = _case(idx)[0]
    layout = CASES[idx][5]
    yd = _poisoned(inp[0], layout).requires_grad_(need[0])
    params = [t.to(DEV).requires_grad_(n) for t, n in zip(inp[1:5], need[1:])]
    g_s, g_p = (torch.cat([t, t[..., :8]], -1).to(DEV)[..., :t.shape[-1]] for t in inp[5:])     # rows of a wider buffer
    assert not g_s.is_contiguous() and not g_p.is_contiguous()
    return yd, params, g_s, g_p


def _kernel(idx, mode="both"):
    yd, params, g_s, g_p = _device_inputs(idx)
    T_m = CASES[idx][3]
    probs, scores = ops.predictor_tail_autograd(yd, *params, 4, T_m, EPS)
    outs = [o for o, m in ((scores, "g_p"), (probs, "g_s")) if mode != m]
    gs = [g for g, m in ((g_s, "g_p"), (g_p, "g_s")) if mode != m]
    grads = torch.autograd.grad(outs, [yd, *params], grad_outputs=gs)
    torch.cuda.synchronize()
    return (probs.detach(), scores.detach()), grads, (yd, params)


def _held(tag, got, ref, bars, dt):
    """(dy, dW, db, dgamma, dbeta) of the op against the reference under the bars; db exactly zero"""
    dy, dW, db, dga, dbe = got
    failures = []
    for name, x, r, bar in zip(NAMES, (dy, dW, dga, dbe), ref, bars):
        assert x.dtype == dt and x.shape == r.shape and torch.isfinite(x).all(), name
        err = (x.double().cpu() - r).abs().max().item()
        print(f"[tail-bwd] {tag} {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f} (max |ref| {r.abs().max().item():.3e})")
        if not err <= bar:
            failures.append((name, err, bar))
    assert db.dtype == dt and (db == 0).all()
    return failures


@pytest.mark.gpu
@pytest.mark.parametrize("idx", range(len(CASES)), ids=[_id(c) for c in CASES])
def test_kernel_against_fp64_reference(idx):
    N, H, T, T_m, dt, layout, _seed = CASES[idx]
    inp, ref, bars = _case(idx)
    (probs, scores), got, (yd, params) = _kernel(idx)
    # the forward is the inference launch, unchanged
    p0, s0 = ops.predictor_tail(yd.detach(), *(t.detach() for t in params), up=4, T_m=T_m, eps=EPS, want_scores=True)
    assert torch.equal(probs, p0) and torch.equal(scores, s0)
    assert got[0].shape == (N, 2 * H, T, T_m // 4) and got[0].is_contiguous()
    failures = _held(_id(CASES[idx]), got, ref, bars, dt)
    assert not failures, failures
    _out, again, _in = _kernel(idx)                                           # no atomics, one order: the same bits
    for a, b in zip(got, again):
        assert torch.equal(a, b)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_either_incoming_gradient_may_be_absent(mode):
    idx = 0
    inp, ref, bars = _case(idx, mode)
    _out, got, _in = _kernel(idx, mode)
    failures = _held(f"{_id(CASES[idx])} {mode}", got, ref, bars, CASES[idx][4])
    assert not failures, failures


@pytest.mark.gpu
def test_saves_y_and_the_parameters_only_and_returns_none_where_no_gradient_is_wanted():
    idx = 1                                                                    # (2,32,37,256) bf16: a map of 1.2 MB
    N, H, T, T_m, dt, _layout, _seed = CASES[idx]
    yd, params, g_s, g_p = _device_inputs(idx)
    ops.predictor_tail_autograd(yd, *params, 4, T_m, EPS)                     # (the cached weight packs of the forward exist now)
    torch.cuda.synchronize()
    packed = []

    def pack(t):
        packed.append(t)
        return t
    before = torch.cuda.memory_allocated()
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        probs, scores = ops.predictor_tail_autograd(yd, *params, 4, T_m, EPS)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - before
    map_bytes = probs.numel() * probs.element_size()
    assert probs.shape == scores.shape == (N, H, T, T_m)
    # after the forward the op holds its two outputs and nothing else of the map's size
    assert 2 * map_bytes <= held < 2 * map_bytes + map_bytes // 4, (held, map_bytes)
    assert len(packed) == 5
    assert packed[0].data_ptr() == yd.data_ptr() and packed[0].shape == yd.shape and packed[0].stride() == yd.stride()
    for t, src in zip(packed[1:], params):
        assert t.data_ptr() == src.data_ptr() and t.shape == src.shape
    assert all(t.numel() < map_bytes // 8 for t in packed[1:])
    base = torch.autograd.grad([scores, probs], [yd, *params], grad_outputs=[g_s, g_p])

    # the Function's own return values: None for every input that wants no gradient
    class Ctx:
        saved_tensors = tuple(packed)
        up, T_m, eps = 4, CASES[idx][3], EPS
    for need in ((True, False, False, False, False), (False, True, False, True, False), (False, False, True, False, True)):
        Ctx.needs_input_grad = (*need, False, False, False)
        res = predictor_tail_grad._PredictorTailFn.backward(Ctx, g_p, g_s)
        assert len(res) == 8 and all(r is None for r in res[5:])
        for r, n, b in zip(res[:5], need, base):
            assert (r is None) == (not n) and (r is None or torch.equal(r, b))
    Ctx.needs_input_grad = (False,) * 8
    assert all(r is None for r in predictor_tail_grad._PredictorTailFn.backward(Ctx, g_p, g_s))
    Ctx.needs_input_grad = (True,) * 5 + (False,) * 3
    assert all(r is None for r in predictor_tail_grad._PredictorTailFn.backward(Ctx, None, None))
    # and through autograd: only y wants one
    y1, p1, _gs, _gp = _device_inputs(idx, need=(True, False, False, False, False))
    _probs, s1 = ops.predictor_tail_autograd(y1, *p1, 4, T_m, EPS)
    s1.backward(g_s)
    want = torch.autograd.grad(ops.predictor_tail_autograd(yd, *params, 4, T_m, EPS)[1], [yd], grad_outputs=[g_s])[0]
    assert torch.equal(y1.grad, want) and all(t.grad is None for t in p1)


@pytest.mark.gpu
def test_a_predictor_length_outside_the_predicate_is_refused_not_emulated():
    """T_m = 384: the lane and LDS plan stop at 256; the predicate says so on both sides of the ABI and the op raises."""
    H, T_m = 4, 384
    y, W, b, gamma, beta, _gs, _gp = (t.to(DEV) for t in make_inputs(1, H, 3, T_m, seed=41, dtype=BF))
    assert _lib.load().sea_predictor_tail_bwd_supported(2 * H, H, T_m // 4, 4, T_m, _lib.dtype_code(BF)) == 0
    assert not ops.predictor_tail_grad_supported(y, W, b, gamma, beta, 4, T_m)
    with pytest.raises(RuntimeError, match="predictor_tail_grad_supported"):
        ops.predictor_tail_autograd(y.requires_grad_(True), W, b, gamma, beta, 4, T_m, EPS)


def test_the_cases_cover_one_block_a_ragged_last_block_and_many():
    rows = [c[0] * c[2] for c in CASES]
    assert rows[0] < block_rows(rows[0]) and rows[4] == 1
    assert rows[5] // block_rows(rows[5]) > 256 and rows[5] % block_rows(rows[5]) != 0 and rows[2] % block_rows(rows[2]) != 0


# ---- module tier -------------------------------------------------------------------------------------------------------
class Cfg:
    def __init__(self, hidden, heads, max_pos):
        self.hidden_size, self.num_attention_heads, self.max_position_embeddings = hidden, heads, max_pos


H_, D_, T_, TM_, K_ = 4, 64, 96, 32, 8


@functools.lru_cache(maxsize=None)
def _layer_and_inputs(dt):
    S.seed(42)
    pc = PerlinAttentionConfig(k=K_, attention_predictor_length=TM_, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix')
    layer = PerlinSelfAttention(Cfg(H_ * D_, H_, T_), pc).to(DEV).to(dt).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = True                                              # sparse mode
    S.seed(1)
    x = torch.randn((1, H_, T_, D_), device=DEV).to(dt)
    fp_min = torch.finfo(torch.float16).min / 2
    idx = torch.arange(T_, device=DEV)
    mask = ((idx.view(1, T_) > idx.view(T_, 1)) * fp_min).view(1, 1, T_, T_).to(dt)
    scores_truth = (torch.randn((1, H_, T_, T_), device=DEV) * 2.0).to(dt)
    return layer, x, mask, scores_truth


def _step(dt, tail, performer=False):
    """One training step of `PerlinAttention.forward`, called directly: (loss, {parameter name: gradient})"""
    layer, x, mask, scores_truth = _layer_and_inputs(dt)
    att = layer.attention
    q, k, v = x * D_ ** -0.5, x.clone(), x.clone()
    att.fused_kd_loss, att.fused_tail_grad, att.fused_performer_grad = True, tail, performer
    layer.zero_grad()
    try:
        out = att(q, k, v, q, k, v, q, k, mask, scores_truth, None)
        out.loss.backward()
    finally:
        att.fused_kd_loss, att.fused_tail_grad, att.fused_performer_grad = False, False, False
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().clone() for n, p in att.named_parameters() if p.grad is not None}
    return out.loss.detach().clone(), grads


def _counting(monkeypatch):
    lib, calls = _lib.load(), []
    real = lib.sea_predictor_tail_bwd

    def spy(*a):
        calls.append(1)
        return real(*a)
    monkeypatch.setattr(lib, "sea_predictor_tail_bwd", spy)
    return calls


def _names(att):
    cnn = att.attention_predictor_cnn
    conv4 = list(cnn[1].module.net.children())[-1].module
    by_id = {id(p): n for n, p in att.named_parameters()}
    return (by_id[id(conv4.weight)], by_id[id(cnn[2].module.weight)], by_id[id(att.attention_predictor_dec_row[0].weight)])


def _torch_stand_in(att):
    """What `_estimate` does with the switch off, behind the new op's name: the layer's own upsample, 1x1 convolution, KeepRes
    resize, LayerNorm and softmax"""
    cnn = att.attention_predictor_cnn
    keepres = cnn[1].module
    body = list(keepres.net.children())

    def f(y, conv_w, conv_b, ln_w, ln_b, up, T_m, eps=1e-5):
        s = cnn[2](interpolate(body[-1](body[-2](y)), (y.shape[-2], keepres.output_width)))
        return torch.softmax(s.float(), dim=-1).to(s.dtype), s
    return f


class _RefTail(torch.autograd.Function):
    """`TailReference`: fp64 inside, rounded to the data type at its edges"""

    @staticmethod
    def forward(ctx, y, conv_w, conv_b, ln_w, ln_b, eps):
        ctx.args = tuple(t.detach().cpu() for t in (y, conv_w, conv_b, ln_w, ln_b))
        ctx.eps, ctx.like = eps, (y, conv_w, conv_b, ln_w, ln_b)
        ctx.set_materialize_grads(False)
        p, s = TailReference().forward(*ctx.args, eps)
        return p.to(y.dtype).to(y.device), s.to(y.dtype).to(y.device)

    @staticmethod
    def backward(ctx, g_p, g_s):
        cpu = lambda g: None if g is None else g.detach().cpu()
        grads = TailReference().backward(*ctx.args, ctx.eps, cpu(g_s), cpu(g_p))
        return (*(g.to(like.dtype).to(like.device) for g, like in zip(grads, ctx.like)), None)


def _ref_stand_in(y, conv_w, conv_b, ln_w, ln_b, up, T_m, eps=1e-5):
    return _RefTail.apply(y, conv_w, conv_b, ln_w, ln_b, eps)


def _numbers(dt, monkeypatch, performer, tag):
    """(ii): the real op against `TailReference` standing in for it, the switch-off run as yardstick"""
    att = _layer_and_inputs(dt)[0].attention
    calls = _counting(monkeypatch)
    loss_y, g_y = _step(dt, False, performer)                                  # the torch modules: the yardstick
    assert calls == []                                                         # (iii) never with the switch off
    loss_k, g_k = _step(dt, True, performer)                                   # the kernels
    assert len(calls) == 1                                                     # (iii) one HIP backward per step
    with monkeypatch.context() as m:
        m.setattr(ops, "predictor_tail_autograd", _ref_stand_in)               # fp64: the reference
        loss_r, g_r = _step(dt, True, performer)
    assert len(calls) == 1
    held = [("loss", loss_k, loss_y, loss_r)] + [(f"d {n}", g_k[n], g_y[n], g_r[n]) for n in _names(att)]
    failures = []
    for name, got, yard, ref in held:
        ref = ref.double().cpu()
        bar = bar_of(yard.double().cpu(), ref)
        err = (got.double().cpu() - ref).abs().max().item()
        print(f"[tail-bwd] layer {tag} {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f} (max |ref| {ref.abs().max().item():.3e})")
        assert torch.isfinite(got).all() and ref.abs().max().item() > 0
        if not err <= bar:
            failures.append((name, err, bar))
    assert not failures, failures


@pytest.mark.gpu
def test_layer_wiring_is_bitwise_the_torch_path_behind_the_switch(monkeypatch):
    att = _layer_and_inputs(BF)[0].attention
    assert att.fused_tail_grad is False                                        # off by default
    calls = _counting(monkeypatch)
    loss_off, g_off = _step(BF, False)
    assert calls == [] and loss_off.item() > 0                                 # with the switch off the HIP backward never runs
    seen = []
    stand_in = _torch_stand_in(att)

    def spy(*a, **kw):
        seen.append(a)
        return stand_in(*a, **kw)
    with monkeypatch.context() as m:
        m.setattr(ops, "predictor_tail_autograd", spy)
        loss_on, g_on = _step(BF, True)
    assert len(seen) == 1 and seen[0][0].shape == (1, 2 * H_, T_, TM_ // 4) and seen[0][1].shape == (H_, 2 * H_) and calls == []
    assert seen[0][5:] == (4, TM_, 1e-5)
    assert torch.equal(loss_on, loss_off) and sorted(g_on) == sorted(g_off)
    for n in g_off:
        assert torch.equal(g_on[n], g_off[n]), n
    for n in _names(att):
        assert g_off[n].abs().max().item() > 0, n


@pytest.mark.gpu
@pytest.mark.parametrize("dt", (BF, F32), ids=("bf16", "fp32"))
def test_layer_numbers_against_the_fp64_tail(dt, monkeypatch):
    _numbers(dt, monkeypatch, performer=False, tag=str(dt).split(".")[1])


@pytest.mark.gpu
def test_layer_numbers_with_the_performer_backward_on_as_well(monkeypatch):
    """`fused_performer_grad` on in all three runs, so that they differ in the tail alone"""
    _numbers(BF, monkeypatch, performer=True, tag="bf16 + performer grad")
