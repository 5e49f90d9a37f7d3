"""-m gpu: the sparse context branch as one op (ops.sparse_context_autograd, csrc/sea_context_grad.hip), DESIGN 5.15.

Reference: the whole expression -- masked softmax product over the op's own CSR, row scale, cumulative average of v rounded to the
data type (identity gradient), mix, permute -- in fp64 dense autograd on the rounded inputs.  Yardstick: today's path on the same
inputs on the GPU, `sparse_attention_autograd` + the fp32 torch cumsum exactly as `_forward_sparse` writes it.  Bar per case and
quantity (5.7's rule): 4 x the yardstick's largest error, at least 2^-22 of the reference's largest magnitude.

An average within the worst-case error of ANY fp32 summation order, 2^-24 (sum |v_s| + |avg|) to first order, of a rounding boundary
of the data type may round the other way in fp32, in the yardstick as in the kernel -- unless fp32 is provably exact there (small
multiples of one ulp, an fp32 quotient: a tie of two averaged 16-bit values above all).  Such elements are left out of the ctx
comparison for both, must be finite, and are at most 1 % of a case (a property of the inputs, asserted before any kernel runs).  v
is drawn around 1.25 so that its average stays in one binade: a zero-mean average shrinks like t^-1/2, and the data type's spacing
with it, while the summation error grows with t."""
import functools

import pytest
import torch

from oracle import sea_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F32, F16, BF, F64 = torch.float32, torch.float16, torch.bfloat16, torch.float64
T_M, K = 16, 4
#         N  H  T    D    data out  row_scale seed
CASES = [(1, 2, 1, 64, BF, F32, True, 1), (1, 2, 64, 64, BF, F32, True, 2), (1, 2, 65, 64, BF, F32, True, 3),
         (2, 3, 130, 64, F16, F32, False, 4), (1, 2, 200, 80, BF, BF, True, 5), (1, 1, 193, 128, F32, F32, True, 6)]
IDS = ["N%d-H%d-T%d-D%d-%s-out-%s%s" % (*c[:4], str(c[4])[6:], str(c[5])[6:], "" if c[6] else "-no-rs") for c in CASES]
NAMES = ("ctx", "dq", "dk", "dv", "d mix", "d row_scale")


def context_reference(q, k, v, dense_mask, rs, mix, dt):
    """fp64: (the (N, T, H D) context, the mask of its elements whose average fp32 may round the other way)"""
    N, H, T, D = v.shape
    s = torch.matmul(q, k.transpose(-1, -2)).masked_fill(~dense_mask, float("-inf"))
    o = torch.matmul(torch.nan_to_num(torch.softmax(s, -1), nan=0.0), v)              # an empty (row, head): all -inf
    if rs is not None:
        o = o * rs.unsqueeze(-1)
    avg = v.cumsum(-2) / torch.arange(1, T + 1, dtype=F64, device=v.device).view(1, 1, T, 1)
    x = avg.detach()
    near = x.to(dt).double()
    a = mix.unsqueeze(-1)
    ctx = (o * a + (1.0 - a) * (avg + (near - x))).permute(0, 2, 1, 3).reshape(N, T, H * D)
    if dt == F32:
        return ctx, torch.zeros_like(ctx, dtype=torch.bool)
    ulp = lambda y: torch.exp2(torch.floor(torch.log2(y.abs())) - (7 if dt == BF else 10))
    band = 2.0 ** -24 * (v.detach().abs().cumsum(-2) + x.abs())
    # fp32 is EXACT in any order where every partial sum is below 2^24 multiples of the smallest ulp among v_0 .. v_t
    n = torch.arange(1, T + 1, dtype=F64, device=v.device).view(1, 1, T, 1)
    exact = (n * v.detach().abs().cummax(-2).values / ulp(v.detach()).cummin(-2).values <= 2.0 ** 24) & (x.float().double() == x)
    amb = (ulp(x) / 2 - (x - near).abs() <= band) & ~exact
    return ctx, amb.permute(0, 2, 1, 3).reshape(N, T, H * D)


@functools.lru_cache(maxsize=None)
def _case(idx, keep_none=False):
    """Inputs and CSR on the device, fp64 reference (ctx + gradients), the ambiguous ctx elements, the yardstick's bars."""
    from sea_attention_amd.perlin_attention import ops
    N, H, T, D, dt, out_dt, use_rs, seed = CASES[idx]
    g = torch.Generator().manual_seed(seed)
    probs = torch.softmax(torch.randn((N, H, T, T_M), generator=g), -1)
    keep = O.keep_counts_module(H, T, T_M, K).clamp_max(H * T_M).to(torch.int32)      # row 0 keeps every key
    if keep_none:
        keep[:] = 0
    elif T == 1:
        keep[:] = 1                                     # one pixel: one head keeps its only key, the other head's row is empty
    else:
        keep[T // 2], keep[-1] = 0, H * T_M             # an empty row, and the longest row keeps all its keys
    csr, _ = ops.topk_to_csr(probs.to(DEV), keep.to(DEV), K, target_width=T)
    dense_mask = ops.flat_csr_to_dense(csr, T, H) > 0
    rnd = lambda *shape: torch.randn(shape, generator=g)
    q, k, v = (rnd(N, H, T, D) * D ** -0.5).to(dt), rnd(N, H, T, D).to(dt), (1.25 + 0.5 * rnd(N, H, T, D)).to(dt)
    rs = torch.sigmoid(rnd(N, H, T)) if use_rs else None
    mix, gout = torch.sigmoid(rnd(N, H, T)), rnd(N, T, H * D).to(out_dt)
    inputs = [t.to(DEV) for t in (q, k, v, mix) + ((rs,) if use_rs else ())]
    gout = gout.to(DEV)
    lv = [t.double().requires_grad_(True) for t in inputs]
    ref_ctx, amb = context_reference(*lv[:3], dense_mask, lv[4] if use_rs else None, lv[3], dt)
    ref = [ref_ctx.detach(), *torch.autograd.grad(ref_ctx, lv, gout.double())]
    assert amb.float().mean().item() <= 0.01, amb.float().mean().item()                # of the inputs alone
    ly = [t.clone().requires_grad_(True) for t in inputs]
    avg = (ly[2].float().cumsum(-2) / torch.arange(1, T + 1, device=DEV, dtype=F32).view(1, 1, -1, 1)).to(dt)
    p2 = ops.sparse_attention_autograd(*ly[:3], csr, row_scale=ly[4] if use_rs else None, avg=avg, mix=ly[3])
    yard_ctx = p2.permute(0, 2, 1, 3).reshape(N, T, H * D).to(out_dt)
    yard = [yard_ctx.detach(), *torch.autograd.grad(yard_ctx, ly, gout)]
    assert torch.isfinite(yard[0]).all()
    keep_ = lambda x, i: x.double()[~amb] if i == 0 else x.double()
    bars = [max(4 * (keep_(y, i) - keep_(r, i)).abs().max().item(), 2.0 ** -22 * r.abs().max().item())
            for i, (y, r) in enumerate(zip(yard, ref))]
    return inputs, csr, gout, ref, amb, bars


def _kernel(idx, keep_none=False):
    from sea_attention_amd.perlin_attention import ops
    inputs, csr, gout, _ref, _amb, _bars = _case(idx, keep_none)
    lk = [t.clone().requires_grad_(True) for t in inputs]
    ctx = ops.sparse_context_autograd(*lk[:3], csr, lk[4] if len(lk) > 4 else None, lk[3], out_dtype=CASES[idx][5])
    grads = torch.autograd.grad(ctx, lk, gout)
    torch.cuda.synchronize()
    return [ctx.detach(), *grads]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=IDS)
def test_op_against_fp64_reference(idx):
    N, H, T, D, dt, out_dt, use_rs, _seed = CASES[idx]
    _inputs, _csr, _gout, ref, amb, bars = _case(idx)
    got = _kernel(idx)
    assert [t.dtype for t in got] == [out_dt, dt, dt, dt, F32] + [F32] * use_rs and got[0].shape == (N, T, H * D)
    failures = []
    for i, (x, r) in enumerate(zip(got, ref)):
        assert x.shape == r.shape and torch.isfinite(x).all(), NAMES[i]
        err = ((x.double() - r)[~amb] if i == 0 else (x.double() - r)).abs().max().item()
        print(f"[ctx-grad] {IDS[idx]} {NAMES[i]}: max err {err:.3e} bar {bars[i]:.3e} ratio {err / max(bars[i], 1e-300):.3f}"
              f" (max |ref| {r.abs().max().item():.3e}, ambiguous {int(amb.sum()) if i == 0 else 0})")
        if not err <= bars[i]:
            failures.append((NAMES[i], err, bars[i]))
    assert not failures, failures


def test_one_row_that_keeps_nothing_is_the_closed_form():
    """T = 1, no entries: o = 0 and the average is v itself, so ctx = (1 - a) v, dv = (1 - a) g and d row_scale = 0"""
    inputs, _csr, gout, *_ = _case(0, keep_none=True)
    ctx, _dq, _dk, dv, _da, drs = _kernel(0, keep_none=True)
    v, one_minus_a = inputs[2].double(), (1.0 - inputs[3].double()).unsqueeze(-1)
    N, H, T, D = v.shape
    want_ctx = (one_minus_a * v).permute(0, 2, 1, 3).reshape(N, T, H * D)
    want_dv = one_minus_a * gout.double().view(N, T, H, D).permute(0, 2, 1, 3)
    assert ((ctx.double() - want_ctx).abs() <= 2.0 ** -22 * want_ctx.abs()).all()
    assert ((dv.double() - want_dv).abs() <= 2.0 ** -8 * want_dv.abs()).all()          # one bf16 rounding
    assert (drs == 0).all()


def test_two_runs_give_the_same_bits():
    a, b = _kernel(4), _kernel(4)
    for i in (0, 1, 4, 5):                                 # ctx, dq, d mix, d row_scale: no order-dependent sum anywhere
        assert torch.equal(a[i], b[i]), NAMES[i]


def test_another_key_length_is_refused_not_emulated():
    from sea_attention_amd.perlin_attention import ops
    inputs, csr, *_ = _case(1)
    q, k, v, mix, rs = inputs
    assert ops.sparse_context_grad_supported(q, k, v, csr, rs, mix)
    q32, mix32, rs32 = q[:, :, -32:].contiguous(), mix[:, :, -32:].contiguous(), rs[:, :, -32:].contiguous()
    assert not ops.sparse_context_grad_supported(q32, k, v, csr, rs32, mix32)
    with pytest.raises(RuntimeError, match="sparse_context_grad_supported"):
        ops.sparse_context_autograd(q32, k, v, csr, rs32, mix32)
