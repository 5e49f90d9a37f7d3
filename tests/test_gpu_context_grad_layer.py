"""-m gpu: the layer switch `PerlinAttention.fused_context_grad`, at the module tier of 5.10: one bf16 layer, H = 4,
d = 64, T = 96, T_M = 32, sparse mode, `fused_kd_loss` with a teacher score tensor AND a context truth, so that the loss is a
function of the context branch.  v comes out of a Linear as the strided (N, T, H, d) view a model hands over: the gradient of that
projection is the context branch's dv, the gradient of `attention_predictor_dec_scaler` its d row_scale and d mix."""
import pytest
import torch

import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from test_gpu_context_grad import context_reference
from test_gpu_kd_score_loss import padded_mask
from test_performer_bwd_reference import bar_of

pytestmark = pytest.mark.gpu
DEV, BF = "cuda", torch.bfloat16
H_, D_, T_, TM_, K_ = 4, 64, 96, 32, 8


class Cfg:
    hidden_size, num_attention_heads, max_position_embeddings = H_ * D_, H_, T_


@pytest.fixture(scope="module")
def setup():
    S.seed(42)
    pc = PerlinAttentionConfig(k=K_, attention_predictor_length=TM_, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix')
    layer = PerlinSelfAttention(Cfg(), pc).to(DEV).to(BF).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = True                                              # sparse mode
    vproj = torch.nn.Linear(H_ * D_, H_ * D_).to(DEV).to(BF)
    S.seed(1)
    x = torch.randn((1, H_, T_, D_), device=DEV).to(BF)
    idx = torch.arange(T_, device=DEV)
    mask = ((idx.view(1, T_) > idx.view(T_, 1)) * (torch.finfo(torch.float16).min / 2)).view(1, 1, T_, T_).to(BF)
    scores_truth = (torch.randn((1, H_, T_, T_), device=DEV) * 2.0).to(BF)
    ctx_truth = torch.randn((1, T_, H_ * D_), device=DEV)
    return layer, vproj, x, mask, scores_truth, ctx_truth


def _step(setup, switch, mask=None):
    """One training step of `PerlinAttention.forward`: (loss, the two gradients the context branch feeds)"""
    layer, vproj, x, causal, scores_truth, ctx_truth = setup
    att = layer.attention
    q, k = x * D_ ** -0.5, x.clone()
    v = vproj(x.permute(0, 2, 1, 3).reshape(1, T_, H_ * D_)).view(1, T_, H_, D_).permute(0, 2, 1, 3)
    att.fused_kd_loss, att.fused_context_grad = True, switch
    layer.zero_grad()
    vproj.zero_grad()
    try:
        out = att(q, k, v, q, k, v, q, k, causal if mask is None else mask, scores_truth, ctx_truth)
        # (a padded batch has no fused KD loss, and sparse mode then leaves the context term out: put that term back)
        loss = out.loss if torch.is_tensor(out.loss) else torch.nn.functional.mse_loss(ctx_truth, out.context_layer)
        loss.backward()
    finally:
        att.fused_kd_loss, att.fused_context_grad = False, False
    torch.cuda.synchronize()
    grads = {"v projection": vproj.weight.grad, "dec_scaler": att.attention_predictor_dec_scaler[0].weight.grad}
    return loss.detach().clone(), {n: g.detach().clone() for n, g in grads.items()}


def _spied(monkeypatch, fn=None):
    calls, real = [], ops.sparse_context_autograd
    monkeypatch.setattr(ops, "sparse_context_autograd", lambda *a, **kw: calls.append(a) or (fn or real)(*a, **kw))
    return calls


def _fp64_stand_in(q, k, v, csr, row_scale, mix, out_dtype=torch.float32):
    dense = ops.flat_csr_to_dense(csr, T_, H_) > 0
    rs = None if row_scale is None else row_scale.double()
    return context_reference(q.double(), k.double(), v.double(), dense, rs, mix.double(), q.dtype)[0].to(out_dtype)


def test_layer_calls_the_op_once_per_step_and_holds_the_fp64_context_branch(setup, monkeypatch):
    assert setup[0].attention.fused_context_grad is False                      # off by default
    with monkeypatch.context() as m:
        calls = _spied(m)
        loss_y, g_y = _step(setup, False)                                      # today's path: the yardstick; the op never runs
        assert calls == []
        loss_k, g_k = _step(setup, True)                                       # the kernels: once per step, on v itself
        assert len(calls) == 1 and calls[0][2].shape == (1, H_, T_, D_) and not calls[0][2].is_contiguous()
    calls = _spied(monkeypatch, _fp64_stand_in)
    loss_r, g_r = _step(setup, True)                                           # fp64 behind the op's name: the reference
    assert len(calls) == 1
    failures = []
    for name, got, yard, ref in [("loss", loss_k, loss_y, loss_r)] + [(f"d {n}", g_k[n], g_y[n], g_r[n]) for n in g_r]:
        ref = ref.double()
        bar, err = bar_of(yard.double(), ref), (got.double() - ref).abs().max().item()
        print(f"[ctx-grad] layer {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f} (max |ref| {ref.abs().max().item():.3e})")
        assert torch.isfinite(got).all() and ref.abs().max().item() > 0
        if not err <= bar:
            failures.append((name, err, bar))
    assert not failures, failures


def test_a_padded_batch_is_bitwise_the_switch_off_step(setup, monkeypatch):
    calls = _spied(monkeypatch)
    mask = padded_mask(setup[3], 8)
    loss_off, g_off = _step(setup, False, mask)
    loss_on, g_on = _step(setup, True, mask)
    assert calls == [] and torch.equal(loss_on, loss_off) and all(torch.equal(g_on[n], g_off[n]) for n in g_off)
