"""The distillation losses with the teacher FACTORED (`ops.TeacherScores(q_t, k_t)` in place of the (N,H,T,T) score tensor;
include/sea_hip_train.h, "the teacher"): what can be held without a GPU.

`TeacherScores` and `opt_plumbing.teacher_scores`; the layer on the CPU, where every path is a fallback and must return, bit for
bit, what it returns for the tensor q_t k_t^T; the references of the two existing suites (`KdReference`, `KdScoreReference`) on the
fp64 teacher product against the fp32 yardsticks on the fp32 product -- the kernels keep the product's fp32 accumulator, they do
NOT round it to the data type, and the printed rate says why; two witnesses that the GPU comparison can fail (the teacher's key
tile taken from the student, the padded k-step of head size 80 forgotten for the teacher).  The C entries themselves:
tests/test_kd_abi.py."""
import pytest
import torch

import sea_attention_amd as S
from sea_attention_amd import opt_plumbing
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from test_kd_loss_reference import FP_MIN16, KdReference, bar_of, torch_rows
from test_kd_score_loss_reference import KdScoreReference, torch_score_rows

F32, F16, BF = torch.float32, torch.float16, torch.bfloat16


def _qk(N, H, T, D, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return tuple((torch.randn((N, H, T, D), generator=g, dtype=torch.float64) * 0.6).to(dtype) for _ in range(4))


def _dd(a, b):
    """a b^T in fp64"""
    return a.double() @ b.double().transpose(-1, -2)


def _ff(a, b):
    """a b^T in fp32, not rounded to the data type: the kernels' semantics"""
    return a.float() @ b.float().transpose(-1, -2)


# ---- TeacherScores ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, BF, F16])
def test_teacher_scores_is_a_factored_stand_in(dtype):
    _q, _k, qt, kt = _qk(2, 3, 20, 64, dtype, 1)
    qt.requires_grad_(True)
    ts = ops.TeacherScores(qt, kt)
    assert ts.shape == (2, 3, 20, 20) and isinstance(ts.shape, torch.Size)
    assert ts.dtype == dtype and ts.device == qt.device
    assert not ts.q.requires_grad and not ts.k.requires_grad                   # held detached: the teacher gets no gradient
    assert ts.q.data_ptr() == qt.data_ptr() and ts.k.data_ptr() == kt.data_ptr()   # references, no copies
    dense = ts.dense()
    assert dense.dtype == dtype and not dense.requires_grad
    assert torch.equal(dense, torch.matmul(qt.detach(), kt.transpose(-1, -2)))
    same = ts.to("cpu", non_blocking=True)
    assert isinstance(same, ops.TeacherScores) and torch.equal(same.q, ts.q) and torch.equal(same.k, ts.k)
    assert ts.to(torch.device("cpu")).shape == ts.shape


def test_teacher_scores_refuses_two_shapes_or_two_dtypes():
    q = torch.zeros(1, 2, 8, 64)
    with pytest.raises(ValueError, match="one shape"):
        ops.TeacherScores(q, q[:, :, :4])
    with pytest.raises(ValueError, match="one shape"):
        ops.TeacherScores(q[0], q[0])
    with pytest.raises(ValueError, match="dtype"):
        ops.TeacherScores(q, q.to(BF))
    with pytest.raises(TypeError):
        ops.TeacherScores(q, None)


def test_opt_plumbing_teacher_scores_uses_the_blocks_head_layout():
    S.seed(3)
    attn = opt_plumbing.SeaOPTAttention(128, 2, max_position_embeddings=32)
    h = torch.randn((2, 12, 128))
    ts = opt_plumbing.teacher_scores(attn, h)
    assert isinstance(ts, ops.TeacherScores) and ts.shape == (2, 2, 12, 12) and ts.q.shape == (2, 2, 12, 64)
    assert not ts.q.requires_grad and ts.q.is_contiguous() and ts.k.is_contiguous()
    with torch.no_grad():
        want = attn._heads(attn.q_proj(h) * attn.scaling) @ attn._heads(attn.k_proj(h)).transpose(-1, -2)
    assert torch.equal(ts.dense(), want)
    attn.teacher_attention_scores = ts                                          # the attribute may hold it
    assert attn.teacher_attention_scores is ts


# ---- the layer on the CPU: every path is a fallback, bit for bit the tensor's ----------------------------------------------
H_, D_, T_, TM_, K_ = 4, 64, 96, 32, 8


class Cfg:
    def __init__(self, hidden, heads, max_pos):
        self.hidden_size, self.num_attention_heads, self.max_position_embeddings = hidden, heads, max_pos


@pytest.fixture(scope="module")
def cpu_layer():
    S.seed(42)
    pc = PerlinAttentionConfig(k=K_, attention_predictor_length=TM_, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix')
    layer = PerlinSelfAttention(Cfg(H_ * D_, H_, T_), pc).eval()
    S.seed(1)
    x = torch.randn((1, H_, T_, D_))
    qt, kt = torch.randn((1, H_, T_, D_)) * 0.4, torch.randn((1, H_, T_, D_)) * 0.4
    context_truth = torch.randn((1, T_, H_ * D_))
    return layer, x, qt, kt, context_truth


@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("switches", [False, True])
def test_layer_on_the_cpu_returns_what_the_dense_tensor_gives(cpu_layer, dtype, switches):
    layer32, x, qt, kt, context_truth = cpu_layer
    import copy
    layer = copy.deepcopy(layer32).to(dtype)
    att = layer.attention
    att.fused_kd_loss = att.fused_kd_score_loss = switches                     # on the CPU `*_supported` is False either way
    x, qt, kt = x.to(dtype), qt.to(dtype), kt.to(dtype)
    idx = torch.arange(T_)
    mask = ((idx.view(1, T_) > idx.view(T_, 1)) * FP_MIN16).view(1, 1, T_, T_).to(dtype)

    def run(truth):
        S.seed(7)
        return layer(None, None, None, query_layer=x * D_ ** -0.5, key_layer=x.clone(), value_layer=x.clone(), attention_mask=mask,
                     attention_scores_truth=truth, context_layer_truth=context_truth.to(dtype))
    ts = ops.TeacherScores(qt, kt)
    want = run(torch.matmul(qt, kt.transpose(-1, -2)))
    got = run(ts)
    lazy = run(lambda: ops.TeacherScores(qt, kt))                               # a callable that returns one
    assert torch.isfinite(want.loss) and want.loss.item() > 0
    for out in (got, lazy):
        assert torch.equal(out.loss, want.loss) and torch.equal(out.context_layer, want.context_layer)


def test_supported_is_false_on_the_cpu_and_for_the_wrong_teacher():
    q, _k, qt, kt = _qk(1, 2, 16, 64, BF, 2)
    est = torch.zeros((1, 2, 16, 8), dtype=BF)
    ts = ops.TeacherScores(qt, kt)
    assert not ops.kd_score_loss_supported(q, q, ts) and not ops.kd_estimator_loss_supported(est, ts)        # CPU tensors
    for bad in (ops.TeacherScores(qt[..., :48], kt[..., :48]),                 # D = 48
                ops.TeacherScores(qt.float(), kt.float()),                     # fp32
                ops.TeacherScores(qt.to(F16), kt.to(F16)),                     # not the student's type (score term)
                ops.TeacherScores(qt[:, :, :8], kt[:, :, :8])):                # another T
        assert not ops.kd_score_loss_supported(q, q, bad)
    for bad in (ops.TeacherScores(qt[..., :48], kt[..., :48]), ops.TeacherScores(qt.float(), kt.float())):
        assert not ops.kd_estimator_loss_supported(est, bad)
    for call in (lambda: ops.kd_score_loss(q, q, ts), lambda: ops.kd_score_loss_parts(q, q, ts),
                 lambda: ops.kd_estimator_loss(est, ts), lambda: ops.kd_estimator_loss_parts(est, ts)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


# ---- the factored references and what they can tell apart ------------------------------------------------------------------
WITNESS = [((1, 2, 300, 80), BF), ((2, 3, 100, 64), F16)]
T_M_W = 32


def _witness_inputs(shape, dtype):
    N, H, T, D = shape
    q, k, qt, kt = _qk(N, H, T, D, dtype, 3)
    g = torch.Generator().manual_seed(5)
    est = (torch.randn((N, H, T, T_M_W), generator=g, dtype=torch.float64) * 2.0).to(dtype)
    return q, k, qt, kt, est


@pytest.mark.parametrize("shape,dtype", WITNESS)
def test_factored_references_against_the_fp32_yardsticks(shape, dtype):
    """The references on the fp64 product agree with the fp32 yardsticks on the fp32 product to fp32 rounding: the yardsticks'
    error is what the bars of the GPU suite are made of, so it has to be small against the quantities themselves."""
    q, k, qt, kt, est = _witness_inputs(shape, dtype)
    ref_s = KdScoreReference(q, k, _dd(qt, kt))
    y_kl, y_mse, y_q, y_st, y_loss = torch_score_rows(q, k, _ff(qt, kt))
    for nm, y in (("row_kl", y_kl), ("row_mse", y_mse), ("row_q", y_q), ("row_stats", y_st)):
        r = getattr(ref_s, nm)
        assert (y.double() - r).abs().max().item() <= 2e-5 * max(1.0, r.abs().max().item()), nm
    assert abs(y_loss.item() - ref_s.loss.item()) <= 1e-5 * abs(ref_s.loss.item())
    ref_e = KdReference(est, _dd(qt, kt))
    e_kl, e_mse, e_g, e_loss = torch_rows(est.float(), _ff(qt, kt), fp_min=FP_MIN16)
    for nm, y in (("row_kl", e_kl), ("row_mse", e_mse), ("pix_tgt", e_g)):
        r = getattr(ref_e, nm)
        assert (y.double() - r).abs().max().item() <= 2e-5 * max(1.0, r.abs().max().item()), nm
    assert abs(e_loss.item() - ref_e.loss.item()) <= 1e-5 * abs(ref_e.loss.item())


@pytest.mark.parametrize("shape,dtype", WITNESS)
def test_the_comparison_can_fail(shape, dtype):
    """(a) The teacher's key tile taken from the STUDENT's k misses row_kl and row_mse of both terms, and pix_tgt, by more than 10
    bars in every row t >= 8.  (b) At D = 80, columns 64 .. 79 of the teacher's product dropped miss them by more than 10 bars in
    every row t >= 8.  Printed, not asserted: the rate for a product rounded to the 16-bit type -- why the kernels' semantics
    (the fp32 accumulator, "the teacher" in the header) is a stated deviation from handing over the teacher's own bmm result."""
    N, H, T, D = shape
    q, k, qt, kt, est = _witness_inputs(shape, dtype)
    x64 = _dd(qt, kt)
    x32 = _ff(qt, kt)
    ref_s, ref_e = KdScoreReference(q, k, x64), KdReference(est, x64)
    y_kl, y_mse, _q, _st, _l = torch_score_rows(q, k, x32)
    e_kl, e_mse, e_g, _l = torch_rows(est.float(), x32, fp_min=FP_MIN16)
    bars = {("score", "row_kl"): bar_of(y_kl, ref_s.row_kl), ("score", "row_mse"): bar_of(y_mse, ref_s.row_mse),
            ("est", "row_kl"): bar_of(e_kl, ref_e.row_kl), ("est", "row_mse"): bar_of(e_mse, ref_e.row_mse),
            ("est", "pix_tgt"): bar_of(e_g, ref_e.pix_tgt)}

    def rates(tag, x_wrong, asserted):
        wrong = {"score": KdScoreReference(q, k, x_wrong), "est": KdReference(est, x_wrong)}
        right = {"score": ref_s, "est": ref_e}
        for (term, nm), bar in bars.items():
            moved = (getattr(wrong[term], nm) - getattr(right[term], nm)).abs()
            moved = moved.amax(-1) if nm == "pix_tgt" else moved                # per row
            over = moved[..., 8:] / bar
            frac = (over > 10).double().mean().item()
            print(f"[kd-qk-witness] {shape} {term} {nm} {tag}: {frac:.3f} of the rows t >= 8 beyond 10 bars "
                  f"(median {over.median().item():.0f} bars, bar {bar:.3e})")
            if asserted:
                assert frac == 1.0, (tag, term, nm, frac, bar, moved[..., 8:].min().item())
    rates("teacher key tile from the student's k", _dd(qt, k), True)
    if D == 80:
        rates("teacher columns 64 .. 79 dropped", _dd(qt[..., :64], kt[..., :64]), True)
    rates(f"teacher product rounded to {str(dtype)[6:]}", torch.matmul(qt.float(), kt.float().transpose(-1, -2)).to(dtype).double(), False)
