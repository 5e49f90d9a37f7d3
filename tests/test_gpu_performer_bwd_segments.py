"""The row-segmented Performer backward (csrc/sea_performer_bwd_seg.hip, `grad_segments` of ops.performer_value_autograd,
`PerlinAttention.fused_performer_grad_segments`), DESIGN 5.10a.

Reference, yardstick, bar and left-out rows are those of test_gpu_performer_bwd.py (5.10), on its cases and seeds: the fp64
`PerformerReference` on the rounded inputs; bar = 4 x the largest error of `performer.py` under fp32 autograd on the CPU, at least
2^-22 of the reference's largest magnitude; rows with a feature at the ReLU's kink left out of dq / dk for both (at most 3 %,
asserted in `_case` before any kernel runs); q, k at 0.05 of unit scale."""
import pytest
import torch

from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import ops
from test_performer_bwd_reference import PerformerReference, ambiguous_rows, bar_of, make_inputs, performer_py  # noqa: F401
from test_gpu_performer_bwd import (CASES, NAMES, _RefPerformer, _case, _device_inputs, _id, _kept, _step,      # noqa: F401
                                    _torch_stand_in, layer_and_inputs)

#          case  requested  effective
SEGMENTS = [(0, 2, 2),           # T = 65: the last segment is one row of a partial chunk
            (0, 8, 2),           # the request is clamped
            (1, 2, 2), (1, 4, 4),                # T = 200, N H = 6; one chunk per segment
            (2, 3, 3),           # nb = 80: NBT = 5
            (3, 5, 5), (4, 3, 3),
            (5, 4, 4),           # T = 1100: 18 chunks -> 5, 5, 5, 3
            (5, 7, 6)]


def _grads(inp, grad_segments):
    qd, kd, vd, pd, Wd, gd = _device_inputs(inp)
    out = ops.performer_value_autograd(qd, kd, vd, pd, Wd, grad_segments=grad_segments)
    grads = torch.autograd.grad(out, [qd, kd, vd, pd], grad_outputs=gd)
    torch.cuda.synchronize()
    return grads


@pytest.mark.gpu
@pytest.mark.parametrize("idx,requested,effective", SEGMENTS, ids=[f"{_id(CASES[i])}-seg{r}" for i, r, _e in SEGMENTS])
def test_segmented_kernels_against_fp64_reference(idx, requested, effective):
    N, H, T, D, nb, dt, _seed = CASES[idx]
    assert _lib.load().sea_performer_causal_bwd_seg_count(T, requested) == effective
    inp, ref, _yard, amb, bars = _case(idx)
    got = _grads(inp, requested)
    failures = []
    for i, name in enumerate(NAMES):
        x = got[i].cpu()
        assert x.dtype == dt and x.shape == inp[i].shape and torch.isfinite(x).all(), name
        err = (_kept(x, i, amb) - _kept(ref[i], i, amb)).abs().max().item()
        print(f"[perf-bwd-seg] {_id(CASES[idx])} segments {requested} -> {effective} {name}: max err {err:.3e} bar {bars[i]:.3e} "
              f"ratio {err / bars[i]:.3f}")
        if not err <= bars[i]:
            failures.append((name, err, bars[i]))
    assert not failures, failures
    for a, b in zip(got, _grads(inp, requested)):                              # one summation order: the same bits
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_one_segment_is_bitwise_the_unsegmented_backward():
    inp = _case(1)[0]
    for a, b in zip(_grads(inp, None), _grads(inp, 1)):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_layer_with_two_segments(layer_and_inputs, monkeypatch):
    """The two rules test_gpu_performer_bwd.py holds the unsegmented switch to.  Wiring: with the module's own FastAttention behind
    the op's name, the loss and every parameter gradient are bitwise those of the switch-off torch step, and the op was handed the
    layer's `fused_performer_grad_segments`.  Numbers: with the kernels, the loss and the gradients that file holds (the value
    embedding, which the backward reaches, and the first encoder weight) against the step with the fp64 Performer standing in, the
    switch-off step as yardstick.  (The other parameters' gradients depend on the op's forward alone, which is not touched.)"""
    att = layer_and_inputs[0].attention
    assert att.fused_performer_grad_segments is None
    loss_y, g_y = _step(layer_and_inputs, False)
    lib, calls, handed = _lib.load(), [], []
    real, stand_in = lib.sea_performer_causal_bwd_seg, _torch_stand_in(att)
    monkeypatch.setattr(lib, "sea_performer_causal_bwd_seg", lambda *a: calls.append(a[20]) or real(*a))
    att.fused_performer_grad_segments = 2
    try:
        with monkeypatch.context() as m:
            m.setattr(ops, "performer_value_autograd",
                      lambda *a, grad_segments=None, **kw: handed.append(grad_segments) or stand_in(*a, **kw))
            loss_w, g_w = _step(layer_and_inputs, True)
        assert handed == [2] and calls == [] and torch.equal(loss_w, loss_y) and sorted(g_w) == sorted(g_y)
        for n in g_y:
            assert torch.equal(g_w[n], g_y[n]), n
        loss_k, g_k = _step(layer_and_inputs, True)
    finally:
        att.fused_performer_grad_segments = None
    assert calls == [2]
    with monkeypatch.context() as m:
        m.setattr(ops, "performer_value_autograd",
                  lambda q, k, v, pos, projection, n_segments=None: _RefPerformer.apply(q, k, v, pos, projection))
        loss_r, g_r = _step(layer_and_inputs, True)
    held = ("v_eye_learned_causal", "attention_predictor_enc.0.weight")
    failures = []
    for name, got, yard, ref in [("loss", loss_k, loss_y, loss_r)] + [(f"d {n}", g_k[n], g_y[n], g_r[n]) for n in held]:
        ref = ref.double().cpu()
        bar = bar_of(yard.double().cpu(), ref)
        err = (got.double().cpu() - ref).abs().max().item()
        print(f"[perf-bwd-seg] layer {name}: max err {err:.3e} bar {bar:.3e} ratio {err / bar:.3f}")
        if not (torch.isfinite(got).all() and err <= bar):
            failures.append((name, err, bar))
    assert not failures, failures
