"""A whole fused training step of `PerlinAttention` on the HIP kernels: all switches at once, batches, padding, optimizer steps
(DESIGN 5.14).  The four backward ops -- `ops.performer_value_autograd` (5.10), `ops.predictor_tail_autograd` (5.11),
`ops.causal_conv_relu_autograd` (5.12), `ops.predictor_mlp_autograd` (5.13) -- each have an op tier and a layer tier in which ONE op
is exchanged on one H = 4, N = 1 layer.  Here the chain runs as a chain.

Whole-step tier.  Three runs of `PerlinAttention.forward` + `loss.backward()` per layer, one teacher score tensor, no context truth:
    got   every switch on (the two KD-loss switches and the four grad switches);
    yard  the four grad switches off, the KD switches on: the torch chain in the data type, the yardstick of 5.10 - 5.13;
    ref   the switches of `got`, all four ops replaced at once by the fp64 stand-ins of their own test files.
The KD-loss kernels are the same in the three runs (5.7 - 5.9 hold them to fp64).  Compared per quantity -- the loss, every parameter
gradient, every input gradient (q / k / v and the *_for_atten / *_for_score leaves) -- under 5.7's rule `err <= bar_of(yard, ref)`.
The backward runs with the upstream gradient g = N H T, `(loss * g).backward()` in the three runs alike, as in 5.8's tests: the
loss is a mean over N H T rows, and without it the activations' gradients of the fp16 layer lie in fp16's subnormal range (below
6.1e-5), where a rounding is 2^-24 absolute, not eps / 2 relative, and kernels and yardstick are compared on quantisation noise.
Rows of q_for_atten / k_for_atten with a Performer feature inside four fp32 worst-case errors of the ReLU's kink are left out of
those two gradients, as in 5.10's op tier (at most 3 % of the rows, asserted before any run).  Both are departures from a plain
`loss.backward()` on every row, taken from 5.8's and 5.10's practice.

The loss is a continuous function of the ops' outputs (read in `forward`, `_forward_sparse`, `_forward_dense`): sparse mode's loss is
`ops.kd_estimator_loss(estimated_attention_score)` + `ops.kd_score_loss(q_for_score, k_for_score)`; `_forward_sparse`, where the
top-k selection lives, returns the context alone, and the context term `F.mse_loss(context_layer_truth, ...)` is the only reader of
it -- absent without a context truth.  Dense mode's loss is `_kl_and_mse` of `resize_from_m_to_t(estimated_attention_score)` -- a
gather whose indices come from the mask alone, no jitter under `.eval()` -- and `_forward_dense`'s `_kl_and_mse` of q k^T; its sort
and `partial_attention_mask` feed the context only.  So no term depends on the discrete selection and a near-tie cannot flip a
result; consequently q and k (the layer's own, which only the attention reads) get no gradient in any run.

Witnesses.  `bar_of` alone cannot see a wrong reference: a fault of size f in `ref` moves `err` by f and the bar by 4 f, so err / bar
tends to 1/4 as f grows.  The reference is therefore itself held, per quantity and by the same rule, to a fourth run that shares
nothing with the other three (`_wide`: the layer's torch chain in fp32 and dense mode, every switch off, on the same 16-bit values):
`|ref - wide| <= bar_of(yard, wide)`, four times the yardstick's distance from that run.  Not a tighter clause: the stand-in chain is
not nearer to the fp32 run than the torch chain is, because both round to the data type at the ops' edges and those roundings,
amplified by the chain, are most of either distance.  Known limit: the clause sees a reference fault above four times the
yardstick's own distance from the fp32 run and no smaller one; of the two witnesses, the MLP's d_x times 1 + 2^-3 is NOT seen in d v
of layer A, where the yardstick itself is that far off, so for that quantity the tier stays blind to a 12.5 % fault of the reference.

Across optimizer steps: both passes take their packed weight images from `ops.predictor._cached`, whose entries are valid while the
parameters' `_version` stands.  A layer takes three optimizer steps with no `ops.clear_prep_cache()` anywhere in that span; only
then a twin takes the same steps clearing the one global cache before every forward; the two must agree bit for bit and each step
must build each image once.  A third run under a `_cached` that ignores `_version` must be reported by the same checks.

[step] lines print err, bar and their ratio per quantity and the distances from the fp32 run; the MI355X values are in DESIGN.md
5.14."""
import copy
import functools
import math

import pytest
import torch

import sea_attention_amd as S
from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from sea_attention_amd.perlin_attention.ops import predictor as predictor_ops
from sea_attention_amd.perlin_attention.ops import performer_grad, predictor_cnn_grad
from sea_attention_amd.perlin_attention.ops.kd_score_loss import KD_SCORE_HEAD_SIZES
from test_gpu_kd_score_loss import padded_mask
from test_gpu_performer_bwd import _RefPerformer
from test_gpu_predictor_cnn_bwd import _RefConvRelu
from test_gpu_predictor_mlp_bwd import _RefMlp
from test_gpu_predictor_tail_bwd import Cfg, D_, _layer_and_inputs, _ref_stand_in
from test_performer_bwd_reference import ambiguous_rows
from test_predictor_tail_bwd_reference import bar_of

DEV = "cuda"
F16, BF = torch.float16, torch.bfloat16
K_ = 8
GRAD_SWITCHES = ("fused_performer_grad", "fused_tail_grad", "fused_cnn_grad", "fused_mlp_grad")
KD_SWITCHES = ("fused_kd_loss", "fused_kd_score_loss")
ENTRIES = ("sea_performer_causal_bwd", "sea_predictor_tail_bwd", "sea_causal_conv_relu_bwd", "sea_predictor_mlp_bwd",
           "sea_kd_estimator_loss_bwd", "sea_kd_score_loss_bwd")
#            N  H   d   T   T_M dtype sparse padded rows of item 1, v_for_atten apart from v, calls per step of ENTRIES
LAYERS = {"A": (2, 12, 64, 80, 64, F16, True, 0, False, (1, 1, 2, 1, 1, 1)),     # three channel groups, W = 16
          "B": (2, 32, 64, 48, 128, BF, True, 0, True, (1, 1, 2, 1, 1, 1)),      # eight channel groups, W = 32, the torch.cat branch
          "C": (2, 4, 64, 96, 32, BF, False, 24, False, (0, 1, 2, 1, 0, 0))}     # dense mode, padded: no Performer, no fused KD
INPUTS = ("q", "k", "v", "q_for_atten", "k_for_atten", "v_for_atten", "q_for_score", "k_for_score")


def test_the_kernels_take_layers_a_to_c():
    """On the CPU, from the library's own predicates: every op of the chain has a form for each layer's shapes."""
    lib = _lib.load()
    for tag, (N, H, d, T, T_M, dt, _sparse, _pad, _split, _calls) in LAYERS.items():
        code, C, W = _lib.dtype_code(dt), 2 * H, T_M // 4
        nb = int(d * math.log(d) / _pconfig(T_M).performer_nb_factor)           # `PerlinAttention.performer_nb_features`
        assert lib.sea_performer_causal_bwd_supported(d, nb, code), tag
        assert lib.sea_predictor_tail_bwd_supported(C, H, W, 4, T_M, code), tag
        assert lib.sea_causal_conv_relu_bwd_supported(C, W, 3, 2, 2, code), tag
        assert lib.sea_predictor_mlp_bwd_supported(2 * d, 2 * W, H, 3 * d, code), tag
        assert ops.predictor_mlp_supported(2 * d, 2 * W, H, 3 * d) and ops.performer_supported(d, nb, dt), tag
        # the two KD losses: 16-byte rows of the (T, T) truth and of the (T, T_M) map, head size 64
        assert (T * 2) % 16 == 0 and (T_M * 2) % 16 == 0 and T_M % 4 == 0 and d in KD_SCORE_HEAD_SIZES
    assert LAYERS["A"][1] * 2 // 8 == 3 and LAYERS["B"][1] * 2 // 8 == 8 and all(v[0] > 1 for v in LAYERS.values())


def _pconfig(T_M):
    return PerlinAttentionConfig(k=K_, attention_predictor_length=T_M, performer_nb_factor=8, causal=True, k_flatten=True,
                                 k_flatten_dim='causal_batch', context_output_method='mix')


@functools.lru_cache(maxsize=None)
def _layer(tag):
    """(layer, the eight input values, mask, teacher scores, rows left out of d q_for_atten / d k_for_atten)"""
    N, H, d, T, T_M, dt, sparse, pad, split, _calls = LAYERS[tag]
    S.seed(42)
    layer = PerlinSelfAttention(Cfg(H * d, H, T), _pconfig(T_M)).to(DEV).to(dt).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = sparse
    S.seed(1)
    r = lambda: torch.randn((N, H, T, d), device=DEV)
    x = r()
    val = {"q": x * d ** -0.5, "k": x, "v": x, "q_for_atten": x * d ** -0.5, "k_for_atten": x, "q_for_score": x * d ** -0.5,
           "k_for_score": x}
    if split:
        val["v_for_atten"] = r()
    val = {n: t.to(dt) for n, t in val.items()}
    idx = torch.arange(T, device=DEV)
    mask = ((idx.view(1, T) > idx.view(T, 1)) * (torch.finfo(F16).min / 2)).view(1, 1, T, T).to(dt).expand(N, 1, T, T).contiguous()
    if pad:
        mask = padded_mask(mask, pad, items=1)
    truth = (torch.randn((N, H, T, T), device=DEV) * 2.0).to(dt)
    W = layer.attention.performer.projection_matrix.detach().cpu()
    amb = {n: ambiguous_rows(val[n].cpu(), W) for n in ("q_for_atten", "k_for_atten")}
    for a in amb.values():                                                     # on the reference side, before any run
        assert a.float().mean().item() <= 0.03, a.float().mean().item()
    return layer, val, mask, truth, amb


def _step(tag, grad_switches, patches=()):
    """One training step of `PerlinAttention.forward`, called directly: {"loss", "d <parameter>", "in <input>"}"""
    layer, val, mask, truth, _amb = _layer(tag)
    att = layer.attention
    leaf = {n: t.clone().requires_grad_(True) for n, t in val.items()}
    leaf.setdefault("v_for_atten", leaf["v"])                                  # the layer's own v unless the branch is apart
    layer.zero_grad()
    with pytest.MonkeyPatch.context() as m:
        for name, f in patches:
            m.setattr(ops, name, f)
        for s in KD_SWITCHES:
            setattr(att, s, True)
        for s in GRAD_SWITCHES:
            setattr(att, s, grad_switches)
        try:
            out = att(*(leaf[n] for n in INPUTS), mask, truth, None)
            # not a plain `loss.backward()`: g = N H T, in all runs alike, keeps the fp16 layer's gradients out of the subnormals
            (out.loss * float(LAYERS[tag][0] * LAYERS[tag][1] * LAYERS[tag][3])).backward()
        finally:
            for s in KD_SWITCHES + GRAD_SWITCHES:
                setattr(att, s, False)
    torch.cuda.synchronize()
    res = {"loss": out.loss.detach().clone()}
    res.update({f"d {n}": p.grad.detach().clone() for n, p in att.named_parameters() if p.grad is not None})
    res.update({f"in {n}": leaf[n].grad.detach().clone() for n in val if leaf[n].grad is not None})
    return res


def _ref_patches(conv=_RefConvRelu, mlp=_RefMlp):
    return (("performer_value_autograd", lambda q, k, v, pos, projection, n_segments=None: _RefPerformer.apply(q, k, v, pos, projection)),
            ("predictor_tail_autograd", _ref_stand_in),
            ("causal_conv_relu_autograd", lambda x8, w, b, k, d, pad: conv.apply(x8, w, b, d)),
            ("predictor_mlp_autograd", lambda x_, e, ln, d, l1, sc, want_tpred=True: mlp.apply(
                x_, e.weight, e.bias, ln.weight, ln.bias, d.weight, d.bias, l1.weight, l1.bias)))


@functools.lru_cache(maxsize=None)
def _runs(tag):
    """(got, yard, ref, calls of ENTRIES in got, in yard, in ref): computed once per layer, shared with the witnesses, never changed"""
    lib, calls = _lib.load(), {e: 0 for e in ENTRIES}
    with pytest.MonkeyPatch.context() as m:
        for e in ENTRIES:
            def spy(*a, _e=e, _real=getattr(lib, e)):
                calls[_e] += 1
                return _real(*a)
            m.setattr(lib, e, spy)
        yard = _step(tag, False)
        in_yard = tuple(calls[e] for e in ENTRIES)
        got = _step(tag, True)
        in_got = tuple(calls[e] - y for e, y in zip(ENTRIES, in_yard))
        ref = _step(tag, True, _ref_patches())
        in_ref = tuple(calls[e] - y - g for e, y, g in zip(ENTRIES, in_yard, in_got))
    return got, yard, ref, in_got, in_yard, in_ref


@functools.lru_cache(maxsize=None)
def _wide(tag):
    """The same step once more with nothing of the other three runs in it: a copy of the layer in fp32 and DENSE mode, every switch
    off (torch modules and `_kl_and_mse` throughout, no HIP backward, no stand-in), the 16-bit parameters, inputs and teacher scores
    as fp32 values.  Dense mode's two loss terms are the two expressions the fused KD kernels of sparse mode evaluate (5.7, 5.8)."""
    layer, val, mask, truth, _amb = _layer(tag)
    wide = copy.deepcopy(layer).float().eval()
    for m in wide.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = False
    att = wide.attention
    assert not any(getattr(att, s) for s in KD_SWITCHES + GRAD_SWITCHES)
    leaf = {n: t.float().clone().requires_grad_(True) for n, t in val.items()}
    leaf.setdefault("v_for_atten", leaf["v"])
    out = att(*(leaf[n] for n in INPUTS), mask.float(), truth.float(), None)
    (out.loss * float(LAYERS[tag][0] * LAYERS[tag][1] * LAYERS[tag][3])).backward()
    torch.cuda.synchronize()
    res = {"loss": out.loss.detach().clone()}
    res.update({f"d {n}": p.grad.detach().clone() for n, p in att.named_parameters() if p.grad is not None})
    res.update({f"in {n}": leaf[n].grad.detach().clone() for n in val if leaf[n].grad is not None})
    return res


def _conv4_bias(att):
    """name of the one gradient that is zero by construction: the tail's LayerNorm removes what the 1x1 convolution's bias adds (5.11)"""
    conv4 = list(att.attention_predictor_cnn[1].module.net.children())[-1].module
    return "d " + {id(p): n for n, p in att.named_parameters()}[id(conv4.bias)]


def _compare(tag, got, yard, ref):
    """[(quantity, what, err, bar, reference to the fp32 run, yardstick to the fp32 run)] of every quantity that is not finite or
    outside its bar (what = "kernel") or whose reference is outside `bar_of(yard, wide)` of the independent fp32 run ("reference")"""
    dt, amb = LAYERS[tag][5], _layer(tag)[4]
    zero, wide = _conv4_bias(_layer(tag)[0].attention), _wide(tag)
    assert sorted(wide) == sorted(ref)
    failures = []
    for n in sorted(ref):
        g, y, r, w = (t[n].double().cpu() for t in (got, yard, ref, wide))
        # deliberate: only d q_for_atten / d k_for_atten leave their own kink rows out (there a flipped ReLU side changes the row's
        # gradient by a whole feature); the parameter gradients and d v still sum over those rows, whose features are continuous
        if n[3:] in amb and n.startswith("in "):
            g, y, r, w = (t[~amb[n[3:]]] for t in (g, y, r, w))
        err, yerr, top = (g - r).abs().max().item(), (y - r).abs().max().item(), r.abs().max().item()
        bar = bar_of(y, r)
        unit = max(torch.finfo(dt).eps * w.abs().max().item(), 1e-300)
        r_w, y_w = (r - w).abs().max().item(), (y - w).abs().max().item()
        print(f"[step] layer {tag} {n}: max err {err:.3e} bar {bar:.3e} ratio {err / max(bar, 1e-300):.3f} (max |ref| {top:.3e}, "
              f"yardstick {0.0 if n == zero else yerr / max(torch.finfo(dt).eps * top, 1e-300):.2f} eps; from the fp32 run: reference "
              f"{r_w / unit:.2f} eps, yardstick {y_w / unit:.2f} eps)")
        sound = r_w <= bar_of(y, w)                                            # 5.7's rule once more: the reference under it
        if not (torch.isfinite(got[n]).all() and err <= bar):
            failures.append((n, "kernel", err, bar, r_w, y_w))
        if not sound:
            failures.append((n, "reference", err, bar, r_w, y_w))
    return failures


@pytest.mark.gpu
@pytest.mark.parametrize("tag", sorted(LAYERS))
def test_whole_step_against_the_fp64_chain(tag):
    split, want_calls = LAYERS[tag][8], LAYERS[tag][9]
    got, yard, ref, in_got, in_yard, in_ref = _runs(tag)
    print(f"[step] layer {tag} calls per step {dict(zip(ENTRIES, in_got))}")
    assert in_got == want_calls, dict(zip(ENTRIES, in_got))
    assert in_yard == (0, 0, 0, 0) + want_calls[4:] and in_ref == (0, 0, 0, 0) + want_calls[4:]    # the KD kernels: in all three
    assert sorted(got) == sorted(yard) == sorted(ref)
    inputs = {"in v", "in q_for_atten", "in k_for_atten", "in q_for_score", "in k_for_score"} | ({"in v_for_atten"} if split else set())
    assert {n for n in got if n.startswith("in ")} == inputs                   # q and k: read by the attention alone
    for n in ("d v_eye_learned_causal", "d attention_predictor_enc.0.weight", "d attention_predictor_dec_row.0.weight"):
        assert n in got, n
    for n in ref:
        assert ref[n].abs().max().item() > 0 or n == _conv4_bias(_layer(tag)[0].attention), n
    failures = _compare(tag, got, yard, ref)
    assert not failures, failures


class _NoMaskConvRelu(_RefConvRelu):
    """witness (i): the backward takes y > 0 everywhere"""

    @staticmethod
    def forward(ctx, x8, w, b, d):
        out = _RefConvRelu.forward(ctx, x8, w, b, d)
        x, w3, y, d_ = ctx.args
        ctx.args = (x, w3, torch.ones_like(y), d_)
        return out


class _ScaledDxMlp(_RefMlp):
    """witness (ii): d_x is 1 + 2^-3 times too large"""

    @staticmethod
    def backward(ctx, g8, g_tp):
        dx, *rest = _RefMlp.backward(ctx, g8, g_tp)
        return (dx * (1 + 2.0 ** -3), *rest)


@pytest.mark.gpu
@pytest.mark.parametrize("fault", ("conv-relu-mask", "mlp-dx"))
def test_a_wrong_reference_is_reported(fault):
    """The bar alone passes both (err / bar 0.25: the module docstring); the comparison with the independent fp32 run reports them, and
    reports them as faults of the reference, not of the kernels.  Known limit, asserted as it is: the scaled d_x is not seen in d v."""
    got, yard, *_rest = _runs("A")
    patches = _ref_patches(conv=_NoMaskConvRelu) if fault == "conv-relu-mask" else _ref_patches(mlp=_ScaledDxMlp)
    bad = _step("A", True, patches)
    assert sorted(bad) == sorted(got)
    failures = _compare("A", got, yard, bad)
    print(f"[step] witness {fault}: " + " ".join(f"{f[0]} ({f[1]})" for f in failures))
    assert failures and all(f[1] == "reference" for f in failures)
    reached = {f[0] for f in failures}
    if fault == "mlp-dx":                                                      # below the MLP's input, and nothing above it
        assert {"in q_for_atten", "in k_for_atten", "d v_eye_learned_causal"} <= reached <= {
            "in q_for_atten", "in k_for_atten", "in v", "d v_eye_learned_causal"}, reached
    else:                                                                      # everything below conv2's output
        assert len(reached) >= 14 and "d attention_predictor_enc.0.weight" in reached and "in v" in reached, reached


# ---- across optimizer steps: 5.11's layer, bf16, sparse mode, all six switches ------------------------------------------------
# SGD: the LayerNorm weights start at exactly 1, where one bf16 step is 2^-7, and their largest gradient in the first step is
# 1.6e-3 .. 6.8e-3 (printed below): lr = 8 moves each of them by more than a step.  AdamW: a first step of lr * sign(g) = 2^-6.6
OPTIMIZERS = {"sgd": lambda ps: torch.optim.SGD(ps, lr=8.0), "adamw": lambda ps: torch.optim.AdamW(ps, lr=1e-2)}
STEPS = 3


def _train(opt_name, clear, version_blind=False):
    """STEPS optimizer steps of a `copy.deepcopy` of 5.11's layer (the cached layer itself is not stepped), one after the other:
    per step (loss, {parameter: gradient}, (builds of conv images, builds of MLP images), parameters the step left unchanged).
    `clear`: `ops.clear_prep_cache()` before every forward; otherwise the cache is not cleared anywhere in the span.
    `version_blind`: `_cached` stands in as it would be without its `_version` comparison."""
    base, x, mask, truth = _layer_and_inputs(BF)
    builds = {"conv": 0, "mlp": 0}
    real_pack, real_frag = predictor_ops.pack_conv_weight, predictor_ops._pack_a_fragments

    def pack(*a):
        builds["conv"] += 1
        return real_pack(*a)

    def frag(*a, **kw):                                                        # `mlp_images`' build packs W1 and W2: two calls
        builds["mlp"] += 1
        return real_frag(*a, **kw)
    held = {}

    def blind(tag, tensors, dtype, build):
        key = (tag, dtype) + tuple((id(t._base if t._base is not None else t), t.data_ptr(), tuple(t.shape), tuple(t.stride()))
                                   for t in tensors)
        if key not in held:
            held[key] = (build(), tensors)                                     # (the tensors: their ids stay theirs)
        return held[key][0]
    layer = copy.deepcopy(base)
    att = layer.attention
    opt = OPTIMIZERS[opt_name](list(layer.parameters()))
    q = x * D_ ** -0.5
    zero_name = _conv4_bias(att)[2:]
    steps = []
    with pytest.MonkeyPatch.context() as m:
        m.setattr(predictor_ops, "pack_conv_weight", pack)
        m.setattr(predictor_cnn_grad, "pack_conv_weight", pack)
        m.setattr(predictor_ops, "_pack_a_fragments", frag)
        if version_blind:
            for mod in (predictor_ops, predictor_cnn_grad, performer_grad):
                m.setattr(mod, "_cached", blind)
        for s in KD_SWITCHES + GRAD_SWITCHES:
            setattr(att, s, True)
        for step in range(STEPS):
            if clear:
                ops.clear_prep_cache()
            before = dict(builds)
            opt.zero_grad(set_to_none=True)
            out = att(q, x.clone(), x.clone(), q, x.clone(), x.clone(), q, x.clone(), mask, truth, None)
            out.loss.backward()
            torch.cuda.synchronize()
            grads = {n: p.grad.detach().clone() for n, p in att.named_parameters() if p.grad is not None}
            old = {n: p.detach().clone() for n, p in att.named_parameters() if n in grads}
            opt.step()
            still = [n for n, p in att.named_parameters() if n in grads and n != zero_name and torch.equal(p.detach(), old[n])]
            steps.append((out.loss.detach().clone(), grads, (builds["conv"] - before["conv"], builds["mlp"] - before["mlp"]), still))
    torch.cuda.synchronize()
    return steps


def _problems(run, cleared, zero_name):
    """what the tier checks of a run against the twin that cleared the cache before every forward"""
    found = []
    for step, ((loss, grads, built, still), (loss_c, grads_c, built_c, _still)) in enumerate(zip(run, cleared)):
        # one build per weight set per step -- two (conv, ReLU) pairs, one MLP of two packs -- and none in the backward
        if built != (2, 2) or built_c != (2, 2):
            found.append(("builds", step, built, built_c))
        if still:                                                              # every parameter that receives a gradient moves
            found.append(("parameter unchanged", step, still))
        if not (torch.isfinite(loss) and torch.equal(loss, loss_c)):
            found.append(("loss", step, loss.item(), loss_c.item()))
        if sorted(grads) != sorted(grads_c) or len(grads) <= 10:
            found.append(("gradient names", step))
        else:
            found += [("gradient", step, n) for n in grads if not torch.equal(grads[n], grads_c[n])]
        if [n for n in grads if grads[n].abs().max().item() == 0] != [zero_name]:     # conv4's bias alone: exactly zero (5.11)
            found.append(("zero gradients", step))
    if len({s[0].item() for s in run}) != len(run):
        found.append(("loss does not move", [s[0].item() for s in run]))
    return found


@functools.lru_cache(maxsize=None)
def _cleared(opt_name):
    return _train(opt_name, clear=True)


@pytest.mark.gpu
@pytest.mark.parametrize("opt_name", sorted(OPTIMIZERS))
def test_packed_images_follow_the_optimizer(opt_name):
    plain = _train(opt_name, clear=False)
    cleared = _cleared(opt_name)
    print(f"[step] {opt_name} losses {[s[0].item() for s in plain]} builds {[s[2] for s in plain]}")
    found = _problems(plain, cleared, _conv4_bias(_layer_and_inputs(BF)[0].attention)[2:])
    assert not found, found


@pytest.mark.gpu
def test_a_cache_that_ignores_the_version_is_reported():
    """Witness: with `_cached` blind to `_version` the same span trains on the first step's images; the checks must say so."""
    stale = _train("sgd", clear=False, version_blind=True)
    found = _problems(stale, _cleared("sgd"), _conv4_bias(_layer_and_inputs(BF)[0].attention)[2:])
    print(f"[step] version-blind cache: {[f[:2] for f in found]}")
    kinds = {(f[0], f[1]) for f in found}
    assert ("builds", 1) in kinds and ("builds", 2) in kinds and ("loss", 1) in kinds and ("loss", 2) in kinds, found
    assert ("loss", 0) not in kinds and not any(f[0] == "gradient" and f[1] == 0 for f in found), found    # step 0 is sound
