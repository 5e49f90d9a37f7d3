"""The mathematics of the causal Performer's backward, on the CPU in fp64.

`PerformerReference` evaluates the chunked forms csrc/sea_performer_bwd.hip computes -- a forward sweep carrying the state, a
reverse sweep carrying R, the per-chunk triangular products -- and is held here to fp64 autograd through `performer.py`'s own
feature map and `causal_linear_attention(..., chunk=T)`.  (`chunk=T`: with the default chunk of 128 and T >= 128, T % 128 != 0, the
padded rows of the last chunk have den = 0 and autograd returns NaN for k and v; that path is existing behaviour)
The GPU tests (test_gpu_performer_bwd.py) take the reference, the yardstick, the bar and the ambiguity rule from this file."""
import functools

import pytest
import torch

from sea_attention_amd.perlin_attention.performer import FastAttention, causal_linear_attention

F64 = torch.float64


class PerformerReference:
    """fp64.  `chunk`: rows per chunk.  Two deliberate faults, for the witnesses: `drop_carry_at` = index of a chunk whose R is
    NOT handed to the chunk below it; `leak_padded_features` = the features are padded to a multiple of 16 and the padding keeps
    phi = 1e-3 instead of 0."""

    def __init__(self, chunk=64, drop_carry_at=None, leak_padded_features=False):
        self.C, self.drop, self.leak = chunk, drop_carry_at, leak_padded_features

    def _features(self, x, W):
        s = x.shape[-1] ** -0.25
        pre = (s * x) @ W.t()
        phi = torch.relu(pre) + 1e-3
        if self.leak:
            pad = (-W.shape[0]) % 16
            phi = torch.cat([phi, torch.full((*phi.shape[:-1], pad), 1e-3, dtype=phi.dtype)], -1)
            pre = torch.cat([pre, torch.zeros((*pre.shape[:-1], pad), dtype=pre.dtype)], -1)
        return phi, (pre > 0).to(x.dtype)

    def _prepare(self, q, k, v, pos, W):
        q, k, v, pos, W = (t.to(F64) for t in (q, k, v, pos, W))
        T = q.shape[-2]
        a, ma = self._features(q, W)
        b, mb = self._features(k, W)
        vh = torch.cat([pos[:T].expand(v.shape), v, torch.ones_like(v[..., :1])], -1)            # [pos | v | 1]
        return q, k, v, W, a, ma, b, mb, vh

    def _forward_sweep(self, a, b, vh, visit):
        *lead, T, F = a.shape
        S = torch.zeros((*lead, F, vh.shape[-1]), dtype=F64)
        for t0 in range(0, T, self.C):
            sl = slice(t0, min(T, t0 + self.C))
            visit(sl, S)
            S = S + b[..., sl, :].transpose(-1, -2) @ vh[..., sl, :]

    def forward(self, q, k, v, pos, W):
        q, k, v, W, a, ma, b, mb, vh = self._prepare(q, k, v, pos, W)
        E = vh.shape[-1] - 1
        out = torch.empty((*v.shape[:-1], E + v.shape[-1]), dtype=F64)

        def visit(sl, S):
            A = torch.tril(a[..., sl, :] @ b[..., sl, :].transpose(-1, -2))
            nz = A @ vh[..., sl, :] + a[..., sl, :] @ S
            den = nz[..., E] + 1e-6 * a[..., sl, :].sum(-1)
            out[..., sl, :E] = nz[..., :E] / den.unsqueeze(-1)
        self._forward_sweep(a, b, vh, visit)
        out[..., E:] = v
        return out

    def backward(self, q, k, v, pos, W, g):
        """(dq, dk, dv, dpos); dpos has pos's shape, rows at or beyond T are 0."""
        q, k, v, W, a, ma, b, mb, vh = self._prepare(q, k, v, pos, W)
        g = g.to(F64)
        T, D = q.shape[-2:]
        E = 2 * D
        s = D ** -0.25
        gh = torch.empty_like(vh)
        da, db, dvh = torch.empty_like(a), torch.empty_like(b), torch.empty_like(vh)

        def visit(sl, S):
            ac, bc, vc = a[..., sl, :], b[..., sl, :], vh[..., sl, :]
            A = torch.tril(ac @ bc.transpose(-1, -2))
            nz = A @ vc + ac @ S
            den = (nz[..., E] + 1e-6 * ac.sum(-1)).unsqueeze(-1)
            ctx = nz[..., :E] / den
            gc = torch.cat([g[..., sl, :E] / den, -(g[..., sl, :E] * ctx).sum(-1, keepdim=True) / den], -1)
            gh[..., sl, :] = gc
            B = torch.tril(gc @ vc.transpose(-1, -2))
            da[..., sl, :] = B @ bc + gc @ S.transpose(-1, -2) + 1e-6 * gc[..., E:]
        self._forward_sweep(a, b, vh, visit)

        R = torch.zeros((*a.shape[:-2], a.shape[-1], E + 1), dtype=F64)
        starts = list(range(0, T, self.C))
        for ci in reversed(range(len(starts))):                        # the partial chunk first
            sl = slice(starts[ci], min(T, starts[ci] + self.C))
            ac, bc, vc, gc = a[..., sl, :], b[..., sl, :], vh[..., sl, :], gh[..., sl, :]
            A = torch.tril(ac @ bc.transpose(-1, -2))
            B = torch.tril(gc @ vc.transpose(-1, -2))
            db[..., sl, :] = B.transpose(-1, -2) @ ac + vc @ R.transpose(-1, -2)
            dvh[..., sl, :] = A.transpose(-1, -2) @ gc + bc @ R
            R = R + ac.transpose(-1, -2) @ gc
            if self.drop is not None and ci == self.drop:
                R = torch.zeros_like(R)
        F = W.shape[0]
        dq = s * ((da * ma)[..., :F] @ W)
        dk = s * ((db * mb)[..., :F] @ W)
        dv = dvh[..., D:E] + g[..., E:]
        dpos = torch.zeros(pos.shape, dtype=F64)
        dpos[:T] = dvh[..., :D].reshape(-1, T, D).sum(0)
        return dq, dk, dv, dpos


def performer_py(q, k, v, pos, W, g, dtype):
    """`performer.py` itself under autograd in `dtype` (fp64: the truth of this file; fp32: the GPU tests' yardstick): its
    feature map, `causal_linear_attention(chunk=T)` and the two concatenations.  Returns (out, dq, dk, dv, dpos)."""
    D, T = q.shape[-1], q.shape[-2]
    fa = FastAttention(dim_heads=D, nb_features=W.shape[0], causal=True, generalized_attention=True)
    fa.projection_matrix = W.to(dtype)
    q, k, v, pos = (t.detach().to(dtype).requires_grad_(True) for t in (q, k, v, pos))
    vfa = torch.cat([pos[:T].expand(v.shape), v], -1)
    ctx = causal_linear_attention(fa.feature_map(q), fa.feature_map(k), vfa, chunk=T)
    out = torch.cat([ctx, v], -1)
    grads = torch.autograd.grad(out, [q, k, v, pos], grad_outputs=g.to(dtype))
    return (out.detach(), *grads)


def make_inputs(N, H, T, D, nb, seed, dtype=torch.float64, qk_scale=1.0):
    """q, k, v, pos (T + 3 rows), W, g as `dtype` values (rounded there, so that every path starts from the same numbers).
    `qk_scale` < 1 makes the ReLU part of the features small, so that the 1e-3 every feature carries weighs in the sums."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=gen, dtype=F64)
    q, k, v, g = qk_scale * r(N, H, T, D), qk_scale * r(N, H, T, D), r(N, H, T, D), r(N, H, T, 3 * D)
    pos = r(T + 3, D)
    W = r(nb, D)
    return tuple(t.to(dtype) for t in (q, k, v, pos, W, g))


def ambiguous_rows(x, W):
    """(..., T) bool: rows of x for which some feature's pre-activation lies within four times the fp32 worst case of its own dot
    product of zero -- |s x.w_f| <= 4 D 2^-24 s sum_i |x_i| |w_fi| -- so that fp32 arithmetic may take the other side of the ReLU."""
    x, W = x.to(F64), W.to(F64)
    D = x.shape[-1]
    return ((x @ W.t()).abs() <= 4 * D * 2.0 ** -24 * (x.abs() @ W.abs().t())).any(-1)


def bar_of(yard, ref):
    """4 x the yardstick's largest error, at least 2^-22 of the reference's largest magnitude (DESIGN 5.7's rule)."""
    return max(4 * (yard.to(F64) - ref).abs().max().item(), 2.0 ** -22 * ref.abs().max().item())


T_S, NB_S, D_S = (1, 63, 64, 65, 200), (17, 33, 80), (64, 80, 128)


@functools.lru_cache(maxsize=None)
def _truth(T, nb, D):
    inp = make_inputs(1, 2, T, D, nb, seed=1000 * T + 10 * nb + D)
    return inp, performer_py(*inp, F64)


@pytest.mark.parametrize("C", (32, 64))
@pytest.mark.parametrize("D", D_S)
@pytest.mark.parametrize("nb", NB_S)
@pytest.mark.parametrize("T", T_S)
def test_chunked_forms_against_fp64_autograd(T, nb, D, C):
    (q, k, v, pos, W, g), (out, *want) = _truth(T, nb, D)
    ref = PerformerReference(chunk=C)
    got_out = ref.forward(q, k, v, pos, W)
    assert (got_out - out).abs().max() <= 1e-12 * out.abs().max()
    got = ref.backward(q, k, v, pos, W, g)
    for name, a, b in zip(("dq", "dk", "dv", "dpos"), got, want):
        assert a.shape == b.shape and torch.isfinite(a).all(), name
        # relative to the gradient's own largest magnitude.  At T = 1 the context hardly depends on q and k (only through the
        # 1e-6 of the denominator): dq and dk are 1e-5 of the O(|g|) terms that cancel in them, in autograd as much as here, so
        # there the scale is that of the terms, max |g|
        scale = max(b.abs().max().item(), g.abs().max().item() if T == 1 and name in ("dq", "dk") else 0.0)
        assert (a - b).abs().max() <= 1e-12 * scale, (name, (a - b).abs().max().item(), scale)
    assert (got[3][T:] == 0).all() and (want[3][T:] == 0).all()


def test_default_chunk_of_performer_py_gives_nan_gradients_where_the_last_chunk_is_padded():
    """Why every comparison here calls `causal_linear_attention` with chunk=T: the note of DESIGN 8, pinned."""
    q, k, v, pos, W, g = make_inputs(1, 1, 130, 64, 17, seed=3)
    fa = FastAttention(dim_heads=64, nb_features=17, causal=True, generalized_attention=True)
    fa.projection_matrix = W
    k, v = k.requires_grad_(True), v.requires_grad_(True)
    out = causal_linear_attention(fa.feature_map(q), fa.feature_map(k), v)
    assert torch.isfinite(out).all()
    dk, dv = torch.autograd.grad(out, [k, v], grad_outputs=g[..., :64])
    assert torch.isnan(dk).any() and torch.isnan(dv).any()


def test_the_two_faults_of_the_witnesses_move_the_gradients():
    q, k, v, pos, W, g = make_inputs(1, 2, 130, 64, 33, seed=5, qk_scale=0.05)
    good = PerformerReference(64).backward(q, k, v, pos, W, g)
    for bad in (PerformerReference(64, drop_carry_at=2), PerformerReference(64, leak_padded_features=True)):
        got = bad.backward(q, k, v, pos, W, g)
        assert max(((a - b).abs().max() / b.abs().max()).item() for a, b in zip(got, good)) > 1e-4
