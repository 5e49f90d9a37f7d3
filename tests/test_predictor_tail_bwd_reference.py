"""The mathematics of the predictor tail's backward, on the CPU in fp64.

`TailReference` evaluates the closed form csrc/sea_tail_bwd.hip computes -- the tap matrix M of the padded nearest upsample and the
area resize, the LayerNorm and softmax gradients per row, the three products, dW as a sum of per-block parts in block order -- and
is held here to fp64 autograd through the framework's own chain: `F.interpolate(nearest)` -> `conv2d(pad (0,1))` ->
`interpolate(area)` -> `layer_norm` -> `softmax`.  The GPU tests (test_gpu_predictor_tail_bwd.py) take the reference, the
yardstick, the inputs and the bar from this file."""
import functools

import pytest
import torch
import torch.nn.functional as F

F64 = torch.float64
UP = 4


def block_rows(rows):
    """rows of one workgroup of csrc/sea_tail_bwd.hip: the shapes alone decide it"""
    return min(32, max(8, (rows + 1023) // 1024))


class TailReference:
    """fp64.  Three deliberate faults, for the witnesses: `drop_xhat_term` leaves mean_j(gamma ds (.) xh) out of da;
    `border_to_pixel0` gives the two border taps to pixel 0 instead of the bias slot; `drop_block` = index of a block of rows whose
    part of dW is left out of the sum."""

    def __init__(self, drop_xhat_term=False, border_to_pixel0=False, drop_block=None):
        self.drop_term, self.border0, self.drop_block = drop_xhat_term, border_to_pixel0, drop_block

    def taps(self, W4, T_m):
        """M (T_m, W4 + 1): output pixel j averages the padded pixels [xs, xe); padded pixel x is the border (column W4: the bias
        alone) for x = 0 and x = Wp - 1, source pixel (x - 1) // up otherwise"""
        Wp = UP * W4 + 2
        M = torch.zeros((T_m, W4 + 1), dtype=F64)
        for j in range(T_m):
            xs, xe = (j * Wp) // T_m, -((-(j + 1) * Wp) // T_m)
            for x in range(xs, xe):
                border = x == 0 or x == Wp - 1
                col = (0 if self.border0 else W4) if border else (x - 1) // UP
                M[j, col] += 1.0 / (xe - xs)
        return M

    def _forward(self, y, W, b, gamma, beta, eps):
        y, W, b, gamma, beta = (t.to(F64) for t in (y, W, b, gamma, beta))
        N, C, T, W4 = y.shape
        M = self.taps(W4, gamma.shape[0])
        z = torch.einsum('hc,nctw->nhtw', W, y) + b.view(1, -1, 1, 1)
        zb = torch.cat([z, b.view(1, -1, 1, 1).expand(N, -1, T, 1)], -1)
        a = zb @ M.t()
        mu = a.mean(-1, keepdim=True)
        rstd = 1.0 / torch.sqrt(((a - mu) ** 2).mean(-1, keepdim=True) + eps)
        xh = (a - mu) * rstd
        s = gamma * xh + beta
        return y, W, gamma, M, rstd, xh, s, torch.softmax(s, -1)

    def forward(self, y, W, b, gamma, beta, eps=1e-5):
        """(probs, scores), (N,H,T,T_m)"""
        *_rest, s, p = self._forward(y, W, b, gamma, beta, eps)
        return p, s

    def backward(self, y, W, b, gamma, beta, eps, g_s, g_p):
        """(dy, dW, db, dgamma, dbeta); either of g_s, g_p may be None"""
        y, W, gamma, M, rstd, xh, s, p = self._forward(y, W, b, gamma, beta, eps)
        N, C, T, W4 = y.shape
        H = W.shape[0]
        ds = torch.zeros_like(s)
        if g_s is not None:
            ds = ds + g_s.to(F64)
        if g_p is not None:
            g_p = g_p.to(F64)
            ds = ds + p * (g_p - (g_p * p).sum(-1, keepdim=True))
        dgamma, dbeta = (ds * xh).sum((0, 1, 2)), ds.sum((0, 1, 2))
        tt = gamma * ds
        da = tt - tt.mean(-1, keepdim=True)
        if not self.drop_term:
            da = da - xh * (tt * xh).mean(-1, keepdim=True)
        da = rstd * da
        dzb = da @ M
        dz = dzb[..., :W4]
        dy = torch.einsum('hc,nhtw->nctw', W, dz)
        # dW: one part per block of consecutive (n, t) rows, added in block order
        dz_r = dz.permute(0, 2, 1, 3).reshape(N * T, H, W4)
        y_r = y.permute(0, 2, 1, 3).reshape(N * T, C, W4)
        rb = block_rows(N * T)
        dW = torch.zeros((H, C), dtype=F64)
        for bi, r0 in enumerate(range(0, N * T, rb)):
            if bi != self.drop_block:
                dW = dW + torch.einsum('rhw,rcw->hc', dz_r[r0:r0 + rb], y_r[r0:r0 + rb])
        db = dz.sum((0, 2, 3)) + dzb[..., W4].sum((0, 2))
        return dy, dW, db, dgamma, dbeta


def tail_chain(y, W, b, gamma, beta, eps, T_m):
    """the module chain of modules.py in the dtype of its arguments: (probs, scores)"""
    x = F.interpolate(y, scale_factor=(1, UP), mode='nearest')
    x = F.conv2d(x, W[:, :, None, None], b, 1, (0, 1), 1)
    x = F.interpolate(x, (x.shape[-2], T_m), mode='area')
    s = F.layer_norm(x, (T_m,), gamma, beta, eps)
    return torch.softmax(s, -1), s


def tail_torch(y, W, b, gamma, beta, eps, g_s, g_p, dtype):
    """`tail_chain` under autograd in `dtype` (fp64: the truth of this file; fp32: the GPU tests' yardstick).
    Returns (dy, dW, db, dgamma, dbeta)."""
    y, W, b, gamma, beta = (t.detach().to(dtype).requires_grad_(True) for t in (y, W, b, gamma, beta))
    p, s = tail_chain(y, W, b, gamma, beta, eps, gamma.shape[0])
    outs, gs = [], []
    if g_s is not None:
        outs.append(s); gs.append(g_s.to(dtype))
    if g_p is not None:
        outs.append(p); gs.append(g_p.to(dtype))
    return torch.autograd.grad(outs, [y, W, b, gamma, beta], grad_outputs=gs)


def make_inputs(N, H, T, T_m, seed, dtype=F64):
    """y = relu(randn) (N, 2H, T, T_m / 4), W, b, gamma, beta, g_s, g_p as `dtype` values (rounded there, so that every path
    starts from the same numbers)"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=gen, dtype=F64)
    C = 2 * H
    y = torch.relu(r(N, C, T, T_m // UP))
    W, b = r(H, C) * C ** -0.5, r(H)
    gamma, beta = 1.0 + 0.25 * r(T_m), 0.25 * r(T_m)
    g_s, g_p = r(N, H, T, T_m), r(N, H, T, T_m)
    return tuple(t.to(dtype) for t in (y, W, b, gamma, beta, g_s, g_p))


def bar_of(yard, ref):
    """4 x the yardstick's largest error, at least 2^-22 of the reference's largest magnitude (DESIGN 5.7's rule)."""
    return max(4 * (yard.to(F64) - ref).abs().max().item(), 2.0 ** -22 * ref.abs().max().item())


EPS = 1e-5
NAMES = ("dy", "dW", "db", "dgamma", "dbeta")
SHAPES = [(1, 12, 5, 64), (2, 4, 7, 96), (1, 5, 3, 128), (1, 3, 2, 256), (2, 2, 3, 32)]


@functools.lru_cache(maxsize=None)
def _inputs(idx):
    return make_inputs(*SHAPES[idx], seed=100 + idx)


@pytest.mark.parametrize("which", ("g_s", "g_p", "both"))
@pytest.mark.parametrize("idx", range(len(SHAPES)), ids=["N%d-H%d-T%d-TM%d" % s for s in SHAPES])
def test_closed_form_against_fp64_autograd(idx, which):
    y, W, b, gamma, beta, g_s, g_p = _inputs(idx)
    g_s, g_p = (g_s if which != "g_p" else None), (g_p if which != "g_s" else None)
    p_want, s_want = tail_chain(y, W, b, gamma, beta, EPS, gamma.shape[0])
    p_got, s_got = TailReference().forward(y, W, b, gamma, beta, EPS)
    assert (s_got - s_want).abs().max() <= 1e-12 * s_want.abs().max() and (p_got - p_want).abs().max() <= 1e-12 * p_want.abs().max()
    got = TailReference().backward(y, W, b, gamma, beta, EPS, g_s, g_p)
    want = tail_torch(y, W, b, gamma, beta, EPS, g_s, g_p, F64)
    for name, a, w in zip(NAMES, got, want):
        assert a.shape == w.shape and torch.isfinite(a).all(), name
        if name == "db":                                   # identically zero: both sides are rounding noise of the terms of dW
            lim = 1e-12 * want[1].abs().max().item()
            assert a.abs().max().item() <= lim and w.abs().max().item() <= lim, (a.abs().max().item(), w.abs().max().item(), lim)
        else:
            assert (a - w).abs().max() <= 1e-12 * w.abs().max(), (name, (a - w).abs().max().item(), w.abs().max().item())


def test_tap_matrix_rows_sum_to_one_and_fit_the_kernels_gather_window():
    """Every output pixel's taps weigh 1 in all; and the output pixels that touch source pixel w lie in the eight slots from
    jlo(w) = max(0, (4 w + 1) T_m // Wp - 1), the window csrc/sea_tail_bwd.hip gathers dz over."""
    for T_m in range(32, 257, 32):
        W4 = T_m // UP
        M = TailReference().taps(W4, T_m)
        assert (M.sum(1) - 1).abs().max() < 1e-15
        for w in range(W4):
            js = M[:, w].nonzero().flatten().tolist()
            jlo = max(0, (4 * w + 1) * T_m // (4 * W4 + 2) - 1)
            assert js and jlo <= js[0] and js[-1] < jlo + 8, (T_m, w, js, jlo)


# ---- witnesses: each fault is far outside the bar the kernel is held to, on the fp32 case ----------------------------------------
WITNESS_SHAPE = (1, 40, 9, 128)                            # fp32; 9 rows: two blocks of rows, the second one row long


@functools.lru_cache(maxsize=None)
def _witness_case():
    inp = make_inputs(*WITNESS_SHAPE, seed=7, dtype=torch.float32)
    ref = TailReference().backward(*inp[:5], EPS, *inp[5:])
    yard = tail_torch(*inp[:5], EPS, *inp[5:], torch.float32)
    bars = [bar_of(yd, r) for yd, r in zip(yard, ref)]
    return inp, ref, bars


@pytest.mark.parametrize("fault", ("xhat-term", "border-to-pixel-0", "dropped-block"))
def test_witnesses_exceed_a_hundred_bars(fault):
    inp, ref, bars = _witness_case()
    assert block_rows(WITNESS_SHAPE[0] * WITNESS_SHAPE[2]) == 8
    bad = {"xhat-term": TailReference(drop_xhat_term=True), "border-to-pixel-0": TailReference(border_to_pixel0=True),
           "dropped-block": TailReference(drop_block=1)}[fault]
    got = bad.backward(*inp[:5], EPS, *inp[5:])
    ratios = {n: (g - r).abs().max().item() / bar for n, g, r, bar in zip(NAMES, got, ref, bars) if n != "db"}
    print(f"[tail-bwd] witness {fault}: err / bar " + " ".join(f"{n} {v:.1f}" for n, v in ratios.items()))
    assert max(ratios.values()) > 100, ratios
