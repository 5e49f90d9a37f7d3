"""-m gpu: the fp32 forms of the estimator kernels held to a float64 evaluation of the same operation on the same inputs,
at production sizes -- the predictor convolution's fp32 form (`causal_conv_c8f_kernel`) at OPT-1.3B x 8 and the fp32-MFMA
Performer (`performer_kernel`) at T = 4096 ... 32768, with the plan's segment count and with one segment.  Until now these
were pinned only to other forms of this build or checked against fp64 at T <= 1024.  (The 16-bit forms -- convolution, 1x1
epilogue, tail and MLP -- are held to fp64 the same way in `test_gpu_estimator_reference_16bit.py`.)

Every bar is elementwise and follows from where the kernel rounds, not from observed errors: a value the kernel forms in
fp32 (the fp32 MFMA is a k-ordered fma chain, one rounding per product) is within n * 2^-24 * sum|terms| of the exact sum,
n = the additions on the longest chain; the output is then rounded once more (`fp32_bar`: 1/2 ulp).  The Performer's
bar grows with T through its running state's accumulation chain (`performer_bar_err`).  These worst-case bars see
structural faults (the witnesses below), not a loss of a few bits in the products.

Each case has a sensitivity witness: the change one plausible fault makes in the reference (a missing 8-channel block of
one conv tap, one 64-row Performer chunk dropped from the prefix sums) must exceed the bar 10x somewhere in the case.

Observed max |out - ref| / bar on MI355X: conv fp32 0.009; Performer fp32 0.002 .. 0.024 (the largest at T = 32768).  The bars
are worst-case bounds, so ratios far below 1 are expected.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                  # unit roundoff of fp32


@pytest.fixture(scope="module")
def ops():
    from sea_attention_amd.perlin_attention import ops
    return ops


def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ulp32(x: torch.Tensor) -> torch.Tensor:
    """Spacing of the fp32 grid at the fp64 values |x| (subnormal spacing below the normal range)."""
    _, e = torch.frexp(x.abs())
    return torch.where(x != 0, torch.ldexp(torch.ones_like(x), (e - 1).clamp(min=-126) - 23), torch.full_like(x, 2.0 ** -149))


def fp32_check(out, ref, err, what):
    """out: the kernel's fp32 values; ref: fp64 value of the operation on the same inputs; err: fp64 bound on |the
    kernel's value before its final rounding - ref|.  Asserts |out - ref| <= err + 1/2 ulp(|ref| + err) everywhere and
    returns that bar (for the witness)."""
    bar = err + ulp32(ref.abs() + err) / 2
    d = (out.double() - ref).abs()
    ratio = (d / bar).max().item()
    print(f"[est-ref] {what}: max|err|/bar = {ratio:.3f}")
    assert torch.isfinite(out).all(), what
    assert ratio <= 1.0, (what, ratio, d.flatten()[(d / bar).argmax()].item())
    return bar


def witness(delta, bar, what):
    """The change one plausible fault makes in the reference must exceed the bar 10x somewhere in the case."""
    w = (delta.abs() / bar).max().item()
    print(f"[est-ref] {what}: witness {w:.1f} x bar")
    assert w >= 10.0, (what, "a fault of this size would pass", w)


# ---- 1. the predictor convolution ---------------------------------------------------------------------------------------
def c8_logical(y):
    """(N, T, C/8, W, 8) -> (N, T, C, W) view."""
    N, T, C8, W, _ = y.shape
    return y.permute(0, 1, 2, 4, 3).reshape(N, T, C8 * 8, W)


def conv_patches(xl, n_idx, t_idx, ks, dil, pad_w):
    """fp64 im2col of the causal conv for output rows (n_idx, t_idx): (R, W, ks*ks*Cin), k order (tap row, tap col, channel)."""
    R = n_idx.numel()
    N, T, Cin, W = xl.shape
    taps = []
    for i in range(ks):
        tt = t_idx - (ks - 1 - i) * dil                                  # CausalConv2d: top padding of (ks - 1) dil rows
        rows = xl[n_idx, tt.clamp(min=0)].double() * (tt >= 0).double().view(-1, 1, 1)
        rows = F.pad(rows, (pad_w, pad_w))
        for j in range(ks):
            taps.append(rows[:, :, j * dil:j * dil + W])
    return torch.stack(taps, 1).permute(0, 3, 1, 2).reshape(R, W, ks * ks * Cin)


def conv_f32_rows(ks, dil, N, T, per_cu):
    """Rows where the fp32 form goes wrong: the first 2 dil + 2 rows and the last 3 rows of (up to 8) sequences (causal
    padding, sequence ends), the two rows on either side of EVERY workgroup boundary of the launch, and random rows.  The
    boundaries are launch_conv_f32's (sea_conv.hip): grid = min(ceil(nwork / CONVF_WAVES), CUs x per_cu) persistent
    workgroups, workgroup b takes the contiguous work items [b per, (b + 1) per), per = ceil(nwork / grid); with W <= 64
    one work item is one row."""
    g = torch.Generator().manual_seed(N * 7919 + T)
    rows = set()
    for n in list(range(min(N, 4))) + list(range(max(4, N - 4), N)):
        for t in list(range(min(T, (ks - 1) * dil + 2))) + list(range(max(0, T - 3), T)):
            rows.add(n * T + t)
    tot = N * T
    grid = min((tot + 3) // 4, cus() * per_cu)
    per = (tot + grid - 1) // grid
    for b in range(per, tot, per):
        rows.update(range(b - 2, min(tot, b + 2)))
    rows.update(torch.randint(0, tot, (512,), generator=g).tolist())
    flat = torch.tensor(sorted(rows), dtype=torch.long)
    return flat // T, flat % T


def check_conv_f32(ops, x, wt, b, ks, dil, pad_w, relu, per_cu, what):
    """`causal_conv_c8` on fp32 C8 input x against the fp64 convolution at the sampled rows.  Bar: the fp32 MFMA's fma chain
    over ks*ks*Cin products plus the bias, n = ks^2 Cin + 1 roundings of at most 2^-24 of the partial sum (<= sum|terms|)."""
    N, T, C8, W, _ = x.shape
    Cin, Cout = C8 * 8, wt.shape[0]
    y = ops.causal_conv_c8(x, wt, b, ks, dil, pad_w, relu=relu)
    n_idx, t_idx = conv_f32_rows(ks, dil, N, T, per_cu)
    n_idx, t_idx = n_idx.to(DEV), t_idx.to(DEV)
    xl = c8_logical(x)
    wm = wt[:, :, :ks, :ks].double().permute(0, 2, 3, 1).reshape(Cout, ks * ks * Cin)
    bb = b.double()
    yl = c8_logical(y)[n_idx, t_idx].permute(0, 2, 1)                   # (R, W, Cout)
    refs, errs, deltas = [], [], []
    cols = torch.arange(ks * ks * Cin, device=DEV).view(ks, ks, Cin)[ks - 1, 0, 8:16].reshape(-1)   # one 8-channel block of one tap
    for s in range(0, n_idx.numel(), 256):
        P = conv_patches(xl, n_idx[s:s + 256], t_idx[s:s + 256], ks, dil, pad_w)
        acc = P @ wm.t() + bb
        terms = P.abs() @ wm.abs().t() + bb.abs()
        ref = torch.relu(acc) if relu else acc
        refs.append(ref)
        errs.append((ks * ks * Cin + 1) * U * terms)
        dropped = acc - P[..., cols] @ wm[:, cols].t()                  # fault: that block's products never added
        deltas.append((torch.relu(dropped) if relu else dropped) - ref)
    bar = fp32_check(yl, torch.cat(refs), torch.cat(errs), what)
    witness(torch.cat(deltas), bar, what)


@pytest.mark.parametrize("relu", [True, False])
def test_conv_fp32_form(ops, relu):
    """fp32 data at OPT-1.3B x 8 size (8 x 4096 rows, 64 -> 64 channels, W = 64, dil 2) takes `causal_conv_c8f_kernel`
    (sea_causal_conv_c8 -> conv_f32 -> launch_conv_f32<3>): conv_c8_f32_supported holds (the 148 KB fp32 weight image fits
    the 160 KB LDS), and an image over 80 KB gives per_cu = 1 -- one persistent workgroup per CU, whose CONVF_WAVES waves
    step through its contiguous run of rows."""
    assert ops.conv_c8_f32_supported(64, 64, 3)
    g = torch.Generator(device=DEV).manual_seed(77)
    x = torch.randn((8, 4096, 8, 64, 8), generator=g, device=DEV)
    wt = torch.randn((64, 64, 5, 3), generator=g, device=DEV) * (64 * 9) ** -0.5
    b = torch.randn(64, generator=g, device=DEV) * 0.1
    check_conv_f32(ops, x, wt, b, 3, 2, 2, relu, 1, f"conv fp32 relu={relu}")


# ---- 2. the Performer --------------------------------------------------------------------------------------------------
def performer_reference(q, k, v, pos, Wp, D, seg_len, C=64):
    """Chunked fp64 prefix sums of phi(k) (x) v_aug and phi(k) (chunks of C = 64 rows), with the magnitudes the bar needs.
    q, k, v (N, H, T, D) fp32 device tensors; Wp (nb, D) = the projection as the kernel holds it.  Returns a dict of (N, H, T, .) fp64 tensors at every row."""
    N, H, T, _ = q.shape
    nb = Wp.shape[0]
    s = D ** -0.25
    W = Wp.double()
    vaug = torch.cat([pos[:T].double().expand(N, H, T, D), v.double()], -1)              # (N, H, T, 2D)

    def phi(x):
        x = x.double()
        pre = s * (x @ W.t())
        # fp32: D exact products summed (D additions), the scale, the relu and the + 1e-3: (D + 3) u of the magnitudes
        e = (D + 3) * U * (s * (x.abs() @ W.abs().t()) + 1e-3)
        return torch.relu(pre) + 1e-3, e

    pq, eq = phi(q)
    pk, ek = phi(k)
    nc = (T + C - 1) // C
    pad = nc * C - T
    P = lambda t: F.pad(t, (0, 0, 0, pad)).view(N, H, nc, C, t.shape[-1])
    pkc, ekc, vc, vac = P(pk), P(ek), P(vaug), P(vaug.abs())
    # states BEFORE each chunk (exclusive prefix over chunks): S = sum phi(k) v^T, A = sum phi(k) |v|^T, E = sum e_k |v|^T
    inc = torch.einsum("nhcsf,nhcse->nhcfe", pkc, vc)
    inca = torch.einsum("nhcsf,nhcse->nhcfe", pkc, vac)
    ince = torch.einsum("nhcsf,nhcse->nhcfe", ekc, vac)
    excl = lambda t: torch.cumsum(t, 2) - t
    S, Sa, Se = excl(inc), excl(inca), excl(ince)
    ks, kse = excl(pkc.sum(3)), excl(ekc.sum(3))                                         # (N, H, nc, nb)
    # the kernel's running state is rounded at every product it takes in (fp32 accumulators): u * sum over the chain of the
    # partial sums' magnitudes <= u * C * sum over earlier chunks of (|S_c| + the chunk's |increment|), counted twice
    # (cut into segments: a segment's own pass starts from zero, the output pass from the carried total S_start)
    cstart = (torch.arange(nc, device=q.device) * C // seg_len) * (seg_len // C)
    Q = excl(2 * C * (S.abs() + S[:, :, cstart].abs() + inca))
    pqc, eqc = P(pq), P(eq)
    A = torch.einsum("nhcif,nhcjf->nhcij", pqc, pkc).tril()
    Ae = (torch.einsum("nhcif,nhcjf->nhcij", eqc, pkc) + torch.einsum("nhcif,nhcjf->nhcij", pqc, ekc)).tril()
    num = A @ vc + torch.einsum("nhcif,nhcfe->nhcie", pqc, S)
    mag = A @ vac + torch.einsum("nhcif,nhcfe->nhcie", pqc, Sa)                          # sum_s a_ts |v_s|
    num_e = Ae @ vac + torch.einsum("nhcif,nhcfe->nhcie", eqc, Sa) + torch.einsum("nhcif,nhcfe->nhcie", pqc, Se)
    qfe = torch.einsum("nhcif,nhcfe->nhcie", pqc, Q)
    den = A.sum(-1) + torch.einsum("nhcif,nhcf->nhci", pqc, ks + 1e-6)
    den_e = Ae.sum(-1) + torch.einsum("nhcif,nhcf->nhci", eqc, ks) + torch.einsum("nhcif,nhcf->nhci", pqc, kse)
    un = lambda t: t.reshape(N, H, nc * C, *t.shape[4:])[:, :, :T]
    out = {"num": un(num), "mag": un(mag), "num_e": un(num_e), "qfe": un(qfe), "den": un(den), "den_e": un(den_e)}
    out["ctx"] = out["num"] / out["den"].unsqueeze(-1)
    out["drop"] = (pkc, vc, pqc)
    return out


def performer_bar_err(R, nb, T, nseg, C):
    """Bound on |the fp32 kernel's ctx - ctx| before the output rounding, from where `performer_kernel` rounds:
      phi: fp32 dot products (R's num_e / den_e carry those errors through the sums);
      every product on the fp32 MFMA (an fma chain: one rounding per product): nb products per A / carry element, C rows
        per chunk, nseg carried totals, a few for the epilogue; the running state's chain (R's qfe); the k-sum, at most 8
        partial sums folded per chunk of C rows, 8 T / C additions;
    then the division: |d(n/d)| <= (dn + |ctx| dd) / d, and two roundings."""
    nbp = (nb + 15) // 16 * 16
    kn = (3 * nbp + 2 * C + nseg + 8) * U
    kd = (3 * nbp + 2 * C + 8 * ((T + C - 1) // C) + 16 + nseg + 8) * U
    den = R["den"].unsqueeze(-1)
    dn = kn * R["mag"] + R["num_e"] + U * R["qfe"]
    dd = (kd * R["den"] + R["den_e"]).unsqueeze(-1)
    ctx = R["ctx"]
    return (dn + ctx.abs() * dd) / den * (1 + 1e-3) + 2 * U * ctx.abs()


@pytest.mark.parametrize("N,H,T,D,nbf", [
    (1, 2, 4096, 64, 8),      # nb 33: perf_form row D = 64, nbt <= 3 (64-row chunks); the plan cuts (2 pairs)
    (1, 2, 8192, 64, 4),      # nb 66: row D = 64, nbt <= 5
    (1, 1, 8192, 128, 8),     # nb 77: row D = 128 (32-row chunks)
    (1, 1, 32768, 80, 8),     # nb 43: row D = 80, nbt <= 3
])
def test_performer_fp32_long_sequences(ops, N, H, T, D, nbf):
    """`performer_value` on fp32 data at long sequences, with the plan's segment count and with n_segments = 1, against
    chunked fp64 prefix sums; the bar grows with T through the state's accumulation chain (`performer_bar_err`)."""
    from sea_attention_amd.perlin_attention.performer import FastAttention
    from sea_attention_amd.perlin_attention.ops import predictor as PR
    dtype = torch.float32
    torch.manual_seed(5)
    nb = int(D * math.log(D) / nbf)
    fa = FastAttention(D, nb_features=nb, causal=True, generalized_attention=True).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(T + D)
    q = (torch.randn(N, H, T, D, generator=g, device=DEV) * D ** -0.5).to(dtype)
    k = torch.randn(N, H, T, D, generator=g, device=DEV).to(dtype)
    v = torch.randn(N, H, T, D, generator=g, device=DEV).to(dtype)
    pos = torch.randn(T, D, generator=g, device=DEV).to(dtype)
    Wp = fa.projection_matrix.to(dtype).float()                         # the reference casts the projection to the data dtype
    plan = PR.performer_plan(N, H, T, D, nb, dtype)[0]
    assert plan > 1                                                     # few pairs: the plan cuts the rows into segments
    Cf = 64 if D == 64 or (D == 80 and nb <= 48) else 32               # perf_form: the fp32 kernel's chunk rows
    for nseg in sorted({plan, 1}):
        chunks = (T + 63) // 64
        R = performer_reference(q, k, v, pos, Wp, D, (chunks + nseg - 1) // nseg * 64)      # perf_seg_len
        out = ops.performer_value(q, k, v, pos, fa.projection_matrix, n_segments=nseg)
        what = f"performer {dtype} T{T} D{D} nb{nb} nseg{nseg}"
        err = performer_bar_err(R, nb, T, nseg, Cf)
        # witness: one 64-row chunk in the middle dropped from the prefix sums, seen at the rows after it
        pkc, vc, pqc = R["drop"]
        c0 = (T // 2) // 64 - 1
        dnum = torch.einsum("nhcf,nhfe->nhce", pqc[:, :, c0 + 1:].flatten(2, 3)[..., :T - 64 * (c0 + 1), :],
                            torch.einsum("nhsf,nhse->nhfe", pkc[:, :, c0], vc[:, :, c0]))
        dden = torch.einsum("nhcf,nhf->nhc", pqc[:, :, c0 + 1:].flatten(2, 3)[..., :T - 64 * (c0 + 1), :], pkc[:, :, c0].sum(2))
        tail = slice(64 * (c0 + 1), T)
        ctx_f = (R["num"][:, :, tail] - dnum) / (R["den"][:, :, tail] - dden).unsqueeze(-1)
        bar = fp32_check(out[..., :2 * D], R["ctx"], err, what)
        witness(ctx_f - R["ctx"][:, :, tail], bar[:, :, tail], what)
        assert torch.equal(out[..., 2 * D:], v)
