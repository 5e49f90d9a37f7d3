"""-m gpu: the 16-bit (bf16 = production, f16) forms of the estimator kernels held to a float64 evaluation of the same
operation on the same inputs -- the predictor convolution in every launch form, its 1x1 epilogue, the predictor tail from
`z` and from `y`, and the fused MLP stage by stage.  `test_gpu_estimator_reference.py` does the same for the fp32 forms;
helpers are shared by import.

Every bar is elementwise and follows from where the kernel rounds, never from observed errors:

  U16 = 2^-23 per term of anything accumulated on a 16-bit MFMA.  Products of two bf16 / two f16 values are exact in fp32;
      the instruction's internal summation order and rounding mode are not documented, and n * 2^-23 * sum|terms| (n = the
      number of terms, C operand and bias included) bounds ANY order under round-to-nearest or truncation.
  U   = 2^-24 per plain fp32 VALU operation.
  an explicit allowance per approximate intrinsic (R_RSQRT, r_exp, R_RCP, G_ERF below: from the published ISA
      accuracy of v_rsq_f32 / v_exp_f32 / v_rcp_f32, 1 ulp each, plus the roundings of the argument scaling; no ulp table of
      the HIP math functions ships with the toolkit, so `test_intrinsic_probes` measures the torch-visible equivalents
      against fp64 and asserts they sit inside the same allowances),
  then the final store: + 1/2 ulp16(|ref| + err)  (`ulp16`: the spacing of the bf16 / f16 grid, correct at binade edges
      and in the subnormal range; fp32 outputs: `ulp32`).

Each case carries sensitivity witnesses: the change one plausible fault makes in the REFERENCE must exceed the bar 10x
somewhere in the case -- i.e. applying that fault to the reference instead of the kernel turns the corresponding *_check
red.  (The truncation witness is a fraction of elements instead: one ulp against half of one cannot reach 10x.)

1. `causal_conv_c8` (sea_conv.hip).  Rounding points: the MFMA chain over ks^2 Cin products (k order (tap row, 32-channel
   chunk, tap column), sea_conv.hip:51), `acc + bias` in fp32 and ReLU (sea_conv.hip:243-244 and :519-520 for the ring form),
   `pack2` = one round-to-nearest to the data type (sea_common.hpp:147).  Reference: fp64 implicit GEMM (`conv_patches`) +
   the bias as the op passes it (bias.to(dtype).float()); err = (ks^2 Cin + 1) U16 (|P| @ |W|^T + |b|); ReLU is 1-Lipschitz.
   EVERY row of every launch is checked (the fp64 reference of the largest launch, 9 x 3701 rows, is 0.3 TFLOP).
   Launch geometry: `conv16_launch` restates ring_takes (sea_conv.hip:752-755), launch_conv_ring (:761-762) and launch_conv
   (:784-788); every case asserts the form it is meant to reach, from `cus()`.
   Witnesses: (a) one 8-channel block of one tap never added; (b) a column tap that leaves the row reads the neighbouring
   pixel instead of zero (the ring's LDS zero pads, sea_conv.hip:441-445; the register form's range check, :184 / :208);
   (c) a row t < 2 dil takes the tap row in the causal padding from the rows before it (the previous sequence) instead of
   skipping it (sea_conv.hip:160 / :484); (d) bf16, no ReLU: the final pack truncates toward zero -- the truncated reference
   must lie outside the bar at >= 10 % of the elements (f16 exempt: there the accumulation term dominates the half ulp).
2. The 1x1 epilogue (`causal_conv_c8_z`, want_y=True; sea_conv.hip:266-295).  y as in 1.  z against fp64 FROM THE y THE SAME
   LAUNCH WROTE (the packed registers `pk` are both the y store and the A operand, :271): z_ref = W1_16 . y + b1,
   err = (Cout + 1) U16 (|W1| |y| + |b1|), fp32 output: + 1/2 ulp32.  Witnesses: one 8-channel k-block of the 1x1 dropped;
   Cout = 80: channels 64-71 swapped with 72-79 (the odd tile's `__shfl` gather, :275-278).
3. The tail (sea_tail.hpp:275-351, `heads_impl`): after z everything is fp32 up to ONE rounding each of scores and probs
   (`store_run`, :28).  Reference in fp64: area resize (padding = the bias, 1/cnt taps of adaptive_avg_pool, `area_taps`) ->
   LayerNorm -> softmax.  Error model (`tail_reference`): resize 3 adds, the 1/cnt constant and a multiply (5 U sum|taps| /
   cnt); mean and variance over T_M terms; rsqrtf; the affine (3 roundings); probs: |dp / p| <= 2 max|d score| + the
   exp-argument subtraction and `__expf` for numerator and denominator + (T_M + 2) U; then 1/2 ulp16.  From `y` (the MFMA
   variant, `tail_z_tile`, sea_tail.hpp:59) z itself carries (C + 1) U16 (|W1| |y| + |b1|).
   Witnesses: the window's last tap dropped from the resize (the issue asked for "the third tap where cnt == 3": with
   T_M = up * W4 even and two padding pixels no window has three taps, so the last tap of the two stands in); gamma / beta
   shifted by one lane slot (E = ceil(T_M / 64) elements); biased against unbiased variance is REPORTED only: at
   LayerNorm length T_M its relative size 1 / (2 T_M) is of the order of half a 16-bit ulp, far under 10x.
4. `predictor_mlp` (sea_mlp.hip:196-290), stage by stage -- see `mlp_*` below.  Stage 1 (tpred) against fp64 from x with a
   flip-aware bound for the Linear's unexposed 16-bit rounding; stage 2 and the gates against fp64 from the kernel's own
   tpred (bit for bit the B operand `tb[]` of the second product, sea_mlp.hip:223-243).

Observed max |out - ref| / bar on MI355X (256 CUs), bf16 / f16 (the half ulp of the final store is most of every 16-bit
bar, so ratios close to 1 are expected: some element always sits next to a rounding midpoint):
  conv, ring form            0.938 .. 0.943 / 0.695        conv, register forms   0.922 .. 0.980 / 0.600 .. 0.870
  conv + z: y                0.923 .. 0.980 / 0.567 .. 0.882      z (fp32)        0.013 .. 0.033 / 0.019 .. 0.047
  tail from z: scores        0.988 .. 0.997 / 0.918 .. 0.982      probs           0.923 .. 0.985 / 0.921 .. 0.961
  tail from y: scores        0.970 .. 0.989 / 0.803 .. 0.922      probs           0.838 .. 0.933 / 0.696 .. 0.940
  tail + selection (bf16)    scores 0.976, probs 0.868
  mlp: tpred                 0.827 .. 0.973 / 0.472 .. 0.673      decoder         0.989 .. 0.999 / 0.673 .. 0.946
       gates (fp32)          0.207 .. 0.996 / 0.176 .. 0.989  (a gate whose Linear output flipped moves by delta / 4)
Witnesses: the smallest of the 296 is 328 x bar (most are thousands); the truncating pack lies outside the bar at 14.1 %
(80 channels) .. 37.6 % (24 channels) of the elements, 19 % at 64; unbiased variance (reported) 6 .. 260 x bar.  No unit was
raised.  Probes: torch's rsqrt 0.50 ulp, reciprocal 0.50 ulp, exp 0.37 of r_exp; the erf formula of gelu_erf in torch fp32
5e-7 (G_ERF = 1.9e-6).
"""
import math

import pytest
import torch
import torch.nn.functional as F

from test_gpu_estimator_reference import c8_logical, conv_patches, cus, fp32_check, ulp32, witness

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24                  # unit roundoff of fp32: one VALU operation
U16 = 2.0 ** -23                # per term of a sum formed inside a 16-bit MFMA (any order, either rounding mode)
# v_rsq_f32 / v_rcp_f32 / v_exp_f32: 1 ulp (the published CDNA ISA guides); 2 ulp allowed for the library wrappers' scaling
R_RSQRT = 2 * 2.0 ** -23        # rsqrtf, relative
R_RCP = 2 * 2.0 ** -23          # __builtin_amdgcn_rcpf and the fp32 division 1.0f / x, relative
DTYPES = [torch.bfloat16, torch.float16]


def r_exp(x):
    """Relative allowance of `__expf(x)` = v_exp_f32(x * log2 e): the instruction's 1 ulp (2^-23), and the product's rounding
    and the constant's representation, each |x log2 e| U in the exponent of 2, i.e. |x| U ln 2 log2 e = |x| U relative."""
    return 2.0 ** -23 + 2 * U * x.abs()


@pytest.fixture(scope="module")
def ops():
    from sea_attention_amd.perlin_attention import ops
    return ops


def ulp16(x: torch.Tensor, dtype) -> torch.Tensor:
    """Spacing of the bf16 / f16 grid at the fp64 values |x|: 2^(e - p + 1) in the binade [2^e, 2^(e+1)) (a power of two
    itself belongs to the binade ABOVE it, the wider spacing: what a bar needs), the subnormal spacing below the normal
    range and at 0.  bf16: p = 8, e_min = -126; f16: p = 11, e_min = -14."""
    p, emin = (8, -126) if dtype == torch.bfloat16 else (11, -14)
    _, e = torch.frexp(x.abs())
    sp = torch.ldexp(torch.ones_like(x), (e - 1).clamp(min=emin) - (p - 1))
    return torch.where(x != 0, sp, torch.full_like(x, 2.0 ** (emin - p + 1)))


def trunc16(x: torch.Tensor, dtype) -> torch.Tensor:
    """fp64 x truncated toward zero onto the 16-bit grid."""
    u = ulp16(x, dtype)
    return torch.sign(x) * torch.floor(x.abs() / u) * u


def half_check(out, ref, err, dtype, what):
    """out: the kernel's 16-bit values; ref: fp64 value of the operation on the same inputs; err: fp64 bound on |the kernel's
    value before its final rounding - ref|.  Asserts |out - ref| <= err + 1/2 ulp16(|ref| + err) everywhere and returns that
    bar (for the witnesses).  On failure the message says where the worst element sits."""
    bar = err + ulp16(ref.abs() + err, dtype) / 2
    d = (out.double() - ref).abs()
    q = d / bar
    ratio = q.max().item()
    print(f"[est-ref16] {what}: max|err|/bar = {ratio:.3f}")
    assert torch.isfinite(out.float()).all(), what
    if ratio > 1.0:
        at = tuple(int(i) for i in torch.unravel_index(q.argmax(), q.shape))
        over = (q > 1).double()
        prof = [over.mean(dim=[a for a in range(q.dim()) if a != ax]).topk(min(4, q.shape[ax])) for ax in range(q.dim())]
        raise AssertionError((what, ratio, at, d[at].item(), bar[at].item(), over.mean().item(),
                              [(p.values.tolist(), p.indices.tolist()) for p in prof]))
    return bar


def wit(delta, bar, what):
    """`witness` with this file's tag: applying this fault to the reference instead of the kernel turns the *_check red."""
    witness(delta, bar, "16 " + what)


def test_ulp16_is_the_grid_spacing():
    """At representable values the spacing to the next value up, at binade edges, in the subnormal range and at 0."""
    for dtype in DTYPES:
        tiny = 2.0 ** (-133 if dtype == torch.bfloat16 else -24)
        vals = torch.tensor([0.0, tiny, 3 * tiny, 2.0 ** -14, 2.0 ** -126 if dtype == torch.bfloat16 else 2.0 ** -14,
                             0.5, 1.0 - 2.0 ** -8 if dtype == torch.bfloat16 else 1.0 - 2.0 ** -11, 1.0, 1.5, 2.0, 3.0, 1000.0,
                             -1.0, -0.75], dtype=torch.float64)
        v16 = vals.to(dtype)
        assert torch.equal(v16.double(), vals)                           # every probe is representable
        up = (v16.abs().view(torch.int16) + 1).view(dtype).double()      # next value away from zero
        assert torch.equal(ulp16(vals, dtype), up - vals.abs()), dtype
        mid = vals.abs() + (up - vals.abs()) / 4                         # inside a binade: the same spacing
        assert torch.equal(ulp16(mid, dtype), up - vals.abs())
        assert torch.equal(trunc16(mid, dtype), vals.abs()) and torch.equal(trunc16(-mid, dtype), -vals.abs())


def test_intrinsic_probes():
    """No ulp table of rsqrtf / __expf / the reciprocal ships with the toolkit: the allowances above come from the ISA's
    1-ulp instructions.  This probe measures the torch-visible fp32 equivalents against fp64 on the inputs the kernels
    feed them (variances 1e-3 .. 1e3, exponents -30 .. 0, denominators 1 .. 1e3) and asserts they sit inside the same
    allowances.  It measures the intrinsics' class, not the kernels."""
    g = torch.Generator(device=DEV).manual_seed(1)
    v = torch.exp(torch.rand(1 << 16, generator=g, device=DEV) * 13.8 - 6.9)
    x = -30 * torch.rand(1 << 16, generator=g, device=DEV)
    rs = ((torch.rsqrt(v).double() - v.double() ** -0.5).abs() * v.double() ** 0.5).max().item()
    ex = ((torch.exp(x).double() / torch.exp(x.double()) - 1).abs() / r_exp(x.double())).max().item()
    rc = ((torch.reciprocal(v).double() * v.double() - 1).abs()).max().item()
    # gelu_erf's E (sea_common.hpp:135-141) with torch's fp32 operations against erf(|x| / sqrt 2) in fp64
    xg = torch.linspace(-8, 8, 1 << 18, device=DEV)
    t = 1 / (1 + (0.3275911 * 0.70710678118654752) * xg.abs())
    p = 1.061405429 * t - 1.453152027
    for c in (1.421413741, -0.284496736, 0.254829592):
        p = p * t + c
    E = 1 - p * t * torch.exp2(xg * xg * (-0.5 * 1.4426950408889634))
    ge = (E.double() - torch.erf(xg.double().abs() / math.sqrt(2))).abs().max().item()
    print(f"[est-ref16] probes: rsqrt {rs / 2 ** -23:.2f} ulp, exp {ex:.2f} of r_exp, reciprocal {rc / 2 ** -23:.2f} ulp, "
          f"gelu_erf's E {ge:.1e} (G_ERF {G_ERF:.1e})")
    assert rs <= R_RSQRT and ex <= 1.0 and rc <= R_RCP and ge <= G_ERF


# ---- 1. the predictor convolution ---------------------------------------------------------------------------------------
def conv16_launch(N, T, W, Cin, Cout, dil, pad_w, ks=3, zepi=False, H1=0):
    """(form, waves per workgroup, workgroups, work items per workgroup run) of a 16-bit `sea_causal_conv_c8` launch.
    ring_takes (sea_conv.hip:752-755): no z epilogue, 3 x 3, 64 -> 64 channels, W = 64, pad_w == dil <= 4 and
    N T >= 128 CUs -> `causal_conv_ring_kernel`, 4 waves, min(ceil(rows / 4), CUs) workgroups (:761-762); workgroup b walks
    rows [b per, (b + 1) per), per = ceil(rows / workgroups), 4 at a time (wave w: row r + w, :474-477).
    Otherwise launch_conv (:776-788): nt = ceil(Cout / 16) tiles, nwork = N T ceil(W / 64) work items; 8-wave workgroups
    when nt <= 3 or nt == 5 or nwork <= 16384, else 6; min(ceil(nwork / waves), 2 CUs) workgroups, at most CUs when the
    LDS image exceeds 80 KB; the same contiguous runs (sea_conv.hip:132-133), a wave steps by the workgroup's waves (:168)."""
    c = cus()
    rows = N * T
    if not zepi and ks == 3 and Cin == 64 and Cout == 64 and W == 64 and pad_w == dil and dil <= 4 and rows >= 128 * c:
        blocks = min((rows + 3) // 4, c)
        return "ring", 4, blocks, (rows + blocks - 1) // blocks
    nt, cinp = (Cout + 15) // 16, (Cin + 31) // 32 * 32
    nwork = rows * ((W + 63) // 64)
    lds = ks * ks * (cinp // 32) * 4 * (16 * nt) * 8 * 2 + 16 * nt * 4
    if zepi:
        lds += (nt + 1) // 2 * ((H1 + 15) // 16) * 64 * 16 + (H1 + 15) // 16 * 16 * 4
    nw = 8 if (nt <= 3 or nt == 5 or nwork <= 16384) else 6
    blocks = min((nwork + nw - 1) // nw, 2 * c)
    if lds > 80 * 1024:
        blocks = min(blocks, c)
    return f"reg{nw}", nw, blocks, (nwork + blocks - 1) // blocks


def conv_patches_fault(xl, flat, ks, dil, pad_w, fault):
    """`conv_patches` for the flat rows `flat` (over N T) with one fault built in.  "edge": a column tap that leaves the row
    reads the nearest pixel of the row instead of zero.  "leak": a tap row in the causal padding is not skipped but read
    from the rows in front of this one in memory (the previous sequence; row 0 for the very first rows)."""
    N, T, Cin, W = xl.shape
    xf = xl.reshape(N * T, Cin, W)
    t = flat % T
    taps = []
    for i in range(ks):
        back = (ks - 1 - i) * dil
        if fault == "leak":
            rows = xf[(flat - back).clamp(min=0)].double()
        else:
            rows = xf[(flat - back).clamp(min=0)].double() * (t - back >= 0).double().view(-1, 1, 1)
        rows = F.pad(rows, (pad_w, pad_w), mode="replicate" if fault == "edge" else "constant")
        for j in range(ks):
            taps.append(rows[:, :, j * dil:j * dil + W])
    return torch.stack(taps, 1).permute(0, 3, 1, 2).reshape(flat.numel(), W, ks * ks * Cin)


def conv16_reference(x, wt, b, ks, dil, pad_w):
    """fp64 convolution of the 16-bit C8 input x at EVERY row, chunks of 256 rows: acc (N T, W, Cout) before the ReLU, the
    bound `err` on the kernel's fp32 value, and the three structural witnesses as changes of acc: `drop` (every row),
    `edge` (rows, delta: the first 256 rows -- every row has the edge pixels), `leak` (rows t < 2 dil of every sequence)."""
    N, T, C8, W, _ = x.shape
    Cin, Cout, dtype = C8 * 8, wt.shape[0], x.dtype
    xl = c8_logical(x)
    wm = wt[:, :, :ks, :ks].to(dtype).double().permute(0, 2, 3, 1).reshape(Cout, ks * ks * Cin)
    bb = b.to(dtype).float().double()                                   # the bias as the op passes it
    cols = torch.arange(ks * ks * Cin, device=DEV).view(ks, ks, Cin)[ks - 1, 0, 8:16].reshape(-1)   # one 8-channel block of one tap
    n_all = torch.arange(N * T, device=DEV)
    accs, errs, drops = [], [], []
    for s in range(0, N * T, 256):
        fl = n_all[s:s + 256]
        P = conv_patches(xl, fl // T, fl % T, ks, dil, pad_w)
        accs.append(P @ wm.t() + bb)
        errs.append((ks * ks * Cin + 1) * U16 * (P.abs() @ wm.abs().t() + bb.abs()))
        drops.append(-(P[..., cols] @ wm[:, cols].t()))
    R = {"acc": torch.cat(accs), "err": torch.cat(errs), "drop": torch.cat(drops)}
    fl = n_all[:256]
    R["edge"] = (fl, conv_patches_fault(xl, fl, ks, dil, pad_w, "edge") @ wm.t() + bb - R["acc"][fl])
    fl = n_all[n_all % T < (ks - 1) * dil]
    R["leak"] = (fl, conv_patches_fault(xl, fl, ks, dil, pad_w, "leak") @ wm.t() + bb - R["acc"][fl])
    return R


def flat_rows(y):
    """C8 (N, T, C/8, W, 8) -> (N T, W, C)."""
    yl = c8_logical(y)
    return yl.permute(0, 1, 3, 2).reshape(-1, yl.shape[3], yl.shape[2])


def conv16_check(y, R, relu, dtype, what):
    """One launch's y against the reference R (`conv16_reference`) with or without the ReLU, and its witnesses."""
    act = torch.relu if relu else (lambda t: t)
    ref = act(R["acc"])
    bar = half_check(flat_rows(y), ref, R["err"], dtype, what)
    wit(act(R["acc"] + R["drop"]) - ref, bar, what + " (a) 8-channel block of a tap dropped")
    for key, name in (("edge", "(b) column tap off the row reads a pixel"), ("leak", "(c) causal padding read from earlier rows")):
        fl, dl = R[key]
        wit(act(R["acc"][fl] + dl) - ref[fl], bar[fl], f"{what} {name}")
    if dtype == torch.bfloat16 and not relu:
        frac = ((trunc16(ref, dtype) - ref).abs() > bar).double().mean().item()
        print(f"[est-ref16] {what} (d) truncating pack: outside the bar at {100 * frac:.1f} % of the elements")
        assert frac >= 0.10, (what, "a pack that truncates toward zero would pass", frac)


def conv_inputs(N, T, W, Cin, Cout, dtype, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((N, T, Cin // 8, W, 8), generator=g, device=DEV).to(dtype)
    wt = (torch.randn((Cout, Cin, 5, 3), generator=g, device=DEV) * (Cin * 9) ** -0.5).to(dtype)
    b = (torch.randn(Cout, generator=g, device=DEV) * 0.1).to(dtype)
    return x, wt, b


def run_conv_case(ops, N, T, W, Cin, Cout, dil, dtype, form, what):
    assert conv16_launch(N, T, W, Cin, Cout, dil, dil)[0] == form, (what, conv16_launch(N, T, W, Cin, Cout, dil, dil))
    x, wt, b = conv_inputs(N, T, W, Cin, Cout, dtype, 1000 * dil + T + Cout)
    R = conv16_reference(x, wt, b, 3, dil, dil)
    for relu in (True, False):
        y = ops.causal_conv_c8(x, wt, b, 3, dil, dil, relu=relu)
        conv16_check(y, R, relu, dtype, f"{what} {str(dtype)[6:]} relu={int(relu)}")


def ragged_n():
    """Sequences of 3701 rows for the ragged ring launch: the fewest that reach 128 rows per CU and leave a per-workgroup run
    that is no multiple of the ring's 4 waves (256 CUs: 9 x 3701 = 33309 rows, 131 per run, sequence starts in mid-run)."""
    n = -(-128 * cus() // 3701)
    while conv16_launch(n, 3701, 64, 64, 64, 2, 2)[3] % 4 == 0:
        n += 1
    return n


@pytest.mark.parametrize("ragged,dil,dtype", [(False, 2, torch.bfloat16), (True, 2, torch.bfloat16), (False, 1, torch.bfloat16),
                                              (True, 3, torch.bfloat16), (True, 2, torch.float16)])
def test_conv16_ring_form(ops, ragged, dil, dtype):
    """64 -> 64 channels, W = 64, pad_w == dil, N T >= 128 CUs: `causal_conv_ring_kernel`, one 4-wave workgroup per CU, each
    walking a contiguous run of >= 128 rows; ragged: the run length is no multiple of 4 (the last step's waves 3.. idle) and
    sequences start in mid-run (the halo rows of a run and the causal padding of a sequence fall together).  With and
    without the ReLU against one reference."""
    N, T = (ragged_n(), 3701) if ragged else (-(-128 * cus() // 4096), 4096)
    form, nw, blocks, per = conv16_launch(N, T, 64, 64, 64, dil, dil)
    assert blocks == cus() and per >= 128 and (not ragged or (per % 4 and T % per))
    run_conv_case(ops, N, T, 64, 64, 64, dil, dtype, "ring", f"conv ring {N}x{T} dil{dil}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name,N,T,W,C,form", [
    ("6-wave", 5, 4096, 64, 64, "reg6"),          # 16384 < N T < 128 CUs: the register form's 6-wave workgroups, two per CU
    ("8-wave", 2, 4096, 64, 64, "reg8"),          # N T <= 16384
    ("80ch", 2, 3000, 64, 80, "reg8"),            # nt = 5, the 138 KB image: ONE workgroup per CU
    ("24ch", 1, 1000, 64, 24, "reg8"),            # nt = 2 (H = 12)
    ("w128", 1, 700, 128, 64, "reg8"),            # ONESEG = false: two 64-pixel work items per row (T_M = 512)
])
def test_conv16_register_form(ops, name, N, T, W, C, form, dtype):
    """`causal_conv_c8_kernel` at the smallest launches that reach each of its geometries (dil 2), every row."""
    nw, blocks, per = conv16_launch(N, T, W, C, C, 2, 2)[1:]
    if name == "6-wave":
        assert 16384 < N * T < 128 * cus() and per % 6                # runs end in a step with idle waves
    if name == "80ch":
        assert blocks == cus() and per > nw                            # one workgroup per CU, several passes each
    run_conv_case(ops, N, T, W, C, C, 2, dtype, form, f"conv {name} {N}x{T}")


# ---- 2. the 1x1 epilogue, 3. the tail -----------------------------------------------------------------------------------
# (name, N, T, W4, C, H): conv 3 x 3 C -> C with the 1x1 C -> H in its epilogue; T_M = 4 W4
ZCASES = {
    "c64h32": (2, 2048, 64, 64, 32),              # NT = 4: whole tile pairs
    "c80h40": (2, 2048, 64, 80, 40),              # NT = 5: the odd tile's shuffle path, 3 head tiles
    "c24h12": (2, 2048, 64, 24, 12),              # blk < C8o, heads padded to 16
    "w24": (2, 2048, 24, 64, 32),                 # T_M = 96: masked pixels and lanes
    "w128": (1, 600, 128, 24, 12),                # T_M = 512 (E = 8), ONESEG = false
}
_Z = {}


def zcase(ops, name, dtype):
    """One launch of `causal_conv_c8_z(want_y=True)` per (case, dtype), shared by the tests of sections 2 and 3."""
    key = (name, dtype)
    if key not in _Z:
        N, T, W4, C, H = ZCASES[name]
        T_M = 4 * W4
        x, wt, b = conv_inputs(N, T, W4, C, C, dtype, 31 * C + W4)
        g = torch.Generator(device=DEV).manual_seed(C + H + W4)
        cw = (torch.randn((H, C), generator=g, device=DEV) * C ** -0.5).to(dtype)
        cb = (torch.randn(H, generator=g, device=DEV) * 0.1).to(dtype)
        lw = (torch.rand(T_M, generator=g, device=DEV) + 0.5).to(dtype)
        lb = (torch.randn(T_M, generator=g, device=DEV) * 0.1).to(dtype)
        assert ops.conv_z_supported(C, H, 3, W4)
        y, z = ops.causal_conv_c8_z(x, wt, b, 3, 2, 2, cw, cb, lw, lb, relu=True, want_y=True)
        _Z[key] = dict(x=x, wt=wt, b=b, cw=cw, cb=cb, lw=lw, lb=lb, y=y, z=z, T_M=T_M, H=H, C=C)
    return _Z[key]


def z_reference(Z, swap=None, drop=None):
    """fp64 1x1 convolution of the 16-bit y: (N T, W4, H) and the (C + 1) U16 bound.  `drop`: channels left out; `swap`:
    two channel ranges exchanged in y (witnesses)."""
    yl = flat_rows(Z["y"]).double()
    w1, b1 = Z["cw"].double(), Z["cb"].double()
    if swap is not None:
        yl = yl.clone()
        a, bb = swap
        yl[..., a], yl[..., bb] = yl[..., bb].clone(), yl[..., a].clone()
    if drop is not None:
        w1 = w1.clone()
        w1[:, drop] = 0
    return yl @ w1.t() + b1, (Z["C"] + 1) * U16 * (yl.abs() @ w1.abs().t() + b1.abs())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", list(ZCASES))
def test_conv16_z_epilogue(ops, name, dtype):
    """`causal_conv_c8_z(want_y=True)`: y against the fp64 convolution like section 1 (the z epilogue never takes the ring
    form), z against fp64 from the y of the same launch.  2 x 2048 rows: every workgroup walks several rows."""
    N, T, W4, C, H = ZCASES[name]
    Z = zcase(ops, name, dtype)
    form, nw, blocks, per = conv16_launch(N, T, W4, C, C, 2, 2, zepi=True, H1=H)
    assert form.startswith("reg") and (name == "w128" or per >= 8)
    what = f"conv+z {name} {str(dtype)[6:]}"
    conv16_check(Z["y"], conv16_reference(Z["x"], Z["wt"], Z["b"], 3, 2, 2), True, dtype, what + " y")
    zk = Z["z"].permute(0, 1, 3, 2).reshape(N * T, W4, H)
    ref, err = z_reference(Z)
    bar = fp32_check(zk, ref, err, what + " z")
    wit(z_reference(Z, drop=slice(8, 16))[0] - ref, bar, what + " z: one 8-channel k-block dropped")
    if C == 80:
        wit(z_reference(Z, swap=(slice(64, 72), slice(72, 80)))[0] - ref, bar, what + " z: channels 64-71 <-> 72-79")


def area_taps(W4, up, T_M):
    """adaptive_avg_pool's windows over the Wp = up W4 + 2 padded pixels as indices into [bias, z upsampled x up, bias, 0]:
    (T_M, 3) indices (unused taps -> the zero slot Wp) and the tap counts.  floor / ceil in exact integer arithmetic."""
    Wp = W4 * up + 2
    j = torch.arange(T_M)
    xs, xe = (j * Wp) // T_M, -((-(j + 1) * Wp) // T_M)
    idx = xs.view(-1, 1) + torch.arange(3).view(1, 3)
    idx = torch.where(idx < xe.view(-1, 1), idx, torch.full_like(idx, Wp))
    return idx, xe - xs


def test_area_taps_are_adaptive_avg_pool():
    for W4, T_M in ((64, 256), (24, 96), (128, 512)):
        idx, cnt = area_taps(W4, 4, T_M)
        assert cnt.min() >= 1 and cnt.max() <= 3
        v = torch.randn(3, 4 * W4 + 2, dtype=torch.float64)
        got = F.pad(v, (0, 1))[:, idx].sum(-1) / cnt
        assert torch.allclose(got, F.adaptive_avg_pool1d(v, T_M), rtol=0, atol=1e-14)


def ln_fp32(a, ea, g, b, eps, n, unbiased=False):
    """LayerNorm over the last axis (n terms) of values a known to within ea, as the kernels evaluate it in fp32
    (sea_tail.hpp:283-316, sea_mlp.hip:204-220 / :263-284): the sum of n terms in any order (n U sum|a|), the 1/n multiply,
    a - mean, the squares and their sum, the 1/n multiply and + eps, rsqrtf, then (a - mean) rstd g + b (three roundings).
    Returns the fp64 value and the bound on the kernel's fp32 value."""
    m = a.sum(-1, keepdim=True) / n
    em = (ea.sum(-1, keepdim=True) + n * U * a.abs().sum(-1, keepdim=True)) / n + 2 * U * m.abs()
    d = a - m
    ed = ea + em + U * d.abs()
    q = (d * d).sum(-1, keepdim=True)
    eq = (2 * d.abs() * ed + ed * ed).sum(-1, keepdim=True) + (n + 1) * U * q
    v = q / (n - 1 if unbiased else n) + eps
    ev = eq / n + 3 * U * v
    rstd = v ** -0.5
    er = rstd * ev / (2 * v) * (1 + 1e-3) + R_RSQRT * rstd
    s = d * rstd * g + b
    es = (g.abs() * (ed * rstd + d.abs() * er + ed * er) + 3 * U * ((d * rstd * g).abs() + b.abs())) * (1 + 1e-3)
    return s, es


def tail_reference(z, ez, cb, lw, lb, T_M, eps, fault=None):
    """fp64 tail from z (..., H, W4) with |kernel's z - z| <= ez: returns scores, probs and the bounds (es, ep) on the
    kernel's fp32 values before their final rounding, following sea_tail.hpp:283-349 line by line (see the module docstring).
    `fault`: "tap" (the window's last tap dropped), "shift" (gamma / beta one lane slot on), "unbiased" (variance / (T_M - 1))."""
    W4 = z.shape[-1]
    idx, cnt = area_taps(W4, 4, T_M)
    idx, cnt = idx.to(z.device), cnt.to(z.device).double()
    bcol = cb.view(-1, 1).expand(*z.shape[:-1], 1)
    row = torch.cat([bcol, z.repeat_interleave(4, -1), bcol, torch.zeros_like(bcol)], -1)
    erow = torch.cat([0 * bcol, ez.repeat_interleave(4, -1), 0 * bcol, 0 * bcol], -1)
    taps, etaps = row[..., idx], erow[..., idx].sum(-1)                  # (..., H, T_M, 3)
    if fault == "tap":
        last = (cnt.long() - 1).view(-1, 1) == torch.arange(3, device=z.device).view(1, 3)
        taps = taps * (~last).double()
    a = taps.sum(-1) / cnt
    ea = etaps / cnt + 5 * U * (taps.abs().sum(-1) + etaps) / cnt
    if fault == "shift":
        E = (T_M + 63) // 64
        lw, lb = torch.roll(lw, E), torch.roll(lb, E)
    s, es = ln_fp32(a, ea, lw, lb, eps, T_M, unbiased=fault == "unbiased")
    p = torch.softmax(s, -1)
    X = s.max(-1, keepdim=True).values - s + 2 * es.max(-1, keepdim=True).values      # |exponent argument|
    rx = U * X + r_exp(X)
    rel = 2 * es.max(-1, keepdim=True).values + rx + rx.max(-1, keepdim=True).values + (T_M + 2) * U
    return s, es, p, p * torch.expm1(rel)


def tail_check(scores, probs, z, ez, Z, dtype, what):
    """scores / probs (N, H, T, T_M) of one tail launch against fp64 from z (N, T, H, W4), with the witnesses."""
    cb, lw, lb, T_M = Z["cb"].double(), Z["lw"].double(), Z["lb"].double(), Z["T_M"]
    s, es, p, ep = tail_reference(z, ez, cb, lw, lb, T_M, 1e-5)
    sk, pk = scores.permute(0, 2, 1, 3), probs.permute(0, 2, 1, 3)
    bs = half_check(sk, s, es, dtype, what + " scores")
    bp = half_check(pk, p, ep, dtype, what + " probs")
    for fault, name in (("tap", "the window's last tap dropped"), ("shift", "gamma/beta one lane slot on")):
        sf, _, pf, _ = tail_reference(z, ez, cb, lw, lb, T_M, 1e-5, fault)
        wit(sf - s, bs, f"{what} scores: {name}")
        wit(pf - p, bp, f"{what} probs: {name}")
    sf = tail_reference(z, ez, cb, lw, lb, T_M, 1e-5, "unbiased")[0]
    print(f"[est-ref16] {what} scores: unbiased variance {((sf - s).abs() / bs).max().item():.1f} x bar (reported, no assert)")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("name", ["c64h32", "c80h40", "c24h12", "w24", "w128"])
def test_tail16_from_z_and_from_y(ops, name, dtype):
    """`predictor_tail_z` on the z of section 2 (FULLROW T_M = 256; 96: W4 = 24, masked lanes; 512: E = 8; 32, 40, 12 heads)
    against fp64 from that z, and `predictor_tail` on the C8 y (the MFMA variant `tail_z_tile`) against fp64 from y, whose z
    carries the 1x1's (C + 1) U16 term.  c64h32 / bf16 also holds the map of `predictor_tail_select` to the same bar."""
    Z = zcase(ops, name, dtype)
    N, T, W4, C, H = ZCASES[name]
    a = (Z["cw"], Z["cb"], Z["lw"], Z["lb"])
    what = f"tail {name} {str(dtype)[6:]}"
    p, s = ops.predictor_tail_z(Z["z"], *a, up=4, T_m=Z["T_M"], dtype=dtype, want_scores=True)
    zd = Z["z"].double()
    tail_check(s, p, zd, torch.zeros_like(zd), Z, dtype, what + " from z")
    p2, s2 = ops.predictor_tail(Z["y"], *a, up=4, T_m=Z["T_M"], want_scores=True)
    zr, ez = z_reference(Z)
    zr, ez = (t.view(N, T, W4, H).permute(0, 1, 3, 2) for t in (zr, ez))
    tail_check(s2, p2, zr, ez, Z, dtype, what + " from y")
    if name == "c64h32" and dtype == torch.bfloat16:
        keep = ops.keep_table_causal(H, T, Z["T_M"], 64, device=DEV)
        p3, s3, _ = ops.predictor_tail_select(Z["y"], *a, up=4, T_m=Z["T_M"], keep=keep, k=64, T_src=T, want_scores=True)
        sr, es, pr, ep = tail_reference(zr, ez, Z["cb"].double(), Z["lw"].double(), Z["lb"].double(), Z["T_M"], 1e-5)
        half_check(s3.permute(0, 2, 1, 3), sr, es, dtype, what + " select scores")
        half_check(p3.permute(0, 2, 1, 3), pr, ep, dtype, what + " select probs")


# ---- 4. the fused MLP -----------------------------------------------------------------------------------------------------
G_ERF = 2.0 ** -19              # |E - erf(|x| / sqrt 2)| of gelu_erf (sea_common.hpp:134-144): Abramowitz & Stegun 7.1.26 (1.5e-7)
                                # + its fp32 evaluation on v_rcp_f32 / v_exp_f32 (t to 1.5 ulp through a polynomial of slope
                                # <= 3.5, four fma roundings, the exponential's ulp and argument: <= 1.4e-6 together)
GELU_LIP = 1.13                 # max |GELU'| (at x = sqrt 2 * 1.0...: 1.1289)


def rn16(x, dtype):
    """fp64 x rounded to nearest-even onto the 16-bit grid (no detour through fp32: no double rounding)."""
    u = ulp16(x, dtype)
    return torch.round(x / u) * u


def flip_delta(a, ea, dtype):
    """The Linear's 16-bit output is not exposed.  The kernel rounds a value within ea of a, and rounding is monotone: its
    result lies between rn16(a - ea) and rn16(a + ea).  Returns r = rn16(a) and delta >= |kernel's rounded value - r|:
    zero unless a lies within ea of a rounding midpoint (then one ulp16, more only where ea exceeds the spacing)."""
    r = rn16(a, dtype)
    return r, torch.maximum((rn16(a + ea, dtype) - r).abs(), (rn16(a - ea, dtype) - r).abs())


def ln_flip_bound(r, delta, g, eps):
    """|LayerNorm(r + e) - LayerNorm(r)| for |e_j| <= delta_j over the last axis.  With xh = (r - mean) rstd,
    d o_i / d r_j = g_i rstd ([i = j] - 1/D - xh_i xh_j / D), so to first order
        |g_i| rstd (delta_i + mean(delta) + |xh_i| mean(|xh| delta)).
    Second order: the relative change of rstd and of the mean are at most k = rstd (mean(delta) + mean(|xh| delta)), and the
    variance's own e^2 term moves rstd by rstd^3 mean(delta^2) / 2: an explicit |g_i| (|xh_i| + 1) (2 k^2 + rstd^2
    mean(delta^2)) plus a 5 % margin on the first-order term, justified by max delta rstd << 1 -- asserted (<= 1/16)."""
    m = r.mean(-1, keepdim=True)
    d = r - m
    rstd = ((d * d).mean(-1, keepdim=True) + eps) ** -0.5
    xh = d * rstd
    md, mxd = delta.mean(-1, keepdim=True), (xh.abs() * delta).mean(-1, keepdim=True)
    assert (delta * rstd).max().item() <= 1 / 16, "the flip bound's second-order margin needs delta * rstd << 1"
    first = g.abs() * rstd * (delta + md + xh.abs() * mxd)
    k = rstd * (md + mxd)
    second = g.abs() * (xh.abs() + 1) * (2 * k * k + rstd * rstd * (delta * delta).mean(-1, keepdim=True))
    return 1.05 * first + second


def gelu64(o):
    return 0.5 * o * (1 + torch.erf(o / math.sqrt(2)))


def mlp_params(d, T_M, H, dtype):
    """The five modules of `test_predictor_mlp`, drawn the same way; returns them on the device in `dtype` and their
    parameters as the kernel sees them (rounded to dtype) in fp64."""
    import copy
    nn = torch.nn
    g = torch.Generator().manual_seed(5)
    Din, D1, Wd = 3 * d, 2 * d, T_M // 4
    mods = [nn.Linear(Din, D1), nn.LayerNorm(D1), nn.Linear(D1, 2 * Wd), nn.LayerNorm(Wd), nn.Linear(D1, 2)]
    with torch.no_grad():
        for m in mods:
            for prm in m.parameters():
                prm.copy_(torch.randn(prm.shape, generator=g) * (0.3 if prm.dim() == 1 else prm.shape[-1] ** -0.5))
        mods[1].weight.add_(1.0); mods[3].weight.add_(1.0)
    dev = [copy.deepcopy(m).to(DEV).to(dtype) for m in mods]
    P = {}
    for name, m in zip(("enc", "ln0", "dec", "ln1", "sc"), dev):
        P[name + "_w"], P[name + "_b"] = m.weight.detach().double(), m.bias.detach().double()
    return dev, P


def mlp_stage1(x, P, dtype, eps, fault=None):
    """tpred before its final rounding, in fp64 from the 16-bit x (rows, Din), and the bound on the kernel's fp32 value:
    Linear on the MFMA ((Din + 1) U16 sum|terms|, sea_mlp.hip:178/189 + the bias add :202) -> round16 (:202-203, flip-aware)
    -> LayerNorm(D1) in fp32 (:204-220) -> gelu_erf (:222).  Faults: "kstep" (inputs 32..63 never multiplied), "gamma" (gamma
    rolled by 4 inside the first 16-feature tile)."""
    W, b, g, be = P["enc_w"], P["enc_b"], P["ln0_w"], P["ln0_b"]
    Din = W.shape[1]
    if fault == "kstep":
        W = W.clone(); W[:, 32:64] = 0
    if fault == "gamma":
        g = g.clone(); g[:16] = torch.roll(g[:16], 4)
    a = x @ W.t() + b
    ea = (Din + 1) * U16 * (x.abs() @ W.abs().t() + b.abs())
    r, delta = flip_delta(a, ea, dtype)
    o, eo = ln_fp32(r, torch.zeros_like(r), g, be, eps, r.shape[-1])[:2]
    eo = eo + ln_flip_bound(r, delta, g, eps)
    t = gelu64(o)
    et = GELU_LIP * eo + 0.5 * o.abs() * G_ERF + 3 * U * (t.abs() + o.abs())
    return t, et


def mlp_stage2(tp, P, dtype, eps, Wd, fault=None):
    """The decoder from the kernel's own tpred (rows, D1), bit for bit the B operand of the second product: Linear on the
    MFMA ((D1 + 1) U16, sea_mlp.hip:243 + :262) -> round16 (:262, flip-aware) -> LayerNorm(Wd) per split in fp32 (:263-284),
    PADW rows outside the statistics.  Returns (rows, 2, Wd) before the final rounding, its bound, and the gates' Linear (value,
    MFMA bound).  Faults: "kstep" (features 32..63 of tpred never multiplied), "gamma" (gamma rolled by 4 in the first tile),
    "joint" (LayerNorm statistics over both splits together), "perm" (tiles 0 and 1 of tpred swapped: the decoder's K
    permutation undone for one tile pair)."""
    W, b, g, be = P["dec_w"], P["dec_b"], P["ln1_w"], P["ln1_b"]
    D1 = W.shape[1]
    tq = tp
    if fault == "kstep":
        W = W.clone(); W[:, 32:64] = 0
    if fault == "gamma":
        g = g.clone(); g[:16] = torch.roll(g[:16], 4)
    if fault == "perm":
        tq = torch.cat([tp[:, 16:32], tp[:, :16], tp[:, 32:]], 1)
    c = tq @ W.t() + b
    ec = (D1 + 1) * U16 * (tq.abs() @ W.abs().t() + b.abs())
    r, delta = flip_delta(c, ec, dtype)
    r, delta = r.view(-1, 2, Wd), delta.view(-1, 2, Wd)
    if fault == "joint":
        m = r.mean((1, 2), keepdim=True)
        o = (r - m) * (((r - m) ** 2).mean((1, 2), keepdim=True) + eps) ** -0.5 * g + be
        return o, None, None, None
    o, eo = ln_fp32(r, torch.zeros_like(r), g, be, eps, Wd)[:2]
    eo = eo + ln_flip_bound(r, delta, g, eps)
    s = tp @ P["sc_w"].t() + P["sc_b"]
    es = (D1 + 1) * U16 * (tp.abs() @ P["sc_w"].abs().t() + P["sc_b"].abs())
    return o, eo, s, es


MLP_CASES = [
    (1, 32, 4096, 64, 256),      # several items per wave of the persistent grid, PACK off
    (1, 12, 2048, 64, 256),      # PACK (H % 16 != 0, launch_mlp sea_mlp.hip:344)
    (1, 40, 1024, 128, 256),     # W1S: streamed encoder weights (sea_mlp.hip:371) + PACK
    (1, 12, 1024, 64, 96),       # PADW: Wd = 24 (sea_mlp.hip:347)
    (1, 20, 1024, 80, 256),      # d = 80
    (3, 32, 1, 64, 256),         # nitems < 256 waves: the `spread` placement of a decode-sized launch (sea_mlp.hip:360)
]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N,H,T,d,T_M", MLP_CASES)
def test_mlp16_stage_by_stage(ops, dtype, N, H, T, d, T_M):
    """`predictor_mlp`, every row: tpred against fp64 from x; the C8 decoder output and the two gates against fp64 from the
    kernel's own tpred."""
    Din, D1, Wd = 3 * d, 2 * d, T_M // 4
    nitems = -(-N * T * H // 16) if H % 16 else N * T * (H // 16)
    nw = 16 if D1 // 16 + 2 * (-(-Wd // 16)) <= 16 and D1 != 256 else 8
    if T == 1:
        assert nitems < 256 * nw                                       # spread
    if (N, H, T) == (1, 32, 4096):
        assert nitems >= 2 * 256 * nw                                  # a wave takes several items
    (enc, ln0, dec, ln1, sc), P = mlp_params(d, T_M, H, dtype)
    g = torch.Generator(device=DEV).manual_seed(N * H * T + d)
    x = torch.randn((N, H, T, Din), generator=g, device=DEV).to(dtype)
    x_c8, tp, rs, av = ops.predictor_mlp(x, enc, ln0, dec, ln1, sc, want_tpred=True)
    what = f"mlp {N}x{H}x{T} d{d} T_M{T_M} {str(dtype)[6:]}"
    # stage 1
    xd = x.double().view(-1, Din)
    t, et = mlp_stage1(xd, P, dtype, ln0.eps)
    bar = half_check(tp.view(-1, D1), t, et, dtype, what + " tpred")
    for fault, name in (("kstep", "one 32-input k-step dropped"), ("gamma", "gamma rolled by 4 inside a tile")):
        wit(mlp_stage1(xd, P, dtype, ln0.eps, fault)[0] - t, bar, f"{what} tpred: {name}")
    # stage 2, from the kernel's tpred
    tpd = tp.double().view(-1, D1)
    o, eo, s, es = mlp_stage2(tpd, P, dtype, ln1.eps, Wd)
    yk = c8_logical(x_c8).reshape(N, T, H, 2, Wd).permute(0, 2, 1, 3, 4).reshape(-1, 2, Wd)       # channel = 2 h + split
    bar = half_check(yk, o, eo, dtype, what + " decoder")
    for fault, name in (("kstep", "one 32-feature k-step dropped"), ("gamma", "gamma rolled by 4 inside a tile"),
                        ("joint", "statistics over both splits"), ("perm", "tpred tiles 0 <-> 1")):
        wit(mlp_stage2(tpd, P, dtype, ln1.eps, Wd, fault)[0] - o, bar, f"{what} decoder: {name}")
    # gates: Linear -> round16 -> sigmoid in fp32 (sea_mlp.hip:249-251).  A flip moves the gate by at most delta / 4 (max
    # slope of the sigmoid); 1 / (1 + __expf(-s)): the exponential's allowance, the add, the division.
    sr, ds = flip_delta(s, es, dtype)
    gate = torch.sigmoid(sr)
    eg = ds / 4 + gate * (r_exp(sr) + 2 * U + R_RCP)
    gk = torch.stack([rs, av], -1).view(-1, 2)
    bar = fp32_check(gk, gate, eg, what + " gates")
    s_f = tpd[:, 32:] @ P["sc_w"][:, 32:].t() + P["sc_b"]               # fault: the gates' first k-step dropped
    wit(torch.sigmoid(rn16(s_f, dtype)) - gate, bar, what + " gates: one k-step dropped")
