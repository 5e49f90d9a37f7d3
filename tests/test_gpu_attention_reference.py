"""-m gpu: the PLAIN prefill launches of the fused sparse attention -- the gather kernels of csrc/sea_attn.hip on an emitted
CSR (`ops.sparse_attention(path="gather")`) and the MFMA tile kernel of csrc/sea_attn_tile.hip (`path="tile"`) -- held to an
INDEPENDENT reference: the oracle's selection and interpolation on the CPU and an fp64 softmax over each (n, h, t) list's kept
keys (`Reference` of tests/test_gpu_decode_reference.py).  The fused-interpolation, row-pool and key-range forms are tied to
these launches (bit for bit, or by a bound in the gather launch's own error); this file is where that error is bounded.

Inputs are made on the CPU with a seeded generator, so what each case is there for is asserted from the oracle's CSR without
a GPU (`check_inputs`, `check_mutations`, `test_case_set_statistics`).  In what the kernels read every K / V row that no kept
key names is poisoned -- NaN in K and V for the gather kernels, NaN in K and a huge finite value in V for the tile kernel
(it multiplies a staged neighbour's V row by an exact 0: the contract of test_empty_rows_and_non_finite_padding_keys) -- so a
neighbour's row shows in the result.

Bars
  * fp32 output of the gather kernels against fp64: TOL32, four times the largest max |err| observed over the cases of this
    file on MI355X (the margin of the decode-probabilities work: builds and rounding patterns differ).
  * fp32 output of the tile kernel: TOL32 plus, per list, (u + L * 2^-25 [fp16]) * max |V over the list's keys| * row_scale
    * mix -- derived in `tile_bound`.
  * 16-bit output: within 1 ulp of the fp64 value rounded to the output type, plus the fp32 bar (`check_outputs` of the
    decode file).
  * per-entry probabilities rs * softmax: TOL_P, measured like TOL32.
The comparison can fail: dropping the last entry of every list, or moving every list's first key to a neighbour that is not
kept, moves at least 90 % of the lists concerned by more than 10 * TOL32 (`check_mutations`, on the CPU in fp64).

Printed per case and form ("[attn-ref] ..."): max |err|, max |ref|, and for the tile kernel the derived bound next to the
measured error; MI355X values are in DESIGN.md 5.4j.
"""
import functools
import zlib

import pytest
import torch

from oracle import sea_oracle as O
from sea_attention_amd.perlin_attention import ops
from test_gpu_decode_reference import Reference, oracle_columns, ulp, unpack_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

# fp32 context of the gather kernels against fp64: the largest max |err| over every case and form of this file observed on
# MI355X is 7.1e-7 (rows80_bf16, plain form; outputs up to 4.4; the decode file saw 4.9e-7); the bar is four times that
TOL32 = 2.8e-6
# per-entry rs * softmax (values in [0, 1]) against fp64: observed 1.15e-7 (rows80_bf16); four times that
TOL_P = 4.6e-7

KEEP_CYCLE = (0, 1, 2, 3, 5, 8, 13, 21, 34, 40)      # kept pixels per query row, cycled: empty rows up to most of a head
BF, FH, F32 = torch.bfloat16, torch.float16, torch.float32

# name: (kernel, dtype, d, N, H, T_dst, T_src, T_m, max_k, causal, strided, one_entry)
#   kernel: what launch_attn_wp / launch_attn_tile choose (asserted from the device tensors' strides by `dispatch`):
#     "rows<L>"  sparse_attn_rows_kernel, L lanes per row       "rows80"  sparse_attn_rows80_kernel
#     "wave<L>"  sparse_attn_kernel (a wave per row), L lanes   "tile"    sparse_attn_tile_kernel
#   strided: q / k / v are views of one fused (N, T_src, 3, H, d) projection.
#   one_entry: False where no list of one entry can exist -- every query row's pixels are at least two keys wide (the
#     narrowest row sees T_src - T_dst + 1 keys, T_m pixels) -- asserted in check_inputs.
CASES = {
    "rows4_f32_d16":    ("rows4", F32, 16, 2, 5, 70, 70, 32, 4, True, False, True),
    "rows4_bf16_d32":   ("rows4", BF, 32, 1, 4, 150, 333, 32, 8, True, False, False),
    "rows8_f32_d32":    ("rows8", F32, 32, 1, 6, 100, 100, 32, 8, True, True, True),
    "rows8_bf16_d64":   ("rows8", BF, 64, 1, 2, 620, 1100, 32, 16, True, False, False),       # lists of > 256 entries
    "rows8_fp16_d64":   ("rows8", FH, 64, 2, 3, 90, 150, 64, 4, True, False, True),
    "rows16_f32_d64":   ("rows16", F32, 64, 2, 3, 45, 45, 32, 4, True, False, True),
    "rows16_bf16_d128": ("rows16", BF, 128, 1, 2, 618, 1100, 32, 16, True, False, False),    # lists of > 256 entries
    "rows16_fp16_d128": ("rows16", FH, 128, 1, 4, 50, 90, 64, 4, False, False, True),        # not causal
    "rows80_bf16":      ("rows80", BF, 80, 1, 2, 620, 1100, 32, 16, True, False, False),     # lists of > 256 entries
    "rows80_fp16":      ("rows80", FH, 80, 2, 3, 75, 75, 32, 8, True, True, True),
    "wave32_f32_d128":  ("wave32", F32, 128, 1, 3, 41, 41, 32, 4, True, False, True),
    "wave32_bf16_d256": ("wave32", BF, 256, 2, 2, 30, 77, 64, 4, True, False, True),
    "wave64_f32_d256":  ("wave64", F32, 256, 1, 2, 37, 100, 64, 8, True, False, True),
    # K / V rows 976136 elements apart: T_src * pitch * 2 bytes >= 2^31, the `small` test of launch_attn_wp fails
    "wave8_bf16_pitch": ("wave8", BF, 64, 1, 3, 150, 1100, 256, 16, True, False, False),
    "tile_bf16_d64":    ("tile", BF, 64, 2, 3, 150, 150, 64, 8, True, True, True),
    "tile_fp16_d64":    ("tile", FH, 64, 1, 4, 37, 200, 32, 8, True, False, False),
    "tile_bf16_d80":    ("tile", BF, 80, 1, 5, 53, 300, 32, 16, True, False, False),
    "tile_fp16_d80":    ("tile", FH, 80, 2, 3, 120, 120, 64, 4, True, False, True),
    "tile_bf16_d128":   ("tile", BF, 128, 1, 3, 41, 170, 32, 8, True, False, False),
    "tile_fp16_d128":   ("tile", FH, 128, 1, 6, 100, 100, 32, 8, True, False, True),
}
PITCH = 976136                                        # wave8_bf16_pitch: elements between consecutive K (and V) rows
LONG = ("rows8_bf16_d64", "rows16_bf16_d128", "rows80_bf16")
# (row_tiles, key_window) every tile case runs: the defaults (one row tile, a 2048-key window halved down to T_src), two row
# tiles, and 64-key windows (every case has T_src > 64: lists cross window boundaries, asserted in check_inputs)
TILE_FORMS = ((0, 0), (2, 0), (1, 64), (2, 64))
PROBS_CASES = ("rows4_f32_d16", "rows8_fp16_d64", "rows16_bf16_d128", "rows80_bf16", "wave32_f32_d128", "wave64_f32_d256",
               "wave8_bf16_pitch")


class ListReference(Reference):
    """`Reference` that also keeps every list's fp64 softmax (the per-entry probabilities before the row scale)."""

    def __init__(self, *a, **kw):
        self.p, self._building = {}, True
        super().__init__(*a, **kw)
        self._building = False

    def head(self, n, h, t, keys):
        o, p = super().head(n, h, t, keys)
        if self._building:
            self.p[n, h, t] = p
        return o, p


class Case:
    """Inputs (CPU), the oracle's selection and columns, the list statistics and the fp64 reference of one case."""

    def __init__(self, name, spec=None):
        (self.kernel, self.dtype, self.d, self.N, self.H, self.T_dst, self.T_src, self.T_m, self.k, self.causal, self.strided,
         self.one_entry) = spec if spec is not None else CASES[name]
        self.name = name
        N, H, T_dst, T_src, T_m, d = self.N, self.H, self.T_dst, self.T_src, self.T_m, self.d
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
        probs = torch.softmax(torch.randn((N, H, T_dst, T_m), generator=g), -1)
        probs[:, H - 1] += 0.6 / T_m                     # a mild bias (the mean probability is 1 / T_m): one head gets the long lists
        self.probs = probs
        self.keep = torch.tensor(KEEP_CYCLE, dtype=torch.int32).repeat(-(-T_dst // len(KEEP_CYCLE)))[:T_dst].contiguous()
        assert int(self.keep.max()) <= H * T_m
        self.mask = O.grouped_topk_mask(probs, self.keep)
        self.crow, self.col = O.resize_m_to_t_csr(self.mask, self.k, target_width=T_src, is_causal=self.causal)
        self.q = (torch.randn((N, H, T_dst, d), generator=g) * d ** -0.5).to(self.dtype)
        self.kk = torch.randn((N, H, T_src, d), generator=g).to(self.dtype)
        self.vv = torch.randn((N, H, T_src, d), generator=g).to(self.dtype)
        self.rs = torch.rand((N, H, T_dst), generator=g) * 0.5 + 0.5
        self.mix = torch.rand((N, H, T_dst), generator=g) * 0.5 + 0.5
        self.avg = torch.randn((N, H, T_dst, d), generator=g).to(self.dtype)
        # fp64 reference (on the clean CPU tensors): `raw` = softmax(q . k) v per list, `full` with the epilogue
        self.ref = ListReference(self.q, self.kk, self.vv, self.crow, self.col, T_src)
        self.raw = self.ref.out
        self.full = self.epilogue(self.raw)
        self.list_len = torch.zeros((N, H, T_dst), dtype=torch.int64)
        self.vmax = torch.zeros((N, H, T_dst), dtype=torch.float64)     # max |V| over the list's keys (tile_bound)
        self.kept = torch.zeros((N, H, T_src), dtype=torch.bool)
        self.crosses64 = 0                                               # lists with keys in more than one 64-key window
        for (n, h, t), keys in self.ref.keys.items():
            assert keys.numel() == 0 or (int(keys.min()) >= 0 and int(keys.max()) < T_src)
            self.list_len[n, h, t] = keys.numel()
            if keys.numel():
                self.kept[n, h, keys] = True
                self.vmax[n, h, t] = self.vv[n, h, keys].double().abs().max()
                self.crosses64 += int(keys.min()) // 64 != int(keys.max()) // 64
                if self.kernel == "tile":                              # a bitmap cannot count: no (row, key) pair twice
                    assert keys.unique().numel() == keys.numel()

    def epilogue(self, raw, rows=None):
        """o * row_scale * mix + (1 - mix) * avg in fp64 ((N, H, T_dst, d), or the rows `rows` = (n, h, t) index tensors)."""
        rs, a, avg = self.rs.double(), self.mix.double(), self.avg.double()
        if rows is not None:
            rs, a, avg = rs[rows], a[rows], avg[rows]
        return raw * (rs * a).unsqueeze(-1) + ((1.0 - a).unsqueeze(-1)) * avg

    # ---- what the kernels read --------------------------------------------------------------------------------------------
    @functools.cached_property
    def dev(self):
        """Device tensors; K / V with every row no kept key names poisoned (K: NaN; V: NaN, for the tile kernel a huge finite
        value), contiguous, or views of a fused projection (strided), or views of one buffer with a wide row pitch."""
        N, H, T_dst, T_src, d, dt = self.N, self.H, self.T_dst, self.T_src, self.d, self.dtype
        poison = (~self.kept).unsqueeze(-1)
        vbad = float("nan") if self.kernel != "tile" else (3.0e38 if dt == BF else 6.0e4)
        kp = torch.where(poison, torch.full((), float("nan"), dtype=dt), self.kk)
        vp = torch.where(poison, torch.full((), vbad, dtype=dt), self.vv)
        c = lambda x: x.to(DEV)
        if self.strided:
            big = torch.zeros((N, T_src, 3, H, d), dtype=dt)
            big[:, T_src - T_dst:, 0] = self.q.permute(0, 2, 1, 3)
            big[:, :, 1], big[:, :, 2] = kp.permute(0, 2, 1, 3), vp.permute(0, 2, 1, 3)
            bd = big.to(DEV)
            q, kd, vd = bd[:, T_src - T_dst:, 0].permute(0, 2, 1, 3), bd[:, :, 1].permute(0, 2, 1, 3), bd[:, :, 2].permute(0, 2, 1, 3)
            assert not kd.is_contiguous() and kd.stride(-1) == 1
        elif self.name == "wave8_bf16_pitch":
            assert 2 * N * H * d <= PITCH and PITCH % 8 == 0
            buf = torch.empty((T_src * PITCH,), dtype=dt, device=DEV)         # ~2.1 GB, of which only the kept rows are written
            kd = buf.as_strided((N, H, T_src, d), (H * d, d, PITCH, 1), 0)
            vd = buf.as_strided((N, H, T_src, d), (H * d, d, PITCH, 1), N * H * d)
            n_, h_, t_ = (x.to(DEV) for x in self.kept.nonzero(as_tuple=True))
            kd[n_, h_, t_] = c(self.kk)[n_, h_, t_]
            vd[n_, h_, t_] = c(self.vv)[n_, h_, t_]
            q = c(self.q)
        else:
            q, kd, vd = c(self.q), c(kp), c(vp)
        csr = ops.topk_to_csr(c(self.probs), c(self.keep), self.k, target_width=T_src, is_causal=self.causal)[0]
        assert not csr.col_is_pending                                       # emitted: the plain launch reads `col`
        return dict(q=q, kk=kd, vv=vd, rs=c(self.rs), mix=c(self.mix), avg=c(self.avg), csr=csr)

    def run(self, form, **kw):
        """One plain launch.  form "f32": fp32 (N, H, T_dst, d) with the full epilogue; "o16": the same in the data type into
        a permuted (N, T_dst, H * d) buffer; "plain": fp32 without row_scale / avg / mix."""
        dv = self.dev
        out, epi = None, dict(row_scale=dv["rs"], avg=dv["avg"], mix=dv["mix"])
        if form == "o16":
            buf = torch.full((self.N, self.T_dst, self.H * self.d), float("nan"), dtype=self.dtype, device=DEV)
            out = buf.view(self.N, self.T_dst, self.H, self.d).permute(0, 2, 1, 3)
        if form == "plain":
            epi = {}
        path = "tile" if self.kernel == "tile" else "gather"
        return ops.sparse_attention(dv["q"], dv["kk"], dv["vv"], dv["csr"], out=out, path=path, **epi, **kw)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return Case(name)


def lanes_per_row(dtype, d):
    need, lanes = -(-d // (4 if dtype == F32 else 8)), 4
    while lanes < need:
        lanes *= 2
    return lanes


def dispatch(c: Case, kd, vd):
    """The kernel `launch_attn_wp` (csrc/sea_attn.hip) gives this launch -- its own tests, on the launch's strides."""
    esz = 4 if c.dtype == F32 else 2
    lanes = lanes_per_row(c.dtype, c.d)
    small = (c.T_src < 1 << 24 and kd.stride(2) * esz < 1 << 24 and vd.stride(2) * esz < 1 << 24
             and c.T_src * kd.stride(2) * esz < 1 << 31 and c.T_src * vd.stride(2) * esz < 1 << 31)
    if esz == 2 and c.d == 80 and small:
        return "rows80"
    return f"rows{lanes}" if lanes <= 16 and small else f"wave{lanes}"


def block_rows(c: Case, row_tiles=1):
    """(query rows per workgroup, per wave) of the case's kernel."""
    if c.kernel == "tile":
        return 2 * 16 * row_tiles, 16 * row_tiles                           # NW = 2 waves of 16 * RT rows
    if c.kernel.startswith("wave"):
        return 4, 1
    lanes = 8 if c.kernel == "rows80" else int(c.kernel[4:])
    return (4 if lanes == 4 else 8) * (64 // lanes), 64 // lanes


# ---- conditions on the inputs alone (no GPU) -----------------------------------------------------------------------------
def check_inputs(c: Case):
    """What each case is there for, from the oracle's CSR."""
    L = c.list_len.view(-1)
    lanes = 8 if c.kernel in ("rows80", "tile") else lanes_per_row(c.dtype, c.d)
    assert c.N * c.H * c.T_dst <= 1300 and c.T_src <= 1100
    assert int((L == 0).sum()) > 0, "an empty list"
    assert int((L > 0).sum()) * 4 >= L.numel(), "a quarter of the lists non-empty"
    assert int(((L % 4 != 0) & (L % lanes != 0)).sum()) > 0, "lengths off the unroll and the lane-group width"
    narrowest = (c.T_src - c.T_dst + 1) if c.causal else c.T_src
    if c.one_entry:
        assert int((L == 1).sum()) > 0, "a list of one entry"
    else:                                                   # every pixel of every row holds two keys or more
        vs, ve = O.pixel_bounds(c.T_dst, c.T_src, c.T_m, c.causal)
        assert narrowest >= 2 * c.T_m and int((ve - vs).min()) >= 2 and c.k >= 2 and int((L == 1).sum()) == 0
    for rt in ((1, 2) if c.kernel == "tile" else (1,)):     # the last workgroup and the last wave are partly empty
        rpb, rpw = block_rows(c, rt)
        assert c.T_dst % rpb != 0 and (rpw == 1 or c.T_dst % rpw != 0), (rpb, rpw)    # (wave per row: the workgroup only)
    if c.name in LONG:
        assert int(L.max()) > 256
    if c.kernel == "tile":
        assert c.T_src > 64 and c.crosses64 > 0
    if c.name == "wave8_bf16_pitch":
        assert c.T_src * PITCH * 2 >= 1 << 31 and PITCH * 2 < 1 << 24


def mutation_shares(c: Case):
    """Two wrong kernels, in fp64 on the CPU: one that loses the last entry of every list of two or more entries, one that
    reads a not-kept neighbour in place of every list's first key.  Returns the share of those lists whose output (with the
    epilogue) moves by more than 10 * TOL32, for each."""
    ref = c.ref
    moved = {"drop": [], "shift": []}
    for (n, h, t), keys in ref.keys.items():
        if keys.numel() == 0:
            continue
        base = c.full[n, h, t]
        kept = set(keys.tolist())
        variants = {}
        if keys.numel() >= 2:
            variants["drop"] = keys[:-1]
        k0 = int(keys[0])
        for j in range(1, c.T_src):
            nb = [x for x in (k0 + j, k0 - j) if 0 <= x < c.T_src and x not in kept]
            if nb:
                sh = keys.clone()
                sh[0] = nb[0]
                variants["shift"] = sh
                break
        for what, ks in variants.items():
            o = c.epilogue(ref.head(n, h, t, ks)[0], rows=(n, h, t))
            moved[what].append(float((o - base).abs().max()) > 10 * TOL32)
    return {what: sum(m) / len(m) for what, m in moved.items()}


def check_mutations(c: Case):
    shares = mutation_shares(c)
    print(f"[attn-ref] {c.name}: lists moved by more than 10 * TOL32 -- last entry dropped {shares['drop']:.3f}, "
          f"first key shifted {shares['shift']:.3f}")
    assert shares["drop"] >= 0.9 and shares["shift"] >= 0.9, (c.name, shares)


def test_case_set_statistics():
    """Across the set: the kernels of the table, N = 2 with H off a multiple of 8, rows of a longer prefix in about half the
    cases, strided inputs on both paths, one non-causal case, lists of more than 256 entries on 8 lanes, 16 lanes and d = 80."""
    cs = list(CASES.values())
    kernels = {(c[0], c[1], c[2]) for c in cs}
    for want in [("rows4", F32, 16), ("rows4", BF, 32), ("rows8", F32, 32), ("rows8", BF, 64), ("rows8", FH, 64),
                 ("rows16", F32, 64), ("rows16", BF, 128), ("rows16", FH, 128), ("rows80", BF, 80), ("rows80", FH, 80),
                 ("wave32", F32, 128), ("wave32", BF, 256), ("wave64", F32, 256), ("wave8", BF, 64)] + \
                [("tile", dt, d) for dt in (BF, FH) for d in (64, 80, 128)]:
        assert want in kernels, want
    assert sum(1 for c in cs if c[3] == 2 and c[4] % 8 != 0) >= 2
    shorter = sum(1 for c in cs if c[5] < c[6])
    assert len(cs) // 2 - 2 <= shorter <= len(cs) // 2 + 2, shorter
    assert any(c[10] and c[0] != "tile" for c in cs) and any(c[10] and c[0] == "tile" for c in cs)
    assert sum(1 for c in cs if not c[9]) == 1
    assert {CASES[n][0] for n in LONG} == {"rows8", "rows16", "rows80"}


# ---- the bars --------------------------------------------------------------------------------------------------------------
def tile_bound(c: Case, with_epilogue=True):
    """Per-list bar of the tile kernel's fp32 output, (N, H, T_dst, 1).

    sparse_attn_tile_kernel computes p_i = exp2(s_i * log2e - m * log2e) in fp32 and forms the softmax sum l from those fp32
    values (`l[rt] += ((pv[0] + pv[1]) + ...`), like the gather kernels; only the numerator sees a rounded P: the matrix
    cores get P~_i = hi + lo with hi = bf16(p_i), lo = bf16(p_i - hi) (bf16 data: |P~_i - p_i| <= 2^-8 * 2^-8 p_i, i.e.
    u = 2^-16, 16 significand bits) or the single term fp16(p_i) (fp16 data: u = 2^-11 while p_i >= 2^-14; below that fp16
    is subnormal and the error is at most 2^-25 absolute).  The products P~_i * v_i are exact in the fp32 accumulator, so
        |sum_i P~_i v_i / l  -  sum_i p_i v_i / l|  <=  sum_i (u p_i + 2^-25 [fp16]) |v_i| / l
                                                    <=  (u + L * 2^-25 [fp16]) * max_i |v_i|
    (sum_i p_i = l; l >= 1 because the list's largest score has p = 1).  c = 1: the denominator is not rounded.  The row
    scale and the mix weight multiply the error like the value; everything else in the kernel is fp32 arithmetic of the
    gather kernels' kind (TOL32)."""
    u = 2.0 ** -16 if c.dtype == BF else 2.0 ** -11
    sub = 0.0 if c.dtype == BF else 2.0 ** -25
    b = (u + c.list_len.double() * sub) * c.vmax
    if with_epilogue:
        b = b * c.rs.double() * c.mix.double()
    return (TOL32 + b).unsqueeze(-1)


def check_form(c: Case, what, o, ref, bound):
    """fp32: |o - ref| <= bound; 16-bit: within 1 ulp of the fp64 value rounded to the type, plus the bound."""
    assert torch.isfinite(o.float()).all(), (c.name, what)
    if o.dtype == torch.float32:
        d = (o.double().cpu() - ref).abs()
        lim = bound if torch.is_tensor(bound) else torch.full_like(d, bound)
        lim = lim.expand_as(d)
    else:
        r16 = ref.to(o.dtype)
        d = (o.cpu().double() - r16.double()).abs()
        lim = ulp(r16) + bound
    i = int((d / lim).argmax())                                             # the element nearest to (or furthest past) its bar
    print(f"[attn-ref] {c.name} ({c.kernel}) {what}: max|err| = {d.max().item():.3e}  max|ref| = {ref.abs().max().item():.3e}  "
          f"nearest its bar: err {d.reshape(-1)[i].item():.3e} / bar {lim.reshape(-1)[i].item():.3e}")
    assert bool((d <= lim).all()), (c.name, what, d.max().item(), (d / lim).max().item())


def check_selection(c: Case):
    """The device CSR is the oracle's, bit for bit: the kept-pixel words, `crow`, and `col` up to each item's end."""
    csr = c.dev["csr"]
    assert torch.equal(unpack_bits(csr.bits, c.H, c.T_m), c.mask), "selection bits != oracle mask"
    assert torch.equal(csr.crow.cpu().long(), c.crow)
    col = csr.col.cpu().long()
    for n in range(c.N):
        z = int(c.crow[n, -1])
        assert torch.equal(col[n, :z], c.col[n, :z]), n
    if c.causal:
        crow_o, col_o = oracle_columns(c.mask, c.k, c.T_src, c.T_src)       # (the decode file's helper agrees)
        assert torch.equal(crow_o, c.crow) and torch.equal(col_o, c.col)


# ---- the tests -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_plain_launch_matches_fp64(name):
    c = case(name)
    check_inputs(c)
    check_mutations(c)
    check_selection(c)
    dv = c.dev
    if c.kernel == "tile":
        forms = [dict(row_tiles=rt, key_window=kw) for rt, kw in TILE_FORMS]
        full_bar, plain_bar = tile_bound(c), tile_bound(c, with_epilogue=False)
        # TOL32 + 2^-16 * 5 = 7.9e-5 for bf16: far below the 2e-3 of test_gpu_tile_attention.py; fp16's single 11-bit term
        # gives 2^-11 * 5 = 2.4e-3 at |V| = 5 -- that bar was already the arithmetic's
        print(f"[attn-ref] {name}: derived tile bound, largest over the lists = {full_bar.max().item():.3e}")
    else:
        assert dispatch(c, dv["kk"], dv["vv"]) == c.kernel                  # the kernel this case is there for
        forms = [dict()]
        full_bar = plain_bar = TOL32
    for kw in forms:
        tag = f"rt={kw['row_tiles']} kw={kw['key_window']} " if kw else ""
        o32 = c.run("f32", **kw)
        assert o32.dtype == torch.float32
        check_form(c, tag + "fp32", o32, c.full, full_bar)
        check_form(c, tag + "plain", c.run("plain", **kw), c.raw, plain_bar)
        if c.dtype != F32:
            o16 = c.run("o16", **kw)
            assert o16.dtype == c.dtype and o16.stride(2) == c.H * c.d      # the layer's (N, T, H * d) layout
            check_form(c, tag + "16-bit", o16, c.full, full_bar)
        assert torch.equal(c.run("f32", **kw), o32), (name, kw, "a second launch differs")
        if kw:                                                              # (another order of the tile pairs: other roundings)
            first = o32 if kw is forms[0] else first
            print(f"[attn-ref] {name} {tag}: {int((o32 != first).sum())} of {o32.numel()} elements differ from the default form's")
    empty = (c.list_len == 0)
    want = ((1.0 - c.mix).unsqueeze(-1) * c.avg.float())[empty]             # an empty list: o = 0 before the mix
    assert torch.allclose(o32.cpu()[empty], want, rtol=0, atol=1e-6)


@pytest.mark.parametrize("name", PROBS_CASES)
def test_probabilities_match_fp64(name):
    """want_probs: the per-entry values rs * softmax at the slots `col` has, against fp64; the context that comes with them
    is the context without them, bit for bit.  One case per lane width of the gather kernels and of sparse_attn_kernel."""
    c = case(name)
    dv = c.dev
    assert dispatch(c, dv["kk"], dv["vv"]) == c.kernel
    epi = dict(row_scale=dv["rs"], avg=dv["avg"], mix=dv["mix"])
    o, pv = ops.sparse_attention(dv["q"], dv["kk"], dv["vv"], dv["csr"], path="gather", want_probs=True, **epi)
    assert torch.equal(o, c.run("f32"))
    pv = pv.cpu().double()
    assert torch.isfinite(pv).all()
    worst = 0.0
    for n in range(c.N):
        for t in range(c.T_dst):
            b, e = int(c.crow[n, t]), int(c.crow[n, t + 1])
            heads = torch.div(c.col[n, b:e], c.T_src, rounding_mode="floor")
            want = torch.zeros(e - b, dtype=torch.float64)
            for h in range(c.H):
                if c.ref.p[n, h, t] is not None:
                    want[heads == h] = c.ref.p[n, h, t] * float(c.rs[n, h, t])
            if e > b:
                worst = max(worst, float((pv[n, b:e] - want).abs().max()))
        assert float(pv[n, int(c.crow[n, -1]):].abs().max() if pv.shape[1] > int(c.crow[n, -1]) else 0.0) == 0.0
    print(f"[attn-ref] {name} ({c.kernel}) probabilities: max|err| = {worst:.3e}")
    assert worst <= TOL_P, (name, worst)
