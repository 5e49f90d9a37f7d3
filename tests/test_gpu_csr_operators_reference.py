"""-m gpu: the reference's UNFUSED operator API -- `flat_csr_masked_bmm`, `flat_csr_softmax`, `flat_csr_elmul`,
`flat_csr_sdbmm` = `sea_csr_sddmm`, `sea_csr_softmax`, `sea_csr_elmul`, `sea_csr_spmm` -- each on its own against fp64, in the
forms nothing else in the suite runs: the `__half` and `__hip_bfloat16` instantiations (d = 64, 80, 128), the 32- and 64-lane
forms of sddmm and spmm (fp32 d = 128, 256), T_dst < T_src, N = 2, H = 9, non-contiguous q / k / v, the stride-0 expanded
`dense` of elmul in three types, and every `idx_bytes == 4` instantiation -- through the C ABI with ctypes on the library's
own int32 `FlatCSR`, which is what a raw-ABI caller would pass.

The CSR is the oracle's (cases of the shape of tests/test_gpu_attention_reference.py, whose `Case` builds them).  Every
operator is fed the fp64 reference's PREVIOUS stage rounded to fp32, so one operator's error does not hide in the next.
The K rows (sddmm) and V rows (spmm) no kept key names hold NaN: an operator that touches a key outside its list shows it.
That found two bugs.  csr_spmm_kernel's lane groups past a list's end loaded V row 0 of the head and accumulated 0 * V[0] --
NaN in the output of every list whose length is no multiple of the keys per wave instruction when that row is not finite
(`test_spmm_reads_kept_keys_only`).  csr_softmax_kernel summed a head's exponentials with float atomics from all four
waves, so a head spread over three or more wave-chunks gave other bits from launch to launch (the int32 launch differed
from the int64 one in `test_softmax_matches_fp64[bf16_d80]`); every wave now sums into its own slot, added in a fixed order.

Bars: four times the largest max |err| observed on MI355X over the cases of this file, the observed value next to each;
printed per case ("[csr-ref] ...").  The int32 results must be `torch.equal` to the int64 results (the index width changes
no arithmetic), and value slots past each item's crow[-1] keep what they held.
"""
import functools
from ctypes import c_void_p

import pytest
import torch

from sea_attention_amd import _lib
from sea_attention_amd.perlin_attention import ops
from test_gpu_attention_reference import BF, FH, F32, DEV, Case

pytestmark = pytest.mark.gpu

# observed on MI355X, largest over the cases: sddmm 4.2e-7 (|scores| up to 4.3), spmm 2.7e-7 (|out| up to 3.5), softmax 8.2e-8,
# elmul 3.0e-8 (values in [0, 1]; the golden tests hold the last two at 1e-6 and 1e-7 at fp32).  Each bar: four times that.
TOL_SDDMM = 1.7e-6
TOL_SPMM = 1.1e-6
TOL_SOFTMAX = 3.3e-7
TOL_ELMUL = 1.2e-7
PAD = 7.25                                              # what the value slots past an item's end hold before every operator

# name: ("ops", dtype, d, N, H, T_dst, T_src, T_m, max_k, causal, strided, one_entry) -- the layout of the attention file's CASES
CASES = {
    "bf16_d64":  ("ops", BF, 64, 2, 9, 60, 100, 32, 4, True, True, True),          # N = 2, H = 9, strided, T_dst < T_src
    "fp16_d64":  ("ops", FH, 64, 1, 3, 75, 75, 32, 8, True, False, True),
    "bf16_d80":  ("ops", BF, 80, 1, 5, 53, 300, 32, 16, True, False, False),       # rows of > 256 entries
    "fp16_d80":  ("ops", FH, 80, 2, 3, 45, 90, 64, 4, True, True, True),
    "bf16_d128": ("ops", BF, 128, 2, 3, 45, 45, 32, 4, True, False, True),
    "fp16_d128": ("ops", FH, 128, 1, 4, 50, 90, 64, 4, False, False, True),
    "f32_d128":  ("ops", F32, 128, 2, 3, 41, 77, 64, 4, True, True, True),         # 32 lanes
    "f32_d256":  ("ops", F32, 256, 1, 2, 37, 100, 64, 8, True, False, True),       # 64 lanes
}


def _p(t):
    return c_void_p(t.data_ptr())


class OpCase(Case):
    """A `Case` with the fp64 stages of the unfused chain laid out like the wire format: (N, Z) per-entry values."""

    def __init__(self, name):
        super().__init__("ops_" + name, CASES[name])
        N, H, T_src = self.N, self.H, self.T_src
        self.Z = self.col.shape[1]
        self.rows, self.heads, self.keys, self.z = [], [], [], []
        for n in range(N):
            z = int(self.crow[n, -1])
            self.z.append(z)
            self.rows.append(torch.repeat_interleave(torch.arange(self.T_dst), self.crow[n, 1:] - self.crow[n, :-1]))
            self.heads.append(torch.div(self.col[n, :z], T_src, rounding_mode="floor"))
            self.keys.append(self.col[n, :z] - self.heads[n] * T_src)
        self.valid = torch.arange(self.Z).view(1, -1) < torch.tensor(self.z).view(-1, 1)
        # stage 1, fp64: q . k per entry (padding: PAD)
        self.s64 = torch.full((N, self.Z), PAD, dtype=torch.float64)
        for n in range(N):
            qe = self.q[n, self.heads[n], self.rows[n]].double()
            ke = self.kk[n, self.heads[n], self.keys[n]].double()
            self.s64[n, :self.z[n]] = (qe * ke).sum(-1)

    def softmax64(self, s32):
        """fp64 softmax over every (row, head) segment of fp32 scores (N, Z)."""
        out = s32.double().clone()
        for n in range(self.N):
            z, seg = self.z[n], self.rows[n] * self.H + self.heads[n]
            v = s32[n, :z].double()
            mx = torch.full((self.T_dst * self.H,), -float("inf"), dtype=torch.float64)
            mx.scatter_reduce_(0, seg, v, reduce="amax")
            e = torch.exp(v - mx[seg])
            den = torch.zeros(self.T_dst * self.H, dtype=torch.float64).index_add_(0, seg, e)
            out[n, :z] = e / den[seg]
        return out

    def elmul64(self, p32, dense):
        out = p32.double().clone()
        for n in range(self.N):
            out[n, :self.z[n]] *= dense[n, self.heads[n], self.rows[n], self.keys[n]].double()
        return out

    def spmm64(self, e32):
        out = torch.zeros((self.N, self.H, self.T_dst, self.d), dtype=torch.float64)
        for n in range(self.N):
            contrib = e32[n, :self.z[n]].double().unsqueeze(-1) * self.vv[n, self.heads[n], self.keys[n]].double()
            out[n].view(self.H * self.T_dst, self.d).index_add_(0, self.heads[n] * self.T_dst + self.rows[n], contrib)
        return out

    # ---- the two index widths ------------------------------------------------------------------------------------------------
    def wire(self, values):
        """The reference's wire format: int64 indices trimmed to Z, padded columns 0, `values` (N, Z) fp32 on the CPU."""
        col = self.col * self.valid
        return torch.sparse_csr_tensor(self.crow.to(DEV), col.to(DEV), values.to(DEV), size=(self.N, self.T_dst, self.H * self.T_src))

    def abi_values(self, values):
        """`values` (N, Z) laid into the library's own (N, z_cap) layout (the stride of FlatCSR.col), slots past Z: PAD."""
        csr = self.dev["csr"]
        out = torch.full(csr.col.shape, PAD, dtype=torch.float32, device=DEV)
        out[:, :self.Z] = values.to(DEV)
        return out

    def same_as_wire(self, got32, got64, what):
        """The int32 launch's values against the int64 launch's: the same bits where an entry lives, PAD everywhere else."""
        g32 = got32.cpu()
        assert torch.equal(g32[:, :self.Z][self.valid], got64.cpu()[self.valid]), (self.name, what, "int32 != int64")
        assert bool((g32[:, :self.Z][~self.valid] == PAD).all()) and bool((g32[:, self.Z:] == PAD).all()), (self.name, what, "padding")


@functools.lru_cache(maxsize=None)
def case(name) -> OpCase:
    return OpCase(name)


def report(c, what, got, ref, tol, valid=None):
    d = (got.double().cpu() - ref).abs()
    if valid is not None:
        d, ref = d[valid], ref[valid]
    print(f"[csr-ref] {c.name} {what}: max|err| = {d.max().item():.3e}  max|ref| = {ref.abs().max().item():.3e}")
    assert bool(torch.isfinite(got).all()) and d.max().item() <= tol, (c.name, what, d.max().item())


def test_case_set_statistics():
    cs = list(CASES.values())
    assert {(c[1], c[2]) for c in cs} == {(dt, d) for dt in (BF, FH) for d in (64, 80, 128)} | {(F32, 128), (F32, 256)}
    assert any(c[3] == 2 for c in cs) and any(c[4] == 9 for c in cs) and any(c[5] < c[6] for c in cs) and any(c[10] for c in cs)


@pytest.mark.parametrize("name", list(CASES))
def test_sddmm_matches_fp64(name):
    c = case(name)
    dv, lib = c.dev, _lib.load()
    q, kk, csr = dv["q"], dv["kk"], dv["csr"]
    assert c.strided == (not kk.is_contiguous()) and kk.stride(-1) == 1
    if c.N == 2:
        assert c.z[0] != c.z[1]                                             # the shorter item has padded slots
    mask = c.wire(torch.where(c.valid, 1.0, PAD).float())
    out = ops.flat_csr_masked_bmm(q, kk, mask)
    got64 = out.values()
    assert torch.equal(out.crow_indices().cpu(), c.crow) and bool((got64.cpu()[~c.valid] == PAD).all())
    report(c, "sddmm", got64, c.s64, TOL_SDDMM, c.valid)
    got32 = c.abi_values(torch.full((c.N, c.Z), PAD))
    assert csr.crow.dtype == csr.col.dtype == torch.int32
    _lib.check(lib.sea_csr_sddmm(_p(q), _p(kk), _lib.dtype_code(c.dtype), c.N, c.H, c.T_dst, c.T_src, c.d, _lib.strides3(q),
                                 _lib.strides3(kk), _p(csr.crow), _p(csr.col), 4, csr.col.stride(0), _p(got32),
                                 _lib.stream_ptr()), "sea_csr_sddmm")
    c.same_as_wire(got32, got64, "sddmm")


def softmax_edges(c: OpCase, s32):
    """The fp64 scores rounded to fp32 with four lists rewritten: all scores equal; scores around +-80; a -inf among finite
    ones; and (asserted from the CSR) the shapes the kernel's loops branch on.  Returns the slots of the -inf entries."""
    s = s32.clone()
    lists = [(n, h, t) for (n, h, t), keys in c.ref.keys.items() if keys.numel() >= 3][:3]
    assert len(lists) == 3
    ninf = []
    for i, (n, h, t) in enumerate(lists):
        sel = ((c.rows[n] == t) & (c.heads[n] == h)).nonzero().view(-1)
        if i == 0:
            s[n, sel] = 0.375
        elif i == 1:
            s[n, sel] = torch.tensor([80.0, -80.0, 79.5] * sel.numel())[:sel.numel()]
        else:
            s[n, sel[1]] = -float("inf")
            ninf.append((n, int(sel[1])))
    return s, ninf


@pytest.mark.parametrize("name", list(CASES))
def test_softmax_matches_fp64(name):
    c = case(name)
    dv, lib = c.dev, _lib.load()
    csr = dv["csr"]
    s32, ninf = softmax_edges(c, c.s64.float())
    row_len = c.crow[:, 1:] - c.crow[:, :-1]
    if name == "bf16_d80":                                                  # several passes of the 256-thread loop, and a head in
        pos = torch.arange(c.z[0]) - c.crow[0][c.rows[0]]                   # three or more 64-entry wave chunks (the sum's order)
        seg = c.rows[0] * c.H + c.heads[0]
        lo = torch.full((c.T_dst * c.H,), 1 << 30).scatter_reduce_(0, seg, pos // 64, reduce="amin")
        hi = torch.full((c.T_dst * c.H,), -1).scatter_reduce_(0, seg, pos // 64, reduce="amax")
        assert int(row_len.max()) > 256 and int((hi - lo).max()) >= 2
    if name == "bf16_d64":                                                  # a wave's 64 entries from more than three heads
        n, t = 0, int(row_len[0].argmax())
        b = int(c.crow[n, t])
        assert any(c.heads[n][b + w:b + w + 64].unique().numel() > 3 for w in range(0, int(row_len[n, t]), 64))
    ref = c.softmax64(s32)
    out = ops.flat_csr_softmax(c.wire(s32), c.H, c.T_src)
    got64 = out.values()
    assert bool((got64.cpu()[~c.valid] == PAD).all())
    report(c, "softmax", got64, ref, TOL_SOFTMAX, c.valid)
    assert torch.equal(ops.flat_csr_softmax(c.wire(s32), c.H, c.T_src).values(), got64), "a second launch differs"
    for n, e in ninf:
        assert float(got64[n, e]) == 0.0 and float(ref[n, e]) == 0.0        # a -inf score: probability exactly 0
    src, got32 = c.abi_values(s32), c.abi_values(torch.full((c.N, c.Z), PAD))
    _lib.check(lib.sea_csr_softmax(_p(src), _p(got32), c.N, c.H, c.T_dst, c.T_src, _p(csr.crow), _p(csr.col), 4,
                                   csr.col.stride(0), _lib.stream_ptr()), "sea_csr_softmax")
    c.same_as_wire(got32, got64, "softmax")


@pytest.mark.parametrize("dense_dtype", [F32, FH, BF], ids=["dense_f32", "dense_fp16", "dense_bf16"])
@pytest.mark.parametrize("name", list(CASES))
def test_elmul_matches_fp64(name, dense_dtype):
    c = case(name)
    dv, lib = c.dev, _lib.load()
    csr = dv["csr"]
    p32 = c.softmax64(c.s64.float()).float()
    p32[~c.valid] = PAD
    dense_cpu = c.rs.to(dense_dtype).view(c.N, c.H, c.T_dst, 1).expand(c.N, c.H, c.T_dst, c.T_src)
    dense = c.rs.to(dense_dtype).to(DEV).view(c.N, c.H, c.T_dst, 1).expand(c.N, c.H, c.T_dst, c.T_src)
    assert dense.stride(-1) == 0                                            # the view the module passes (attention.py:1170-1171)
    ref = c.elmul64(p32, dense_cpu)
    out = ops.flat_csr_elmul(c.wire(p32), dense)
    got64 = out.values()
    assert bool((got64.cpu()[~c.valid] == PAD).all())
    report(c, f"elmul({dense_dtype})", got64, ref, TOL_ELMUL, c.valid)
    src, got32 = c.abi_values(p32), c.abi_values(torch.full((c.N, c.Z), PAD))
    _lib.check(lib.sea_csr_elmul(_p(src), _p(got32), _p(dense), _lib.dtype_code(dense_dtype), _lib.strides4(dense), c.N, c.H,
                                 c.T_dst, c.T_src, _p(csr.crow), _p(csr.col), 4, csr.col.stride(0), _lib.stream_ptr()),
               "sea_csr_elmul")
    c.same_as_wire(got32, got64, "elmul")


@pytest.mark.parametrize("name", list(CASES))
def test_spmm_matches_fp64(name):
    c = case(name)
    dv, lib = c.dev, _lib.load()
    vv, csr = dv["vv"], dv["csr"]
    e32 = c.elmul64(c.softmax64(c.s64.float()).float(), c.rs.view(c.N, c.H, c.T_dst, 1).expand(-1, -1, -1, c.T_src)).float()
    e32[~c.valid] = PAD
    ref = c.spmm64(e32)
    got64 = ops.flat_csr_sdbmm(c.wire(e32), vv, c.T_m)
    assert got64.dtype == torch.float32 and got64.shape == (c.N, c.H, c.T_dst, c.d)
    report(c, "spmm", got64, ref, TOL_SPMM)
    assert bool((got64.cpu()[c.list_len == 0] == 0).all())                  # an empty list: zeros
    got32 = torch.full((c.N, c.H, c.T_dst, c.d), float("nan"), dtype=torch.float32, device=DEV)
    _lib.check(lib.sea_csr_spmm(_p(c.abi_values(e32)), _p(vv), _lib.dtype_code(c.dtype), c.N, c.H, c.T_dst, c.T_src, c.d,
                                _lib.strides3(vv), _p(csr.crow), _p(csr.col), 4, csr.col.stride(0), _p(csr.head_off), _p(got32),
                                _lib.stream_ptr()), "sea_csr_spmm")
    assert torch.equal(got32, got64), (name, "int32 != int64")


def test_spmm_reads_kept_keys_only():
    """Regression: a wave of csr_spmm_kernel takes 64 / lanes keys per instruction, and the lane groups past a list's end
    used to load key 0 of the head and accumulate 0 * V[0] -- NaN out of a V row that nobody keeps (an unwritten cache row).
    Here a head whose key 0 nobody keeps (NaN in what the kernel reads) has lists whose lengths are no multiple of the
    group count."""
    c = case("bf16_d80")
    per_instr = 64 // 16                                                    # d = 80, 16-bit: 16 lanes per key, 4 keys per instruction
    ragged = (c.list_len > 0) & (c.list_len % per_instr != 0)
    heads = [(n, h) for n in range(c.N) for h in range(c.H) if not c.kept[n, h, 0] and bool(ragged[n, h].any())]
    assert heads
    vv = c.dev["vv"]
    assert all(bool(torch.isnan(vv[n, h, 0].float()).all()) for n, h in heads)
    e32 = c.softmax64(c.s64.float()).float()
    e32[~c.valid] = PAD
    got = ops.flat_csr_sdbmm(c.wire(e32), vv, c.T_m)
    assert bool(torch.isfinite(got).all())
