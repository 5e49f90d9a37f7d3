"""The backward of the sparse attention (csrc/sea_attn_bwd.hip: the atomic form and the gather form -- CSC count, two-launch
scan, row pass, column pass) held to an INDEPENDENT fp64 reference, per element.  tests/test_gpu_backward.py compares by
global relative norm after the cast to the input type; one wrong dK row, one lost record, a lost scan carry pass there.

Reference (`BwdReference`, CPU, fp64, per (n, h, t) list with keys j -- `Case` / `ListReference` of
tests/test_gpu_attention_reference.py give the oracle's CSR, the keys and the softmax p; a (row, key) pair that a list holds
twice counts twice, as in the kernels):
    dp_j = dO . v_j      delta = sum_j p_j dp_j      ds_j = p_j (dp_j - delta)
    dQ_t = sum_j ds_j k_j      dK_key += ds_j q_t      dV_key += p_j dO_t
`test_closed_forms_match_autograd` (no GPU) holds these forms to torch.autograd in fp64 through
softmax(q . k[keys]) @ v[keys] per list, so they do not rest on the header comment of the file under test.

Tier A: `sea_sparse_attention_bwd` through the C ABI, its `form` pinned to the gather and to the atomic form (and left to the
library on one case per side of its lane rule).  The test supplies `probs` and
`out` itself: the reference's p and o rounded to fp32 on the device CSR's slots (the device `col` is the oracle's, asserted;
slots past an item's end hold NaN).  What is measured is then the backward's own rounding, and the bar is DERIVED
(`BwdReference`; u = 2^-24, D the head size, L the list's length, R the key's record count; a sum of n products formed in
any order of fmas and additions is off by at most n u sum |terms|, which covers the lane fragments' fma chains, the
lane-group sum, the row's and the key's chains and any order of the atomics):
    e_p_j   = u p_j                                                    p stored as fp32
    e_delta = D u sum_i |dO_i o_i|  +  u sum_i |dO_i o_i|              the D-term chain; o stored as fp32
    e_dp_j  = D u sum_i |dO_i v_ji|                                    the D-term chain (v is exact)
    e_ds_j  = (p_j + e_p_j) (e_dp_j + e_delta) + (e_p_j + 2 u p_j) |dp_j - delta|       a subtraction and a product
    bar dQ  = L u sum_j |ds_j k_j|  +  sum_j e_ds_j |k_j|  +  u |dQ|
    bar dK  = R u sum_r |ds_r q_r|  +  sum_r e_ds_r |q_r|  +  u |dK|
    bar dV  = R u sum_r p_r |dO_r|  +  sum_r e_p_r |dO_r|  +  u |dV|
each times 1 + 1e-3 for the terms of second order.  Nothing in them is measured.  Exact, asserted outright: dQ of a row that
keeps nothing is 0, dK / dV of a key without a record are 0, everything is finite although every K / V row no kept key
names is NaN; both forms get NaN-filled dq / dk / dv, the gather form a workspace of 0xFF bytes, the atomic form NULL.  In the
strided cases K / V are views of a fused projection and q has a wider row pitch of its own with NaN around its rows (`run_abi`).

Tier B: `ops.sparse_attention_autograd` on the same poisoned inputs, both `backward_form`s: gradients in the input type
within 1 ulp of the reference rounded to that type, plus the Tier A bar with the forward's error carried through the same
formulas (e_p_j += TOL_P, o off by TOL32 per element: e_delta += TOL32 sum |dO| -- the forward file's measured bars).

The comparison can fail (`witness_shares`, CPU, fp64): a row pass that loses a row's last entry moves that row's dQ, and a
column pass that loses one record of a key moves that key's dK and dV, by more than 10 bars, for at least 90 % of the rows /
keys whose lost entry has p >= 1e-3.

Printed per case, form and gradient ("[bwd-ref] ..."): max |err| / bar; MI355X values are in DESIGN.md 5.4k.
"""
import functools
import zlib

import pytest
import torch

from sea_attention_amd.perlin_attention import ops
from sea_attention_amd.perlin_attention.ops import flat_csr
from test_gpu_attention_reference import BF, F32, FH, TOL32, TOL_P, Case, check_selection, lanes_per_row
from test_gpu_decode_reference import ulp

gpu = pytest.mark.gpu
_lib = flat_csr._lib
DEV = "cuda:0"
U = 2.0 ** -24

# name: (form, dtype, d, N, H, T_dst, T_src, T_m, max_k, causal, strided, one_entry) -- `Case`'s spec; form "gather": both
# forms run the case, "atomic": the atomic form only (rows wider than 16 lanes).  Every query row's pixels
# are two keys wide or more (causal: T_src - T_dst + 1 >= 2 T_m) and max_k >= 2, so no list has one entry: there p = 1 and
# ds = dp - delta = 0 identically, and a lost entry cannot show in dQ or dK (asserted in check_case)
SPECS = {
    "g4_bf16_d32":   ("gather", BF, 32, 2, 3, 70, 140, 32, 4, True, True, False),         # strided, (h + n) % H with H = 3
    "g4_fp16_d32":   ("gather", FH, 32, 1, 4, 128, 600, 256, 4, False, False, False),    # T_dst % 64 == 0, T_src % 64 != 0; key 0
    "g8_bf16_d64":   ("gather", BF, 64, 2, 5, 60, 128, 32, 4, True, True, False),        # T_src % 64 == 0, T_dst % 64 != 0; strided
    "g8_fp16_d64":   ("gather", FH, 64, 1, 3, 75, 150, 32, 8, True, False, False),
    "g8_fp16_d40":   ("gather", FH, 40, 1, 3, 64, 600, 256, 4, False, False, False),     # 5 of 8 lanes active; key 0
    "g16_fp16_d128": ("gather", FH, 128, 1, 3, 64, 600, 256, 4, False, True, False),     # strided; key 0
    "g16_bf16_d80":  ("gather", BF, 80, 2, 3, 45, 120, 32, 8, True, False, False),       # 10 of 16 lanes active
    "g4_f32_d16":    ("gather", F32, 16, 1, 4, 100, 170, 32, 4, True, False, False),
    "g8_f32_d32":    ("gather", F32, 32, 2, 3, 50, 120, 32, 8, True, False, False),
    "g16_f32_d64":   ("gather", F32, 64, 1, 2, 45, 110, 32, 4, True, False, False),
    "g16_f32_d48":   ("gather", F32, 48, 1, 3, 40, 105, 32, 4, True, False, False),      # 12 of 16 lanes active
    # C = H * T_src = 33000 > 32768 and off a multiple of 1024: the scan walks two 1024-wide passes per chunk
    "scan_bf16_d32": ("gather", BF, 32, 1, 3, 48, 11000, 32, 16, True, False, False),
    "a32_f32_d128":  ("atomic", F32, 128, 1, 2, 37, 100, 32, 4, True, False, False),
    "a32_bf16_d256": ("atomic", BF, 256, 2, 2, 30, 95, 32, 4, True, False, False),
    "a64_f32_d256":  ("atomic", F32, 256, 1, 2, 33, 100, 32, 8, True, False, False),
}
GATHER = [n for n, s in SPECS.items() if s[0] == "gather"]
# the atomic form: 4 / 8 / 16 lanes on shapes of the gather form (one dtype each), then 32 and 64 lanes
ATOMIC = ["g4_bf16_d32", "g8_fp16_d40", "g16_f32_d48", "a32_f32_d128", "a32_bf16_d256", "a64_f32_d256"]
# through autograd: one case per lane count and 16-bit type
AUTOGRAD = ["g4_bf16_d32", "g4_fp16_d32", "g8_bf16_d64", "g8_fp16_d64", "g16_fp16_d128", "g16_bf16_d80"]
KEY0 = {"g4_fp16_d32": 4, "g8_fp16_d40": 8, "g16_fp16_d128": 16}          # an empty row beside a NaN key 0, per lane count
SCAN = "scan_bf16_d32"


def gather_block(dtype, d):
    """(lanes per row, rows -- and keys -- per workgroup, per wave) of launch_bwd_gather's row and column passes."""
    lanes = lanes_per_row(dtype, d)
    nwb = 4 if lanes == 4 else 8
    return lanes, nwb * (64 // lanes), 64 // lanes


class BwdReference:
    """fp64 gradients of one case for a seeded upstream dO, the derived bars (`bar`: Tier A; `bar_b`: with the forward's
    TOL_P / TOL32 carried, Tier B), the record count of every key, and what the two wrong kernels of the witnesses lose."""

    def __init__(self, c: Case):
        N, H, T_dst, T_src, D = c.N, c.H, c.T_dst, c.T_src, c.d
        g = torch.Generator().manual_seed(zlib.crc32(c.name.encode()) + 1)
        self.dout = torch.randn((N, H, T_dst, D), generator=g)              # fp32: what the kernels read
        dO, q, kk, vv = self.dout.double(), c.q.double(), c.kk.double(), c.vv.double()
        z = lambda *s: torch.zeros(s, dtype=torch.float64)
        self.dq, self.dk, self.dv = z(N, H, T_dst, D), z(N, H, T_src, D), z(N, H, T_src, D)
        self.records = torch.zeros((N, H, T_src), dtype=torch.int64)
        sets = {"bar": (0.0, 0.0), "bar_b": (TOL_P, TOL32)}                  # (added to e_p_j, added to |o - o32|)
        bq = {s: z(N, H, T_dst, D) for s in sets}
        ek = {s: z(N, H, T_src, D) for s in sets}
        ev = {s: z(N, H, T_src, D) for s in sets}
        ak, av = z(N, H, T_src, D), z(N, H, T_src, D)                        # sum |ds_r q_r|, sum p_r |dO_r|
        # the witnesses: the row's last entry; per key the record of the last row that names it
        self.last_dq = z(N, H, T_dst, D)
        self.last_p_row = z(N, H, T_dst)
        self.last_dk, self.last_dv, self.last_p_key = z(N, H, T_src, D), z(N, H, T_src, D), z(N, H, T_src)
        for (n, h, t), keys in c.ref.keys.items():
            L = keys.numel()
            if L == 0:
                continue
            p, k_, v_, qt, go, o = c.ref.p[n, h, t], kk[n, h][keys], vv[n, h][keys], q[n, h, t], dO[n, h, t], c.raw[n, h, t]
            dp = v_ @ go
            delta = p @ dp
            ds = p * (dp - delta)
            self.dq[n, h, t] = ds @ k_
            dkr, dvr = ds[:, None] * qt[None], p[:, None] * go[None]
            self.dk[n, h].index_add_(0, keys, dkr)
            self.dv[n, h].index_add_(0, keys, dvr)
            ak[n, h].index_add_(0, keys, dkr.abs())
            av[n, h].index_add_(0, keys, dvr.abs())
            self.records[n, h].index_add_(0, keys, torch.ones_like(keys))
            self.last_dq[n, h, t], self.last_p_row[n, h, t] = ds[-1] * k_[-1], p[-1]
            self.last_dk[n, h][keys], self.last_dv[n, h][keys], self.last_p_key[n, h][keys] = dkr, dvr, p
            for s, (tol_p, tol_o) in sets.items():
                e_p = U * p + tol_p
                e_delta = D * U * (go.abs() @ o.abs()) + go.abs() @ (U * o.abs() + tol_o)
                e_dp = D * U * (v_.abs() @ go.abs())
                e_ds = (p + e_p) * (e_dp + e_delta) + (e_p + 2 * U * p) * (dp - delta).abs()
                bq[s][n, h, t] = L * U * (ds.abs() @ k_.abs()) + e_ds @ k_.abs()
                ek[s][n, h].index_add_(0, keys, e_ds[:, None] * qt.abs()[None])
                ev[s][n, h].index_add_(0, keys, e_p[:, None] * go.abs()[None])
        R = self.records.double().unsqueeze(-1)
        for s in sets:
            setattr(self, s, {"dq": (bq[s] + U * self.dq.abs()) * (1 + 1e-3),
                              "dk": (R * U * ak + ek[s] + U * self.dk.abs()) * (1 + 1e-3),
                              "dv": (R * U * av + ev[s] + U * self.dv.abs()) * (1 + 1e-3)})
        self.grads = {"dq": self.dq, "dk": self.dk, "dv": self.dv}
        self.empty_rows = c.list_len == 0
        self.no_record = self.records == 0
        assert torch.equal(~self.no_record, c.kept)


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return Case(name, spec=SPECS[name])


@functools.lru_cache(maxsize=None)
def reference(name) -> BwdReference:
    return BwdReference(case(name))


# ---- conditions on the inputs and on the reference alone (no GPU) -------------------------------------------------------
def witness_shares(c: Case, r: BwdReference):
    """Share of the rows (keys) concerned that a lost last entry (a lost record) moves by more than 10 Tier A bars."""
    moved = lambda d, bar: (d.abs() / bar.clamp_min(1e-300)).amax(-1) > 10
    rows = r.last_p_row >= 1e-3
    keys = r.last_p_key >= 1e-3
    assert int(rows.sum()) >= 20 and int(keys.sum()) >= 20
    row_share = float(moved(r.last_dq, r.bar["dq"])[rows].double().mean())
    key_share = float((moved(r.last_dk, r.bar["dk"]) & moved(r.last_dv, r.bar["dv"]))[keys].double().mean())
    return row_share, key_share


def scan_chunks(c: Case):
    """Per batch item and scan chunk the kept (row, key) pairs in the chunk's first 1024 counters and in the rest, from the
    oracle's CSR -- launch_bwd_gather's own chunking (32 chunks of L counters, walked 1024 at a time)."""
    C = c.H * c.T_src
    L = -(-(-(-C // 32)) // 1024) * 1024
    out = []
    for n in range(c.N):
        cnt = torch.bincount(c.col[n, :int(c.crow[n, -1])], minlength=C)
        out.append([(int(cnt[lo:lo + 1024].sum()), int(cnt[lo + 1024:min(C, lo + L)].sum())) for lo in range(0, C, L)])
    return C, L, out


def check_case(c: Case, r: BwdReference):
    """What each case is there for."""
    lanes, rpb, rpw = gather_block(c.dtype, c.d) if c.kernel == "gather" else (lanes_per_row(c.dtype, c.d), 0, 0)
    L = c.list_len
    assert int(L.max()) < 2048 and int((L == 0).sum()) > 0 and int((L > 0).sum()) * 4 >= L.numel()
    assert int(r.no_record.sum()) > 0, "a poisoned K / V row"
    assert int(r.records.max()) >= 3, "a key with several records"
    assert int((L == 1).sum()) == 0 and (c.T_src - c.T_dst + 1 if c.causal else c.T_src) >= 2 * c.T_m and c.k >= 2
    if c.name != SCAN:                                                      # (there every list is a multiple of max_k = 16 long)
        assert int(((L % lanes != 0) & (L > 0)).sum()) > 0, "a list that ends inside a lane group's step"
    if c.name == "g4_fp16_d32":
        assert c.T_dst % rpb == 0 and c.T_src % rpb != 0
    if c.name == "g8_bf16_d64":
        assert c.T_src % rpb == 0 and c.T_dst % rpb != 0
    if c.name in KEY0:
        assert lanes == KEY0[c.name]
        found = False
        for n in range(c.N):
            for h in range(c.H):
                if bool(c.kept[n, h, 0]):
                    continue
                for b in range(0, c.T_dst, rpb):                            # the row pass's own blocks
                    ln = L[n, h, b:b + rpb]
                    n0, n1 = int((ln == 0).sum()), int((ln > 0).sum())
                    # rows_by_length ranks by length, ranks w * rpw .. to wave w: the first empty row shares its wave with
                    # a non-empty one when the non-empty count is off a multiple of rpw (a full block: the empty count too)
                    found |= n0 > 0 and n1 > 0 and n0 % rpw != 0 and n1 % rpw != 0
        assert found, "no empty row shares a wave with a non-empty one in a head whose key 0 is NaN"
    if c.name == SCAN:
        C, Lc, chunks = scan_chunks(c)
        assert C > 32768 and C % 1024 != 0 and Lc == 2048 and C % Lc != 0
        assert any(a > 0 and b > 0 for a, b in chunks[0]), "a chunk whose second pass needs the first pass's carry"
        assert sum(1 for a, b in chunks[0] if a + b > 0) >= 3, "chunk bases"
    rows, keys = witness_shares(c, r)
    print(f"[bwd-ref] {c.name}: moved by more than 10 bars -- dQ by a lost last entry {rows:.3f} of the rows, "
          f"dK and dV by a lost record {keys:.3f} of the keys")
    assert rows >= 0.9 and keys >= 0.9, (c.name, rows, keys)


@pytest.mark.parametrize("name", list(SPECS))
def test_case_conditions(name):
    check_case(case(name), reference(name))


def test_case_set_statistics():
    sp = SPECS
    lanes = lambda n: lanes_per_row(sp[n][1], sp[n][2])
    assert {(sp[n][1] == F32, sp[n][2]) for n in GATHER} >= {(False, 32), (False, 64), (False, 128), (False, 80), (False, 40),
                                                           (True, 16), (True, 32), (True, 64), (True, 48)}
    assert {sp[n][1] for n in GATHER} == {BF, FH, F32}
    assert sum(1 for n in GATHER if sp[n][3] == 2 and sp[n][4] in (3, 5)) >= 2
    assert {lanes(n) for n in GATHER if sp[n][10]} == {4, 8, 16}              # a strided case per lane count
    assert [lanes(n) for n in ATOMIC] == [4, 8, 16, 32, 32, 64] and len({sp[n][1] for n in ATOMIC[:3]}) == 3
    assert {(lanes(n), sp[n][1]) for n in AUTOGRAD} == {(l, t) for l in (4, 8, 16) for t in (BF, FH)}
    assert sorted(KEY0.values()) == [4, 8, 16] and all(lanes(n) == l for n, l in KEY0.items())


@pytest.mark.parametrize("name", ["g4_f32_d16", "g16_bf16_d80"])
def test_closed_forms_match_autograd(name):
    """The closed forms of `BwdReference` against torch.autograd in fp64 through softmax(q . k[keys]) @ v[keys], list by
    list (index_select: a key a list holds twice gets both gradients)."""
    c, r = case(name), reference(name)
    q, kk, vv = (x.double().clone().requires_grad_(True) for x in (c.q, c.kk, c.vv))
    dO = r.dout.double()
    loss = torch.zeros((), dtype=torch.float64)
    for (n, h, t), keys in c.ref.keys.items():
        if keys.numel():
            p = torch.softmax(kk[n, h].index_select(0, keys) @ q[n, h, t], 0)
            loss = loss + (p @ vv[n, h].index_select(0, keys)) @ dO[n, h, t]
    loss.backward()
    for nm, x in (("dq", q), ("dk", kk), ("dv", vv)):
        err = (x.grad - r.grads[nm]).abs().max().item()
        scale = r.grads[nm].abs().max().item()
        assert scale > 0.1 and err <= 1e-13 * max(scale, 1.0), (nm, err, scale)
        assert bool((r.bar[nm] >= 0).all()) and float(r.bar[nm].max()) < 1e-4 * scale    # the bars are fp32 rounding, not slack


# ---- on the GPU -----------------------------------------------------------------------------------------------------------
def forward_on_slots(c: Case, stride):
    """(N, stride) fp32: the reference's p on the CSR's slots, NaN past each item's end."""
    pr = torch.full((c.N, stride), float("nan"), dtype=torch.float32)
    for n in range(c.N):
        for t in range(c.T_dst):
            b, e = int(c.crow[n, t]), int(c.crow[n, t + 1])
            heads = torch.div(c.col[n, b:e], c.T_src, rounding_mode="floor")
            for h in range(c.H):
                if c.ref.p[n, h, t] is not None:
                    pr[n, b:e][heads == h] = c.ref.p[n, h, t].float()
    return pr


def run_abi(c: Case, r: BwdReference, form):
    """One backward launch the way _SparseAttentionFn.backward makes it, `form` pinned ("gather" / "atomic") or left to the
    library ("auto"); fp32 (dq, dk, dv)."""
    lib = _lib.load()
    dv_, p_ = c.dev, flat_csr._p
    q, kk, vv, csr = dv_["q"], dv_["kk"], dv_["vv"], dv_["csr"]
    N, H, T_dst, T_src, D = c.N, c.H, c.T_dst, c.T_src, c.d
    if c.strided:
        # K and V share the fused projection's strides, and so does `Case`'s q: here q gets a WIDER row pitch of its own
        # (slot 1 of four, NaN around it), so a pass that walks q with K's strides, or K with q's, reads NaN, inside q's buffer
        qbuf = torch.full((N, T_dst, 4, H, D), float("nan"), dtype=c.dtype, device=DEV)
        qbuf[:, :, 1] = q.permute(0, 2, 1, 3)
        q = qbuf[:, :, 1].permute(0, 2, 1, 3)
        assert q.stride(2) > kk.stride(2) == vv.stride(2) > D and q.stride(0) != kk.stride(0)
    probs = forward_on_slots(c, csr.col.stride(0)).to(DEV)
    out, dout = c.raw.float().to(DEV), r.dout.to(DEV)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=DEV)
    dq = nan(N, H, T_dst, D)
    common = (p_(q), p_(kk), p_(vv), _lib.dtype_code(c.dtype), N, H, T_dst, T_src, D, _lib.strides3(q), _lib.strides3(kk),
              _lib.strides3(vv), p_(csr.crow), p_(csr.col), csr.col.stride(0), p_(csr.head_off), p_(probs), probs.stride(0),
              p_(out), p_(dout), p_(dq))
    dk, dv = nan(N, H, T_src, D), nan(N, H, T_src, D)                       # both forms write every row: neither gets zeros
    code = {"gather": _lib.SEA_ATTN_BWD_GATHER, "atomic": _lib.SEA_ATTN_BWD_ATOMIC, "auto": _lib.SEA_ATTN_BWD_AUTO}[form]
    with torch.cuda.device(q.device):
        nb = int(lib.sea_sparse_attention_bwd_workspace_bytes(_lib.dtype_code(c.dtype), N, H, T_src, D, csr.col.stride(0), code))
        assert (nb > 0) == (form == "gather" or (form == "auto" and lanes_per_row(c.dtype, c.d) <= 16))
        ws = torch.full((nb,), 0xFF, dtype=torch.uint8, device=DEV) if nb else None         # the atomic form: NULL, 0
        _lib.check(lib.sea_sparse_attention_bwd(*common, p_(dk), p_(dv), p_(ws), nb, code, _lib.stream_ptr()),
                   "sea_sparse_attention_bwd")
        torch.cuda.synchronize()
    return {"dq": dq.cpu(), "dk": dk.cpu(), "dv": dv.cpu()}


def check_gradients(c: Case, r: BwdReference, what, got, bars):
    """fp32: |g - ref| <= bar; 16-bit: within 1 ulp of the reference rounded to the type, plus the bar.  Then what is exact."""
    bad = []
    for nm in ("dq", "dk", "dv"):
        g, ref, bar = got[nm], r.grads[nm], bars[nm]
        finite = bool(torch.isfinite(g.float()).all())
        if g.dtype == torch.float32:
            d, lim = (g.double() - ref).abs(), bar
        else:
            r16 = ref.to(g.dtype)
            d, lim = (g.double() - r16.double()).abs(), ulp(r16) + bar
        d = torch.nan_to_num(d, nan=float("inf"))
        ratio = (d / lim.clamp_min(1e-300)).max().item() if float(d.max()) > 0 else 0.0
        print(f"[bwd-ref] {c.name} {what} {nm}: max|err|/bar = {ratio:.3f}  max|err| = {d.max().item():.3e}  "
              f"max|ref| = {ref.abs().max().item():.3e}  finite: {finite}")
        if not finite or not bool((d <= lim).all()):
            bad.append((nm, ratio, finite))
    assert not bad, (c.name, what, bad)
    assert bool((got["dq"][r.empty_rows] == 0).all()), "dQ of a row that keeps nothing"
    assert bool((got["dk"][r.no_record] == 0).all()) and bool((got["dv"][r.no_record] == 0).all()), "a key without a record"


@gpu
@pytest.mark.parametrize("name", GATHER)
def test_gather_form_matches_fp64(name):
    c, r = case(name), reference(name)
    check_selection(c)                                                      # the device CSR is the oracle's
    check_gradients(c, r, "gather", run_abi(c, r, "gather"), r.bar)


@gpu
@pytest.mark.parametrize("name", ATOMIC)
def test_atomic_form_matches_fp64(name):
    c, r = case(name), reference(name)
    check_selection(c)
    check_gradients(c, r, "atomic", run_abi(c, r, "atomic"), r.bar)


@gpu
@pytest.mark.parametrize("name", ["g8_bf16_d64", "a32_f32_d128"])
def test_auto_form_matches_fp64(name):
    """SEA_ATTN_BWD_AUTO on either side of the lane rule: the gather form with its workspace at 8 lanes, the atomic form with
    NULL, 0 at 32 (`run_abi` asserts which the workspace query announces)."""
    c, r = case(name), reference(name)
    check_selection(c)
    check_gradients(c, r, "auto", run_abi(c, r, "auto"), r.bar)


@gpu
@pytest.mark.parametrize("form", ["gather", "atomic"])
@pytest.mark.parametrize("name", AUTOGRAD)
def test_autograd_matches_fp64(name, form, monkeypatch):
    c, r = case(name), reference(name)
    monkeypatch.setattr(flat_csr._SparseAttentionFn, "backward_form", form)
    dv_ = c.dev
    q, kk, vv = (dv_[x].detach().requires_grad_(True) for x in ("q", "kk", "vv"))
    out = ops.sparse_attention_autograd(q, kk, vv, dv_["csr"])
    (out * r.dout.to(DEV)).sum().backward()
    got = {"dq": q.grad.cpu(), "dk": kk.grad.cpu(), "dv": vv.grad.cpu()}
    assert all(g.dtype == c.dtype for g in got.values())
    check_gradients(c, r, f"autograd/{form}", got, r.bar_b)
