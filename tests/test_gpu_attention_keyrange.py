"""-m gpu: the key-range form of the fused sparse attention (`ops.sparse_attention(path="keyrange", range_keys=...)`,
csrc/sea_attn_keyrange.hip) held to an INDEPENDENT reference: the oracle's selection and interpolation on the CPU and an fp64
softmax over the kept keys (`Reference` of tests/test_gpu_decode_reference.py).

Per case the gather form (`path="gather"`) and the key-range form run on the same inputs; with e_g and e_k their max |err|
against the fp64 context and R the number of ranges, the key-range form must keep

    e_k <= 2 e_g + R * 2^-22 * max|ref|

-- the partial walks are the gather walk's own arithmetic on subsets of a row's entries (error of its kind; the factor 2 allows
for another rounding pattern), and per range the combining launch adds, for every output element and for the softmax sum, one
__expf, one multiply and one add: four roundings of 2^-24 relative per range.  Inputs are made on the CPU (so the statistics
each case is there for can be checked without a GPU) and every K / V row no kept key names holds NaN in what the kernels
read: a neighbour's row shows in the result.

Printed per case ("[keyrange] ..."): e_g, e_k and the bound; MI355X values are in DESIGN.md 5.4h.
"""
import functools

import pytest
import torch

from oracle import sea_oracle as O
import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from sea_attention_amd.perlin_attention import attention as A
from test_gpu_decode_reference import Reference, oracle_columns, ulp, unpack_bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LDS_LIST = 8192          # SEA_KEYRANGE_LIST (csrc/sea_attn.hpp): entries of a workgroup's key lists in LDS, shared out evenly



def rows_per_block(dtype, d):
    """... to its rows: 8 waves of 64 / lanes rows -- 64 rows of 8 lanes (16-bit d = 64, fp32 d = 32), 32 rows of 16 lanes."""
    return 64 if d * (4 if dtype == torch.float32 else 2) <= 128 else 32


# name: (dtype, d, N, H, T_dst, T_src, T_m, max_k, keep, is_causal, range_keys)
CASES = {
    "A": (torch.bfloat16, 64, 1, 4, 64, 1100, 32, 4, 40, True, 100),
    "B": (torch.float16, 128, 1, 2, 33, 2100, 64, 8, 24, True, 256),
    "C": (torch.float32, 64, 2, 8, 200, 520, 32, 16, "module", True, 128),
    "D": (torch.bfloat16, 64, 2, 4, 300, 300, 32, 2, 12, True, 64),
    "E": (torch.bfloat16, 64, 1, 2, 32, 2100, 64, 16, 64, True, 1100),
    "F": (torch.bfloat16, 64, 1, 2, 40, 40, 32, 4, 8, False, 16),
}


class Case:
    """Inputs (CPU), the oracle's selection and columns, the entry statistics and the fp64 reference of one case."""

    def __init__(self, name):
        (self.dtype, self.d, self.N, self.H, self.T_dst, self.T_src, self.T_m, self.k, keep, self.causal,
         self.range_keys) = CASES[name]
        self.name = name
        self.rpb = rows_per_block(self.dtype, self.d)
        N, H, T_dst, T_src, T_m, d = self.N, self.H, self.T_dst, self.T_src, self.T_m, self.d
        g = torch.Generator().manual_seed(1000 + ord(name))
        if name == "E":                                   # one head takes the budget; no softmax: only the order matters
            probs = torch.rand((N, H, T_dst, T_m), generator=g) * 1e-3
            probs[:, 1] += 1
        else:
            probs = torch.softmax(torch.randn((N, H, T_dst, T_m), generator=g), -1)
        self.probs = probs
        if keep == "module":
            self.keep = torch.clamp_max(O.keep_counts_module(H, T_dst, T_m, self.k), H * T_m).to(torch.int32)
        else:
            self.keep = torch.full((T_dst,), keep, dtype=torch.int32)
        self.mask = O.grouped_topk_mask(probs, self.keep)
        self.crow, self.col = O.resize_m_to_t_csr(self.mask, self.k, target_width=T_src, is_causal=self.causal)
        self.R = -(-T_src // self.range_keys)
        self.q = (torch.randn((N, H, T_dst, d), generator=g) * d ** -0.5).to(self.dtype)
        self.kk = torch.randn((N, H, T_src, d), generator=g).to(self.dtype)
        self.vv = torch.randn((N, H, T_src, d), generator=g).to(self.dtype)
        self.rs = torch.rand((N, H, T_dst), generator=g) * 0.5 + 0.5
        self.mix = torch.rand((N, H, T_dst), generator=g) * 0.5 + 0.5
        self.avg = torch.randn((N, H, T_dst, d), generator=g).to(self.dtype)
        self._stats()

    def _stats(self):
        """Per kept pixel: width, entries, lowest / highest key; per (n, h, t) list: length, ranges it spans; per (row block,
        range): entries.  A pixel belongs to the range that holds its lowest key."""
        N, H, T_dst, T_src, T_m, rk = self.N, self.H, self.T_dst, self.T_src, self.T_m, self.range_keys
        vs, ve = O.pixel_bounds(T_dst, T_src, T_m, self.causal)
        width = (ve - vs).to(torch.int64)                                       # (T_dst, T_m)
        self.pix_width, self.pix_straddles = [], 0
        self.list_len = torch.zeros((N, H, T_dst), dtype=torch.int64)
        self.list_spans = torch.zeros((N, H, T_dst), dtype=torch.int64)
        self.block_range = torch.zeros((N, H, -(-T_dst // self.rpb), self.R), dtype=torch.int64)
        kept = torch.zeros((N, H, T_src), dtype=torch.bool)
        for n in range(N):
            for t in range(T_dst):
                e = int(self.crow[n, t])
                for h in range(H):
                    ranges = set()
                    for b in self.mask[n, h, t].nonzero().view(-1).tolist():
                        cnt = min(int(width[t, b]), self.k)
                        if cnt == 0:
                            continue
                        keys = self.col[n, e:e + cnt] - h * T_src
                        assert int(keys.min()) >= 0 and int(keys.max()) < T_src
                        e += cnt
                        lo, hi = int(keys.min()), int(keys.max())
                        kept[n, h, keys] = True
                        self.pix_width.append(int(width[t, b]))
                        self.pix_straddles += lo // rk != hi // rk
                        ranges.add(lo // rk)
                        self.list_len[n, h, t] += cnt
                        self.block_range[n, h, t // self.rpb, lo // rk] += cnt
                    self.list_spans[n, h, t] = len(ranges)
                assert e == int(self.crow[n, t + 1])
        self.kept = kept

    @functools.cached_property
    def dev(self):
        """Device tensors; K / V as the kernels see them: NaN in every row no kept key names."""
        c = lambda x: x.to(DEV)
        poison = (~self.kept).unsqueeze(-1).to(DEV)
        nan = torch.full((), float("nan"), dtype=self.dtype, device=DEV)
        return dict(q=c(self.q), kk=torch.where(poison, nan, c(self.kk)), vv=torch.where(poison, nan, c(self.vv)),
                    kk_clean=c(self.kk), vv_clean=c(self.vv), rs=c(self.rs), mix=c(self.mix), avg=c(self.avg),
                    probs=c(self.probs), keep=c(self.keep))

    @functools.cached_property
    def ref(self):
        dv = self.dev
        return Reference(dv["q"], dv["kk_clean"], dv["vv_clean"], self.crow, self.col, self.T_src, row_scale=dv["rs"],
                         avg=dv["avg"], mix=dv["mix"])

    def handle(self):
        dv = self.dev
        csr = ops.topk_to_csr(dv["probs"], dv["keep"], self.k, target_width=self.T_src, is_causal=self.causal, defer_emit=True)[0]
        assert csr.col_is_pending
        return csr

    def run(self, path, range_keys=None, out16=False, csr=None):
        """One launch on a fresh handle with pending columns: fp32 (N, H, T_dst, d), or 16-bit into a permuted (N, T, H*d) buffer."""
        dv = self.dev
        csr = csr if csr is not None else self.handle()
        out = None
        if out16:
            buf = torch.full((self.N, self.T_dst, self.H * self.d), float("nan"), dtype=self.dtype, device=DEV)
            out = buf.view(self.N, self.T_dst, self.H, self.d).permute(0, 2, 1, 3)
        kw = dict(range_keys=range_keys) if path == "keyrange" else dict(keep_columns_pending=True)
        o = ops.sparse_attention(dv["q"], dv["kk"], dv["vv"], csr, row_scale=dv["rs"], avg=dv["avg"], mix=dv["mix"], out=out,
                                 path=path, **kw)
        return o, csr


@functools.lru_cache(maxsize=None)
def case(name) -> Case:
    return Case(name)


def check_selection(c: Case, csr):
    assert torch.equal(unpack_bits(csr.bits, c.H, c.T_m), c.mask), "selection bits != oracle mask"
    assert torch.equal(csr.crow.cpu().long(), c.crow)


def check_precondition(c: Case):
    """What each case is there for, from the oracle's selection (no GPU work)."""
    w = torch.tensor(c.pix_width)
    n_lists = c.N * c.H * c.T_dst
    multi = int((c.list_spans > 1).sum())
    if c.name == "A":
        assert c.R == 11 and bool((w > c.k).all()) and int(w.max()) >= 30        # every kept pixel thinned
        assert multi >= n_lists * 9 // 10 and c.pix_straddles >= 500             # lists span ranges, pixels straddle boundaries
    if c.name == "B":
        assert c.R == 9 and c.T_dst % 32 != 0 and int(c.list_len.max()) >= 100 and multi > n_lists // 2
    if c.name == "C":
        assert c.N == 2 and c.R == 5 and multi >= n_lists // 5
        assert int((w <= c.k).sum()) > 0 and c.pix_straddles > 0
    if c.name == "D":
        assert c.R == 5 and int((c.list_len == 0).sum()) > 0                     # empty (row, head) lists
        assert c.T_dst > 2 * c.rpb and c.range_keys * (c.R - 1) >= c.rpb   # whole row blocks below a range
        assert int(c.block_range[:, :, 0, 1:].sum()) == 0 and int(c.block_range[:, :, -1, -1].sum()) > 0
    if c.name == "E":
        assert c.R == 2 and int(c.list_len[:, 0].max()) == 0 and int(c.list_len[:, 1].min()) == 64 * 16
        assert int(c.block_range[0, 1].min()) > LDS_LIST                         # a row block's entries of ONE range
        per_row = c.block_range[0, 1, 0] // c.T_dst
        assert int(per_row.min()) > LDS_LIST // c.rpb                   # ... and a row's share of the list
    if c.name == "F":
        assert not c.causal and c.R == 3 and multi > 0


def errors(c: Case, o32):
    return (o32.double().cpu() - c.ref.out).abs().max().item()


@pytest.mark.parametrize("name", list(CASES))
def test_keyrange_matches_fp64(name):
    c = case(name)
    check_precondition(c)
    ok, csr_k = c.run("keyrange", c.range_keys)
    assert csr_k.col_is_pending
    check_selection(c, csr_k)
    og, _ = c.run("gather")
    ref = c.ref
    e_g, e_k = errors(c, og), errors(c, ok)
    bound = 2 * e_g + c.R * 2.0 ** -22 * ref.out.abs().max().item()
    print(f"[keyrange] case {name}: R = {c.R}  e_g = {e_g:.3e}  e_k = {e_k:.3e}  bound = {bound:.3e}")
    assert torch.isfinite(ok).all() and torch.isfinite(og).all()
    assert e_k <= bound, (name, e_k, bound)
    sens = ref.sensitivity(c.T_src)
    assert sens >= 10 * bound, (name, "a wrong key would pass", sens, bound)
    if c.dtype != torch.float32:
        o16, _ = c.run("keyrange", c.range_keys, out16=True)
        r16 = ref.out.to(c.dtype)
        d16 = (o16.cpu().double() - r16.double()).abs()
        lim = ulp(r16) + bound
        assert torch.isfinite(o16.float()).all() and bool((d16 <= lim).all()), (name, (d16 / lim).max().item())


@pytest.mark.parametrize("name", ["A", "B"])
def test_one_range_is_the_gather_form_bit_for_bit(name):
    """range_keys >= T_src: one range -- the two new kernels still run, and only the combine's arithmetic (a weight of
    exp(0) = 1) separates them from the gather form: the walk, the state layout and the epilogue are pinned."""
    c = case(name)
    rk = c.T_src + 5
    assert c.T_src <= rk < 32768
    for out16 in (False, True):
        ok, csr = c.run("keyrange", rk, out16=out16)
        assert csr.col_is_pending
        og, _ = c.run("gather", out16=out16)
        assert torch.equal(ok, og), (name, out16, (ok.float() - og.float()).abs().max().item())


def test_keyrange_is_deterministic():
    c = case("A")
    a, _ = c.run("keyrange", c.range_keys)
    b, _ = c.run("keyrange", c.range_keys)
    assert torch.equal(a, b)


def test_keyrange_leaves_the_columns_pending():
    c = case("A")
    _, csr = c.run("keyrange", c.range_keys)
    assert csr.col_is_pending
    col = csr.col.cpu().long()                                                  # the emit launch, now
    assert not csr.col_is_pending
    crow_o, col_o = oracle_columns(c.mask, c.k, c.T_src, c.T_src)
    assert torch.equal(crow_o, c.crow)
    for n in range(c.N):
        z = int(crow_o[n, -1])
        assert torch.equal(col[n, :z], col_o[n, :z])


def test_keyrange_in_a_graph():
    c = case("A")
    dv = c.dev
    eager, _ = c.run("keyrange", c.range_keys)
    csr = c.handle()
    out = torch.empty_like(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.sparse_attention(dv["q"], dv["kk"], dv["vv"], csr, row_scale=dv["rs"], avg=dv["avg"], mix=dv["mix"], out=out,
                             path="keyrange", range_keys=c.range_keys)
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager)


class Cfg:
    def __init__(self, hidden, heads, max_pos):
        self.hidden_size, self.num_attention_heads, self.max_position_embeddings = hidden, heads, max_pos


def test_module_key_range(monkeypatch):
    N, H, d, T, T_m, k, dtype, key_range = 1, 4, 64, 1024, 64, 16, torch.bfloat16, 256
    S.seed(42)
    pc = PerlinAttentionConfig(k=k, attention_predictor_length=T_m, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix')
    layer = PerlinSelfAttention(Cfg(H * d, H, T), pc).to(DEV).to(dtype).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = True
    layer.attention.assume_not_padded = True
    assert layer.attention.key_range is None
    S.seed(7)
    x = torch.randn((N, H, T, d), device=DEV)
    q, kk, vv = (x * d ** -0.5).to(dtype), torch.randn_like(x).to(dtype), torch.randn_like(x).to(dtype)
    fp_min = torch.finfo(torch.float16).min / 2
    ar = torch.arange(T, device=DEV)
    amask = ((ar.view(1, T) > ar.view(T, 1)).to(dtype) * fp_min).view(1, 1, T, T)
    seen = []
    real = A.ops.sparse_attention

    def spy(q_, k_, v_, csr, **kw):
        seen.append(dict(q=q_, k=k_, v=v_, csr=csr, kw=kw))
        return real(q_, k_, v_, csr, **kw)
    monkeypatch.setattr(A.ops, "sparse_attention", spy)

    def forward(kr, want_probs=False):
        layer.attention.key_range = kr
        layer.attention.return_attention_probs = want_probs
        with torch.no_grad():
            out = layer(None, None, None, query_layer=q, key_layer=kk, value_layer=vv, attention_mask=amask)
        torch.cuda.synchronize()
        return out

    base = forward(None)
    assert seen[-1]["kw"].get("path") != "keyrange"
    kr = forward(key_range)
    call = seen[-1]
    assert call["kw"]["path"] == "keyrange" and call["kw"]["range_keys"] == key_range
    assert kr.partial_attention_mask.col_is_pending
    # the same selection and map
    assert torch.equal(kr.partial_attention_mask.bits, base.partial_attention_mask.bits)
    assert torch.equal(kr.partial_attention_mask.crow, base.partial_attention_mask.crow)
    z = int(base.partial_attention_mask.crow[0, -1])                            # (entries past the last row's end are undefined)
    assert torch.equal(kr.partial_attention_mask.col[:, :z], base.partial_attention_mask.col[:, :z])
    assert torch.equal(ops.realize(kr.estimated_attention_probs_m), ops.realize(base.estimated_attention_probs_m))
    # fp64 reference on the launch's own inputs: a dense masked softmax over the kept keys (no pixel is thinned here: no
    # duplicate entries)
    kw = call["kw"]
    keep = ops.flat_csr_to_dense(kr.partial_attention_mask, T, H).double()
    assert float(keep.max()) == 1.0
    s = call["q"].double() @ call["k"].double().transpose(-1, -2)
    p = torch.nan_to_num(torch.softmax(s.masked_fill(keep == 0, float("-inf")), -1), nan=0.0)      # (a head that keeps nothing: 0)
    o = (p @ call["v"].double()) * kw["row_scale"].double().unsqueeze(-1)
    a = kw["mix"].double().unsqueeze(-1)
    ref = (o * a + (1 - a) * kw["avg"].double()).permute(0, 2, 1, 3).reshape(N, T, H * d)
    e_g = (base.context_layer.double() - ref).abs().max().item()
    e_k = (kr.context_layer.double() - ref).abs().max().item()
    R = -(-T // key_range)
    bound = 2 * e_g + R * 2.0 ** -22 * ref.abs().max().item()
    print(f"[keyrange] module: R = {R}  e_g = {e_g:.3e}  e_k = {e_k:.3e}  bound = {bound:.3e}")
    assert torch.isfinite(kr.context_layer).all() and e_k <= bound, (e_k, bound)
    # with the probabilities wanted the layer takes today's path
    forward(key_range, want_probs=True)
    assert seen[-1]["kw"].get("path") != "keyrange" and seen[-1]["kw"]["want_probs"]
    # keys within one range: today's path as well
    forward(T)
    assert seen[-1]["kw"].get("path") != "keyrange"


def test_keyrange_refusals_through_python():
    c = case("A")
    dv = c.dev
    args = (dv["q"], dv["kk_clean"], dv["vv_clean"])
    emitted = c.handle()
    emitted.col                                                                 # a handle whose columns are written
    with pytest.raises(ValueError, match="pending"):
        ops.sparse_attention(*args, emitted, path="keyrange", range_keys=100)
    with pytest.raises(ValueError, match="probabilities"):
        ops.sparse_attention(*args, c.handle(), path="keyrange", range_keys=100, want_probs=True)
    plan = torch.zeros((((c.N * c.H * ((c.T_dst + 15) // 16) + 3) & ~3) + 4,), dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError, match="plan"):
        ops.sparse_attention(*args, c.handle(), path="keyrange", range_keys=100, plan=plan)
    with pytest.raises(ValueError, match="range_keys"):
        ops.sparse_attention(*args, c.handle(), path="keyrange")
    for bad in (0, 32768):
        with pytest.raises(ValueError, match="range_keys"):
            ops.sparse_attention(*args, c.handle(), path="keyrange", range_keys=bad)
    with pytest.raises(ValueError, match="64 ranges"):
        ops.sparse_attention(*args, c.handle(), path="keyrange", range_keys=10)
    with pytest.raises(ValueError, match="range_keys"):
        ops.sparse_attention(*args, c.handle(), path="gather", range_keys=100)
    q80 = torch.zeros((c.N, c.H, c.T_dst, 80), dtype=c.dtype, device=DEV)
    kv80 = torch.zeros((c.N, c.H, c.T_src, 80), dtype=c.dtype, device=DEV)
    with pytest.raises(ValueError, match="d = 80"):
        ops.sparse_attention(q80, kv80, kv80, c.handle(), path="keyrange", range_keys=100)
    torch.cuda.synchronize()
