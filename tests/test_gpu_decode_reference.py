"""-m gpu: decode attention held to an INDEPENDENT reference -- the oracle's selection and interpolation
(oracle/sea_oracle.py) plus an fp64 softmax on the CPU -- instead of to another form of the build.

Every decode form of `sea_sparse_attention` (sparse_attn_decode1_kernel for one new row, the DEC instantiations of
sparse_attn_rows_kernel / sparse_attn_rows80_kernel for 2..8 rows) and the decode form of `sea_csr_emit` expand a thinned
pixel with the same fp32 column arithmetic, so the tests that compare them with each other cannot see a bug in it.  Here:

  (a) the decode operator against fp64, on the edges where the kernels branch (first position, pixel widths stepping past a
      multiple of T_M, heads of thousands of entries, every pixel thinned, empty heads, ragged row totals, unwritten cache
      rows holding a sentinel);
  (b) the same with a long cache capacity ((H - 1) * T_cap far above 2^24, K / V over 4 GiB): the capacity the column ids are
      encoded with must not change a bit;
  (c) a DecodeSession's columns on EVERY step, eager and graph-replayed, fused attention or not, and the round-4 launches;
  (d) two sessions that differ only in their capacity: bitwise the same context, map and columns.
"""
import pytest
import torch

import sea_attention_amd as S
from oracle import sea_oracle as O
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from sea_attention_amd.perlin_attention.decode import DecodeSession

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_M = 256
# fp32 context against the fp64 reference: max |err| over every case of this file observed 4.9e-7 on MI355X (outputs O(1))
TOL32 = 2e-6
SENT_V = 1000.0          # V rows at and past T_src (never written by a real session): any read of one shows as a large error


# ---- the reference ----------------------------------------------------------------------------------------------------
def unpack_bits(bits, H, T_m):
    """(N, T_dst, W) kept-pixel words -> 0/1 fp32 mask (N, H, T_dst, T_m): bit f % 32 of word f // 32 is flat pixel f = h*T_m + b."""
    N, T_dst, W = bits.shape
    b = bits.cpu().to(torch.int64) & 0xffffffff
    flat = ((b.unsqueeze(-1) >> torch.arange(32)) & 1).reshape(N, T_dst, W * 32)[:, :, :H * T_m]
    return flat.reshape(N, T_dst, H, T_m).transpose(1, 2).float()


def oracle_columns(mask, k, T_src, T_cap):
    """The oracle's CSR of the last T_dst rows of a T_src-long sequence, ids re-encoded from h*T_src + key to h*T_cap + key."""
    crow, col = O.resize_m_to_t_csr(mask, k, target_width=T_src, is_causal=True)
    return crow, (col // T_src) * T_cap + col % T_src


def _neighbour(key, T_src):
    return key + 1 if key + 1 < T_src or key == 0 else key - 1


class Reference:
    """fp64 o = softmax(q . k_e) v_e over each (n, h, row)'s kept keys, times row_scale, then the mix with avg -- the form
    `sea_sparse_attention` documents (an empty head contributes o = 0).  K / V rows are gathered from the device tensors."""

    def __init__(self, q, kk, vv, crow, col, T_cap, row_scale=None, avg=None, mix=None):
        self.q, self.kk, self.vv, self.T_cap = q.double().cpu(), kk, vv, T_cap
        self.rs = row_scale.double().cpu() if row_scale is not None else None
        self.avg = avg.double().cpu() if avg is not None else None
        self.mix = mix.double().cpu() if mix is not None else None
        N, H, T_dst, D = q.shape
        self.keys = {}
        for n in range(N):
            for t in range(T_dst):
                ids = col[n, int(crow[n, t]):int(crow[n, t + 1])]
                hs = torch.div(ids, T_cap, rounding_mode="floor")
                for h in range(H):
                    self.keys[n, h, t] = ids[hs == h] - h * T_cap
        self.out = torch.zeros((N, H, T_dst, D), dtype=torch.float64)
        self.best, best_p = None, -1.0
        for (n, h, t), keys in self.keys.items():
            o, p = self.head(n, h, t, keys)
            self.out[n, h, t] = self.epilogue(n, h, t, o)
            if p is not None and float(p.max()) > best_p:
                best_p, self.best = float(p.max()), (n, h, t, int(p.argmax()))

    def head(self, n, h, t, keys):
        if keys.numel() == 0:
            return torch.zeros(self.q.shape[-1], dtype=torch.float64), None
        idx = keys.to(self.kk.device)
        kr = self.kk[n, h].index_select(0, idx).double().cpu()
        vr = self.vv[n, h].index_select(0, idx).double().cpu()
        p = torch.softmax(kr @ self.q[n, h, t], 0)
        return p @ vr, p

    def epilogue(self, n, h, t, o):
        if self.rs is not None:
            o = o * self.rs[n, h, t]
        if self.mix is not None:
            a = self.mix[n, h, t]
            o = o * a + (1.0 - a) * self.avg[n, h, t]
        return o

    def sensitivity(self, T_src):
        """max |change| of the reference when its most probable kept key is replaced by its neighbour: what the comparison
        must be able to see."""
        n, h, t, i = self.best
        keys = self.keys[n, h, t].clone()
        keys[i] = _neighbour(int(keys[i]), T_src)
        o = self.epilogue(n, h, t, self.head(n, h, t, keys)[0])
        return float((o - self.out[n, h, t]).abs().max())


def ulp(x: torch.Tensor) -> torch.Tensor:
    """Spacing of the 16-bit grid at |x| (x in its own dtype), as fp64."""
    a = x.abs()
    return (torch.nextafter(a, torch.full_like(a, float("inf"))) - a).double()


def check_outputs(ref: Reference, o32, o16, T_src, what):
    """fp32 context within TOL32 of fp64; 16-bit context within 1 ulp of the fp64 value rounded to its dtype (plus the fp32
    tolerance, which only matters where the 16-bit grid is finer than it: near zero); the comparison can fail."""
    err = (o32.double().cpu() - ref.out).abs().max().item()
    print(f"[decode-ref] {what}: fp32 max|err| = {err:.3e}")
    assert torch.isfinite(o32).all() and err <= TOL32, (what, err)
    if o16 is not None:
        r16 = ref.out.to(o16.dtype)
        d16 = (o16.cpu().double() - r16.double()).abs()
        bound = ulp(r16) + TOL32
        worst = (d16 / bound).max().item()
        assert torch.isfinite(o16.float()).all() and bool((d16 <= bound).all()), (what, worst)
    sens = ref.sensitivity(T_src)
    assert sens >= 10 * TOL32, (what, "a wrong key would pass", sens)


def check_columns(csr, crow_o, col_o, what):
    N = crow_o.shape[0]
    assert torch.equal(csr.crow.cpu().long(), crow_o), what
    col = csr.col.cpu().long()
    for n in range(N):
        z = int(crow_o[n, -1])
        assert torch.equal(col[n, :z], col_o[n, :z]), (what, n)


# ---- (a) the decode operator against fp64 -----------------------------------------------------------------------------
def _selection(dtype, N, H, T_dst, T_src, k, keep_count, heavy, seed):
    S.seed(seed)
    probs = torch.rand((N, H, T_dst, T_M), device=DEV) * 0.1
    if heavy:
        probs[:, 0] += 1.0                                                  # head 0 wins the pooled top-k
        probs[N - 1, 1] = 0.0                                               # ... and the last item's head 1 keeps nothing
    if T_src < T_M:                                                         # most pixels of a short row are empty: favour the others
        vs, ve = O.pixel_bounds(T_dst, T_src, T_M, True)
        probs += ((ve - vs) > 0).any(0).to(probs.device).float()
    probs = probs.to(dtype)
    keep = torch.full((T_dst,), keep_count, dtype=torch.int32, device=DEV)
    sel = ops.topk_to_csr(probs, keep, k, target_width=T_src, is_causal=True)[0]
    mask = O.grouped_topk_mask(probs.float().cpu(), keep.cpu())
    assert torch.equal(unpack_bits(sel.bits, H, T_M), mask), "selection bits != oracle mask"
    assert int(sel.row_nnz.min()) > 0
    return sel, mask


def _caches(N, H, T_src, T_cap, d, dtype):
    """K / V caches of T_cap rows: random rows below T_src; at and past T_src K = 0 (a score of 0: never masked out by a huge
    negative score) and V = SENT_V."""
    kk = torch.empty((N, H, T_cap, d), dtype=dtype, device=DEV)
    vv = torch.empty((N, H, T_cap, d), dtype=dtype, device=DEV)
    kk[:, :, :T_src] = torch.randn((N, H, T_src, d), device=DEV).to(dtype)
    vv[:, :, :T_src] = torch.randn((N, H, T_src, d), device=DEV).to(dtype)
    kk[:, :, T_src:] = 0
    vv[:, :, T_src:] = SENT_V
    return kk, vv


def _decode_call(q, kk, vv, sel, H, T_src, T_cap, k, N, T_dst, z_cap, pending, **epi):
    """One decode-form launch: fp32 context, then a 16-bit one (16-bit data) on a fresh handle; returns (o32, o16, csr32)."""
    ts = torch.tensor([T_src], dtype=torch.int32, device=DEV)
    outs = []
    for odt in ([None, q.dtype] if q.dtype != torch.float32 else [None]):
        csr = ops.csr_from_selection(sel.bits, sel.row_nnz, sel.head_off, H, T_M, T_cap, k, True, z_cap, t_src_dev=ts,
                                     defer_emit=True)
        o = ops.sparse_attention(q, kk, vv, csr, path="gather", keep_columns_pending=pending, out_dtype=odt, **epi)
        assert csr.col_is_pending == pending                                # the fused decode form served the launch
        outs.append((o, csr))
    return outs[0][0], (outs[1][0] if len(outs) > 1 else None), outs[0][1]


# (dtype, d, T_dst, T_src, k, keep, heavy): decode1 for T_dst = 1 (16-bit), DEC lane-group forms for 2..8 rows and fp32
CASES_A = [
    (torch.bfloat16, 64, 1, 1, 16, 37, False),         # the very first position: one key per head
    (torch.float16, 128, 1, 257, 16, 61, False),       # just past T_M: widths 1 and 2
    (torch.bfloat16, 80, 1, 513, 16, 61, False),       # just past 2 T_M
    (torch.bfloat16, 64, 1, 3000, 64, 341, True),      # head 0 ~ thousands of entries (12 chunks of 256); an empty head
    (torch.float16, 64, 1, 3000, 4, 341, True),        # every pixel thinned (widths 11 / 12 -> 4)
    (torch.bfloat16, 128, 1, 3000, 64, 341, True),     # 16-lane rows: chunks of 128
    (torch.float16, 80, 1, 517, 16, 37, False),        # ragged head totals (% 4 != 0)
    (torch.float16, 64, 1, 1100, 4, 200, False),       # thinned widths 5 -> 4 next to unthinned 4
    (torch.bfloat16, 64, 2, 257, 16, 61, False),
    (torch.float16, 80, 3, 1500, 4, 120, True),
    (torch.bfloat16, 128, 8, 513, 16, 61, False),
    (torch.float16, 64, 8, 3000, 64, 341, True),
    (torch.bfloat16, 80, 2, 2, 16, 37, False),         # two rows of a two-token sequence
    (torch.float16, 128, 3, 257, 4, 90, False),
    (torch.float32, 64, 1, 3000, 64, 341, True),       # fp32 data: the DEC lane-group form serves one row too
    (torch.float32, 64, 3, 257, 4, 90, False),
]


def _case_id(c):
    dt = {torch.bfloat16: "bf16", torch.float16: "fp16", torch.float32: "fp32"}[c[0]]
    return f"{dt}-d{c[1]}-rows{c[2]}-T{c[3]}-k{c[4]}" + ("-heavy" if c[6] else "")


@pytest.mark.parametrize("pending", [True, False], ids=["cols_pending", "write_cols"])
@pytest.mark.parametrize("dtype,d,T_dst,T_src,k,keep_count,heavy", CASES_A, ids=[_case_id(c) for c in CASES_A])
def test_decode_operator_matches_fp64(dtype, d, T_dst, T_src, k, keep_count, heavy, pending):
    N, H = 2, 4 if heavy else 8
    T_cap = T_src + 40
    sel, mask = _selection(dtype, N, H, T_dst, T_src, k, keep_count, heavy, seed=T_src + 7 * T_dst + d)
    crow_o, col_o = oracle_columns(mask, k, T_src, T_cap)
    z_cap = max(int(sel.crow[:, -1].max().item()), 1)
    kk, vv = _caches(N, H, T_src, T_cap, d, dtype)
    q = (torch.randn((N, H, T_dst, d), device=DEV) * d ** -0.5).to(dtype)
    rs = torch.rand((N, H, T_dst), device=DEV) * 0.5 + 0.5
    mix = torch.rand((N, H, T_dst), device=DEV) * 0.5 + 0.5
    avg = torch.randn((N, H, T_dst, d), device=DEV).to(dtype)
    epi = dict(row_scale=rs, avg=avg, mix=mix)
    o32, o16, csr = _decode_call(q, kk, vv, sel, H, T_src, T_cap, k, N, T_dst, z_cap, pending, **epi)
    check_columns(csr, crow_o, col_o, "columns")                            # pending: emitted on this read; else the launch's
    ref = Reference(q, kk, vv, crow_o, col_o, T_cap, **epi)
    check_outputs(ref, o32, o16, T_src, _case_id((dtype, d, T_dst, T_src, k, keep_count, heavy)))
    # the edges this case is there for
    ho = sel.head_off.cpu()
    per_head = ho[..., 1:] - ho[..., :-1]                                   # (N, T_dst, H)
    if heavy:
        assert int(per_head[0, 0, 0]) > (1000 if k > 4 else 300)           # many chunks
        assert int(per_head[N - 1, :, 1].max()) == 0                        # an empty head
        empty = ((1.0 - mix[N - 1, 1]).unsqueeze(-1) * avg[N - 1, 1].float())
        assert torch.allclose(o32[N - 1, 1], empty, rtol=0, atol=1e-6)
    if T_src == 517:
        assert bool((per_head % 4 != 0).any())
    if k == 4 and T_src >= 4 * T_M + 1:
        w = T_src - T_dst + 1                                               # the narrowest row
        assert w // T_M >= k                                                # every pixel of every row is thinned


# ---- (b) long capacity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,d,T_cap,T_dst,dtype", [(32, 64, 1 << 20, 1, torch.bfloat16),
                                                   (32, 64, 1 << 20, 3, torch.float16),
                                                   (40, 128, 450_000, 1, torch.bfloat16)])   # K and V 4.6 GB each
def test_decode_operator_long_capacity(H, d, T_cap, T_dst, dtype):
    """(H - 1) * T_cap far above 2^24, a short sequence with thinned pixels (T_src = 1100, k = 4: widths 5 -> 4): the
    output is bitwise the same call's with a small capacity, the columns are the oracle's, the fp64 check of (a) holds --
    for the fused decode form and for the decode form of sea_csr_emit + the unfused launch."""
    N, T_src, k, keep_count = 1, 1100, 4, (H * T_M) // 4
    assert (H - 1) * T_cap > (1 << 24)
    sel, mask = _selection(dtype, N, H, T_dst, T_src, k, keep_count, False, seed=H + T_dst)
    z_cap = max(int(sel.crow[:, -1].max().item()), 1)
    T_small = T_src + 3
    ks, vs = _caches(N, H, T_src, T_small, d, dtype)
    q = (torch.randn((N, H, T_dst, d), device=DEV) * d ** -0.5).to(dtype)
    rs = torch.rand((N, H, T_dst), device=DEV) * 0.5 + 0.5
    try:
        kb = torch.empty((N, H, T_cap, d), dtype=dtype, device=DEV)
        vb = torch.empty((N, H, T_cap, d), dtype=dtype, device=DEV)
        kb[:, :, :T_src], vb[:, :, :T_src] = ks[:, :, :T_src], vs[:, :, :T_src]
        kb[:, :, T_src:], vb[:, :, T_src:] = 0, SENT_V
        small = _decode_call(q, ks, vs, sel, H, T_src, T_small, k, N, T_dst, z_cap, False, row_scale=rs)
        big = _decode_call(q, kb, vb, sel, H, T_src, T_cap, k, N, T_dst, z_cap, False, row_scale=rs)
        assert torch.equal(big[0], small[0]) and torch.equal(big[1], small[1]), "the capacity changed the context"
        crow_o, col_o = oracle_columns(mask, k, T_src, T_cap)
        check_columns(big[2], crow_o, col_o, "fused decode form, written by the launch")
        heads = torch.div(col_o[0, :int(crow_o[0, -1])], T_cap, rounding_mode="floor")
        assert int(heads.max()) * T_cap >= (1 << 24)                        # ids the fp32 stepping of h*T_cap + key rounds
        ref = Reference(q, kb, vb, crow_o, col_o, T_cap, row_scale=rs)
        check_outputs(ref, big[0], big[1], T_src, f"H{H}-d{d}-Tcap{T_cap}-rows{T_dst}")
        # the pending handle's columns (decode form of sea_csr_emit), and that emit + the unfused launch
        ts = torch.tensor([T_src], dtype=torch.int32, device=DEV)
        cp = ops.csr_from_selection(sel.bits, sel.row_nnz, sel.head_off, H, T_M, T_cap, k, True, z_cap, t_src_dev=ts, defer_emit=True)
        op = ops.sparse_attention(q, kb, vb, cp, row_scale=rs, path="gather", keep_columns_pending=True)
        assert cp.col_is_pending and torch.equal(op, small[0])
        check_columns(cp, crow_o, col_o, "decode form of sea_csr_emit")
        cu = ops.csr_from_selection(sel.bits, sel.row_nnz, sel.head_off, H, T_M, T_cap, k, True, z_cap, t_src_dev=ts)
        ou = ops.sparse_attention(q, kb, vb, cu, row_scale=rs, path="gather")
        assert torch.equal(ou, small[0]), "emit + unfused launch at the long capacity"
        torch.cuda.synchronize()
    finally:
        kb = vb = ref = None                                                # (the reference holds the caches too)
        torch.cuda.empty_cache()


def test_stateless_fused_attention_refuses_inexact_ids():
    """The stateless fused form steps a thinned pixel on h*T_src + key in fp32 (the reference's arithmetic): like sea_csr_emit
    it refuses H*T_src >= 2^24 instead of computing.  (K / V are stride-0 views: nothing T_src-sized is allocated.)"""
    N, H, T_dst, k, d = 1, 64, 33, 64, 64                                   # N*H*T_dst > attention_few_rows(): the fused form
    T_src = (1 << 24) // H
    assert N * H * T_dst > ops.attention_few_rows() and ops.fused_interp_supported(torch.bfloat16, d, T_M, N * H * T_dst)
    S.seed(4)
    probs = torch.rand((N, H, T_dst, T_M), device=DEV).to(torch.bfloat16)
    keep = torch.full((T_dst,), 500, dtype=torch.int32, device=DEV)
    sel = ops.topk_to_csr(probs, keep, k, target_width=T_src, is_causal=True, defer_emit=True)[0]
    assert sel.col_is_pending
    q = (torch.randn((N, H, T_dst, d), device=DEV) * d ** -0.5).to(torch.bfloat16)
    row = torch.randn((N, H, 1, d), device=DEV).to(torch.bfloat16)
    kv = row.expand(N, H, T_src, d)
    with pytest.raises(RuntimeError, match=r"2\^24"):
        ops.sparse_attention(q, kv, kv, sel, path="gather")
    torch.cuda.synchronize()


# ---- (c), (d) sessions ------------------------------------------------------------------------------------------------
class Cfg:
    def __init__(self, hidden, heads, max_pos):
        self.hidden_size, self.num_attention_heads, self.max_position_embeddings = hidden, heads, max_pos


def _mask(N, T_dst, T_src, dtype):
    fp_min = torch.finfo(torch.float16).min / 2
    rows = torch.arange(T_src - T_dst, T_src, device=DEV).view(T_dst, 1)
    m = ((torch.arange(T_src, device=DEV).view(1, T_src) > rows) * fp_min).view(1, 1, T_dst, T_src)
    return m.expand(N, 1, T_dst, T_src).contiguous().to(dtype)


def _layer(H, d, k, max_pos, dtype):
    S.seed(42)
    pc = PerlinAttentionConfig(k=k, attention_predictor_length=T_M, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix', use_cache=True)
    layer = PerlinSelfAttention(Cfg(H * d, H, max_pos), pc).to(DEV).to(dtype).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = True
    layer.attention.context_layer_dtype = dtype
    return layer


def _prefix(layer, N, H, d, T0, T, dtype, seed):
    S.seed(seed)
    x = torch.randn((N, H, T, d), device=DEV).to(dtype)
    q = (x.float() * d ** -0.5).to(dtype)
    out = layer(None, None, None, query_layer=q[:, :, :T0], key_layer=x[:, :, :T0], value_layer=x[:, :, :T0],
                attention_mask=_mask(N, T0, T0, dtype))
    return x, q, out.state


def _session_step_columns(sess, T_src, what):
    """The step's selection is the oracle's top-k of the map it returned, its columns (`.col`, and the int64 wire format of
    `.col_indices()`) the oracle's interpolation of that mask for a T_src-long sequence."""
    N, H, k = sess.N, sess.H, sess.k
    csr = sess.csr
    assert csr is not None, what
    probs = sess.probs.reshape(N, H, 1, T_M).float().cpu()
    mask = O.grouped_topk_mask(probs, sess.keep_table[T_src - 1:T_src].cpu())
    assert torch.equal(unpack_bits(csr.bits, H, T_M), mask), (what, "bits")
    crow_o, col_o = oracle_columns(mask, k, T_src, sess.capacity)
    check_columns(csr, crow_o, col_o, what)
    wire = csr.col_indices().cpu()
    for n in range(N):
        z = int(crow_o[n, -1])
        assert torch.equal(wire[n, :z], col_o[n, :z]), (what, "col_indices", n)
    return crow_o, col_o


@pytest.mark.parametrize("fused_attention", [True, False], ids=["fused_attn", "emit_attn"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_session_columns_every_step(use_graph, fused_attention):
    """A prefix that crosses T_M = 256 (pixel widths 1 -> 2): consecutive steps have different columns, and every step's are
    the oracle's -- a graph replay re-arms the captured handle instead of serving the first step's columns."""
    dtype, N, H, d, k, T0, steps = torch.bfloat16, 2, 8, 64, 16, 250, 12
    T = T0 + steps
    layer = _layer(H, d, k, T + 3, dtype)
    with torch.no_grad():
        x, q, state = _prefix(layer, N, H, d, T0, T, dtype, seed=13)
        sess = DecodeSession(layer.attention, state, x[:, :, :T0], x[:, :, :T0], capacity=T + 3, use_graph=use_graph,
                             fused_attention=fused_attention)
        seen = set()
        for i in range(steps):
            hi = T0 + i + 1
            sess.step(q[:, :, hi - 1:hi], x[:, :, hi - 1:hi], x[:, :, hi - 1:hi])
            crow_o, col_o = _session_step_columns(sess, hi, f"step {i}")
            seen.add(tuple(col_o[0, :int(crow_o[0, -1])].tolist()))
        assert len(seen) > steps // 2, "consecutive steps should have different columns"


def test_session_columns_every_step_deeper_cnn(monkeypatch):
    """PERLIN_HOTFIX_OPT_DEEPER=1 (three convolutions): the round-4 launches hand out the step's CSR too."""
    monkeypatch.setenv("PERLIN_HOTFIX_OPT_DEEPER", "1")
    dtype, N, H, d, k, T0, steps = torch.bfloat16, 1, 4, 64, 16, 250, 10
    T = T0 + steps
    layer = _layer(H, d, k, T + 3, dtype)
    with torch.no_grad():
        x, q, state = _prefix(layer, N, H, d, T0, T, dtype, seed=3)
        sess = layer.attention.decode_session(state, x[:, :, :T0], x[:, :, :T0], capacity=T + 3)
        assert not sess.fused_cnn and sess.graph is not None
        for i in range(steps):
            hi = T0 + i + 1
            sess.step(q[:, :, hi - 1:hi], x[:, :, hi - 1:hi], x[:, :, hi - 1:hi])
            _session_step_columns(sess, hi, f"step {i}")


@pytest.mark.parametrize("fused_attention", [True, False], ids=["fused_attn", "emit_attn"])
def test_session_capacity_changes_no_bit(fused_attention):
    """The same prefix continued by a session of capacity T + 3 and one of 2^20 (H = 32: (H - 1) * 2^20 > 2^24; k = 4 over
    ~1100 tokens: thinned pixels): per step bitwise the same context and map, the same columns after re-encoding."""
    dtype, N, H, d, k, T0, steps = torch.bfloat16, 1, 32, 64, 4, 1100, 6
    T, T_big = T0 + steps, 1 << 20
    layer = _layer(H, d, k, T_big, dtype)
    try:
        with torch.no_grad():
            x, q, state = _prefix(layer, N, H, d, T0, T, dtype, seed=21)
            a = DecodeSession(layer.attention, state, x[:, :, :T0], x[:, :, :T0], capacity=T + 3, fused_attention=fused_attention)
            b = DecodeSession(layer.attention, state, x[:, :, :T0], x[:, :, :T0], capacity=T_big, fused_attention=fused_attention)
            for i in range(steps):
                hi = T0 + i + 1
                ca = a.step(q[:, :, hi - 1:hi], x[:, :, hi - 1:hi], x[:, :, hi - 1:hi]).clone()
                cb = b.step(q[:, :, hi - 1:hi], x[:, :, hi - 1:hi], x[:, :, hi - 1:hi]).clone()
                assert torch.isfinite(ca.float()).all()
                assert torch.equal(ca, cb), (i, (ca.float() - cb.float()).abs().max().item())
                assert torch.equal(a.probs, b.probs), i
                _, col_a = _session_step_columns(a, hi, f"capacity {T + 3}, step {i}")
                _, col_b = _session_step_columns(b, hi, f"capacity {T_big}, step {i}")
                z = int(a.csr.crow[0, 1])
                ka, kb_ = col_a[0, :z], col_b[0, :z]
                assert torch.equal((ka // (T + 3)) * T_big + ka % (T + 3), kb_), i
                assert int(kb_.max()) >= (1 << 24)                          # ids past the fp32-exact range
                w = hi / T_M
                assert w > k                                                # thinned pixels
    finally:
        a = b = layer = None
        torch.cuda.empty_cache()
