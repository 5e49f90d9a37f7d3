"""-m gpu: paged K / V for the ragged decode session (`DecodeSession.from_sequences(..., page_rows=...)`).  The reference is
the contiguous ragged session over the same sequences (test_gpu_decode_ragged.py holds that one to N = 1 sessions): every
step of a paged session must give the same context rows, estimated probabilities, CSR row and columns, bit for bit --
eagerly launched and graph-replayed -- while its K / V live in a shared pool of pages that may be far smaller than
N x capacity rows."""
import pytest
import torch

import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
from sea_attention_amd.perlin_attention.attention_state import PerlinAttentionState as PS
from sea_attention_amd.perlin_attention.decode import DecodeSession

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_M, K = 256, 16


# ---- helpers (copied from test_gpu_decode_ragged.py) -------------------------------------------------------------------
class Cfg:
    def __init__(self, hidden, heads, max_pos):
        self.hidden_size, self.num_attention_heads, self.max_position_embeddings = hidden, heads, max_pos


def _mask(T_dst, T_src, dtype):
    fp_min = torch.finfo(torch.float16).min / 2
    rows = torch.arange(T_src - T_dst, T_src, device=DEV).view(T_dst, 1)
    return ((torch.arange(T_src, device=DEV).view(1, T_src) > rows) * fp_min).view(1, 1, T_dst, T_src).to(dtype)


def _layer(H, d, max_pos, dtype):
    S.seed(42)
    pc = PerlinAttentionConfig(k=K, attention_predictor_length=T_M, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix', use_cache=True)
    layer = PerlinSelfAttention(Cfg(H * d, H, max_pos), pc).to(DEV).to(dtype).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = True
    layer.attention.context_layer_dtype = dtype
    return layer


def _sequences(H, d, lengths, steps, dtype, seed):
    """One (x, q) pair per sequence, (1, H, L_i + steps, d): the prefix and the rows its steps take."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    out = []
    for L in lengths:
        x = torch.randn((1, H, L + steps, d), device=DEV, generator=g).to(dtype)
        out.append((x, (x.float() * d ** -0.5).to(dtype)))
    return out


def _prefill(layer, x, q, L):
    """An N = 1 cached forward over the first L rows: (state, key_prefix, value_prefix)."""
    mask = _mask(L, L, x.dtype).expand(x.shape[0], 1, L, L).contiguous()
    out = layer(None, None, None, query_layer=q[:, :, :L], key_layer=x[:, :, :L], value_layer=x[:, :, :L], attention_mask=mask)
    return out.state, x[:, :, :L], x[:, :, :L]


def _batch_rows(seqs, pos):
    """The step's new rows of every sequence, stacked: q, k (= v), (N, H, 1, d)."""
    q = torch.cat([q[:, :, p:p + 1] for (_x, q), p in zip(seqs, pos)])
    k = torch.cat([x[:, :, p:p + 1] for (x, _q), p in zip(seqs, pos)])
    return q, k


# ---- paged against contiguous -----------------------------------------------------------------------------------------
def _setup(H, d, lengths, steps, capacity, dtype, page_rows, pool_pages=None, use_graph=True, seed=7):
    layer = _layer(H, d, capacity + 4, dtype)
    seqs = _sequences(H, d, lengths, steps, dtype, seed)
    with torch.no_grad():
        pre = [_prefill(layer, x, q, L) for (x, q), L in zip(seqs, lengths)]
        ref = DecodeSession.from_sequences(layer.attention, pre, capacity, use_graph=use_graph)
        sess = DecodeSession.from_sequences(layer.attention, pre, capacity, use_graph=use_graph, page_rows=page_rows,
                                            pool_pages=pool_pages)
    return layer, seqs, pre, ref, sess


def _step_both(sess, ref, seqs, pos, tag, columns=True):
    """One step of both sessions on the same rows; every output bitwise equal."""
    q, k = _batch_rows(seqs, pos)
    got = sess.step(q, k, k).clone()
    want = ref.step(q, k, k)
    assert torch.equal(got, want), (tag, (got.float() - want.float()).abs().max().item())
    assert torch.equal(sess.probs, ref.probs), tag
    assert torch.equal(sess.crow, ref.crow), tag
    if columns:
        cs, cr = sess.csr.col, ref.csr.col                       # (pending: the first read emits)
        for n in range(sess.N):
            nnz = int(ref.crow[n, 1].item())
            assert torch.equal(cs[n, :nnz], cr[n, :nnz]), (tag, n)


def _table_rows(sess):
    tab = sess.block_table.cpu()
    return [tab[n, :len(sess.pages[n])].tolist() for n in range(sess.N)]


def _assert_table(sess):
    """The device table is the host mirror; every page is held by one slot at most; pages + free = pool."""
    rows = _table_rows(sess)
    assert rows == sess.pages
    held = [pg for r in rows for pg in r]
    assert len(held) == len(set(held)) and all(0 <= pg < sess.allocator.pool_pages for pg in held)
    assert len(held) + sess.free_pages == sess.allocator.pool_pages
    for n, L in enumerate(sess.lengths):                         # the rows written (and at most the next one), nothing more
        assert -(-L // sess.page_rows) <= len(sess.pages[n]) <= -(-(L + 1) // sess.page_rows)


def _contiguous(pages):
    return all(b == a + 1 for a, b in zip(pages, pages[1:]))


# lengths: the steps cross page boundaries (multiples of page_rows) and Performer chunk boundaries (64 at d = 64, 32 at
# d = 80 / 128) in different slots at different steps; slot 0 sits at the CNN's reach (8 rows)
CASES = [(torch.bfloat16, 8, 64, 64, [8, 61, 250, 126]),
         (torch.float16, 32, 64, 128, [8, 125, 254, 300, 60, 380, 190, 9]),
         (torch.bfloat16, 40, 64, 64, [8, 254, 189, 62]),
         (torch.bfloat16, 8, 80, 64, [8, 29, 251, 124]),
         (torch.float16, 8, 128, 128, [8, 30, 253, 125]),
         (torch.bfloat16, 32, 128, 64, [8, 28, 190, 59])]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype,H,d,page_rows,lengths", CASES)
def test_paged_rows_equal_contiguous_session(dtype, H, d, page_rows, lengths, use_graph):
    steps = 8
    capacity = max(lengths) + steps + 4
    need = sum(-(-(L + steps + 1) // page_rows) for L in lengths)
    layer, seqs, pre, ref, sess = _setup(H, d, lengths, steps, capacity, dtype, page_rows, pool_pages=need + 2,
                                         use_graph=use_graph)
    assert sess.paged and sess.ragged and (sess.graph is not None) == use_graph
    assert tuple(sess.kv_cache.shape) == (2, need + 2, H, page_rows, d)
    assert tuple(sess.block_table.shape) == (len(lengths), -(-capacity // page_rows))
    _assert_table(sess)
    captures = getattr(sess, "captures", 0)
    with torch.no_grad():
        for i in range(steps):
            _step_both(sess, ref, seqs, [L + i for L in lengths], f"step {i}")
            _assert_table(sess)
    assert sess.lengths == ref.lengths == [L + steps for L in lengths]
    assert getattr(sess, "captures", 0) == captures
    # the slots crossed page boundaries in turn: at least one holds pages that are not consecutive
    assert any(not _contiguous(p) for p in sess.pages), sess.pages
    assert torch.equal(sess.image, ref.image) and torch.equal(sess.win, ref.win)
    for n in range(len(lengths)):
        k_p, v_p = sess.sequence_kv(n)
        k_c, v_c = ref.sequence_kv(n)
        assert k_p.shape == (1, H, sess.lengths[n], d)
        assert torch.equal(k_p, k_c) and torch.equal(v_p, v_c), n
        assert torch.equal(k_c, ref.k_cache[n:n + 1, :, :sess.lengths[n]])


def test_paged_oversubscribed_pool():
    """N = 4 at capacity 1024 in 40 pages of 64 rows (2560 rows for 4096 of contiguous caches)."""
    dtype, H, d, page_rows, steps = torch.bfloat16, 8, 64, 64, 10
    lengths = [509, 600, 316, 701]                                  # 8 + 10 + 5 + 11 = 34 pages seeded, 3 more while stepping
    layer, seqs, pre, ref, sess = _setup(H, d, lengths, steps, 1024, dtype, page_rows, pool_pages=40, seed=11)
    assert sess.kv_cache.shape[1] * page_rows < len(lengths) * 1024
    assert sess.free_pages == 40 - 34
    with torch.no_grad():
        for i in range(steps):
            _step_both(sess, ref, seqs, [L + i for L in lengths], f"step {i}")
            _assert_table(sess)
    assert sess.free_pages == 40 - 37


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_paged_pool_runs_dry_then_admit_frees_pages(use_graph):
    dtype, H, d, page_rows = torch.bfloat16, 8, 64, 64
    lengths = [62, 200, 120]                    # 1 + 4 + 2 = 7 pages; slot 0 needs its 2nd page at row 64 (step 2)
    steps = 8
    layer, seqs, pre, ref, sess = _setup(H, d, lengths, steps, 512, dtype, page_rows, pool_pages=7, use_graph=use_graph,
                                         seed=13)
    captures = getattr(sess, "captures", 0)
    assert sess.free_pages == 0
    with torch.no_grad():
        for i in range(2):
            _step_both(sess, ref, seqs, [L + i for L in lengths], f"step {i}")
        before = (list(sess.lengths), sess.ctr32.clone(), sess.image.clone(), sess.kv_cache.clone(), sess.block_table.clone())
        q, k = _batch_rows(seqs, [L + 2 for L in lengths])
        with pytest.raises(RuntimeError, match=r"slot\(s\) \[0\]"):
            sess.step(q, k, k)
        # refused before any launch: nothing moved
        assert sess.lengths == before[0] and torch.equal(sess.ctr32, before[1])
        assert torch.equal(sess.image, before[2]) and torch.equal(sess.kv_cache, before[3])
        assert torch.equal(sess.block_table, before[4]) and sess.free_pages == 0
        # slot 1 (4 pages) starts over on a prompt of 100 rows (2 pages): two pages come free
        (x_new, q_new), = _sequences(H, d, [100], steps, dtype, seed=97)
        st_new = _prefill(layer, x_new, q_new, 100)
        sess.admit(1, *st_new)
        ref.admit(1, *st_new)
        assert sess.free_pages == 2
        seqs[1] = (x_new, q_new)
        start = [lengths[0] + 2, 100, lengths[2] + 2]
        for i in range(4):
            _step_both(sess, ref, seqs, [p + i for p in start], f"after admit, step {i}")
            _assert_table(sess)
    assert getattr(sess, "captures", 0) == captures


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_paged_admit_reuses_pages(use_graph):
    dtype, H, d, page_rows, steps = torch.bfloat16, 8, 64, 64, 4
    lengths = [8, 200, 262, 63]
    layer, seqs, pre, ref, sess = _setup(H, d, lengths, 2 * steps, 400, dtype, page_rows, pool_pages=16, use_graph=use_graph,
                                         seed=31)
    captures = getattr(sess, "captures", 0)
    with torch.no_grad():
        for i in range(steps):
            _step_both(sess, ref, seqs, [L + i for L in lengths], f"step {i}")
        old = list(sess.pages[2])                                # 5 pages: rows 0 .. 319
        free_before = sess.free_pages
        (x_new, q_new), = _sequences(H, d, [150], steps, dtype, seed=99)
        st_new = _prefill(layer, x_new, q_new, 150)
        sess.admit(2, *st_new)
        ref.admit(2, *st_new)
        assert set(sess.pages[2]) <= set(old) and len(sess.pages[2]) == 3   # its own pages, given back, are taken again
        assert sess.free_pages == free_before + len(old) - 3
        _assert_table(sess)
        seqs[2] = (x_new, q_new)
        start = [L + steps for L in lengths]
        start[2] = 150
        for i in range(steps):
            _step_both(sess, ref, seqs, [p + i for p in start], f"after admit, step {i}")
        for n in range(len(lengths)):
            got, want = sess.export_state(n), ref.export_state(n)
            assert got.seq_len == want.seq_len
            assert torch.equal(got.states[PS.PERFORMER].image, want.states[PS.PERFORMER].image)
            assert torch.equal(got.states[PS.CNN].rows_c8, want.states[PS.CNN].rows_c8)
            kp, vp = sess.sequence_kv(n)
            kc, vc = ref.sequence_kv(n)
            assert torch.equal(kp, kc) and torch.equal(vp, vc), n
    assert getattr(sess, "captures", 0) == captures


def test_paged_admit_refused_when_the_pool_cannot_hold_the_prefix():
    dtype, H, d, page_rows = torch.bfloat16, 8, 64, 64
    lengths = [40, 100]                                          # 1 + 2 pages of 4
    layer, seqs, pre, ref, sess = _setup(H, d, lengths, 2, 512, dtype, page_rows, pool_pages=4, use_graph=False, seed=17)
    (x_new, q_new), = _sequences(H, d, [300], 2, dtype, seed=19)                 # 5 pages: 1 free + 1 of slot 0 is not enough
    with torch.no_grad():
        st_new = _prefill(layer, x_new, q_new, 300)
        pages, image = [list(p) for p in sess.pages], sess.image.clone()
        with pytest.raises(RuntimeError, match="page pool exhausted"):
            sess.admit(0, *st_new)
        assert sess.pages == pages and torch.equal(sess.image, image) and sess.lengths == lengths and sess.free_pages == 1
        _assert_table(sess)
        _step_both(sess, ref, seqs, lengths, "after the refused admit")


def test_paged_refusals():
    dtype, H, d = torch.bfloat16, 8, 64
    layer = _layer(H, d, 300, dtype)
    seqs = _sequences(H, d, [40, 150], 0, dtype, seed=5)
    with torch.no_grad():
        pre = [_prefill(layer, x, q, x.shape[2]) for x, q in seqs]
        with pytest.raises(ValueError, match="fused_attention"):
            DecodeSession.from_sequences(layer.attention, pre, 256, use_graph=False, fused_attention=False, page_rows=64)
        for bad in (48, 32, 0):                                  # not a power of two / below the d = 64 chunk of 64 rows
            with pytest.raises(ValueError, match="page_rows"):
                DecodeSession.from_sequences(layer.attention, pre, 256, use_graph=False, page_rows=bad)
        with pytest.raises(ValueError, match="cannot hold the prefixes"):          # 1 + 3 pages wanted
            DecodeSession.from_sequences(layer.attention, pre, 256, use_graph=False, page_rows=64, pool_pages=3)
        with pytest.raises(ValueError, match="pool_pages goes with page_rows"):
            DecodeSession.from_sequences(layer.attention, pre, 256, use_graph=False, pool_pages=3)
        sess = DecodeSession.from_sequences(layer.attention, pre, 256, use_graph=False)
        assert not sess.paged and sess.free_pages is None
