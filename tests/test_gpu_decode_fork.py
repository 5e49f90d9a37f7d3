"""-m gpu: fork and beam reorder of a paged ragged decode session (`DecodeSession.fork / reorder`, one `sea_decode_fork`
call each).  Forked slots share their source's closed pages and copy its open page; the reference is always a CONTIGUOUS
ragged session that uses no fork code -- seeded with the same prompt in every slot, or `admit`ted with the exported state and
K / V of the source at the same point.  Every step after a move must give the same context rows, estimated probabilities,
CSR row and columns, bit for bit, eagerly launched and graph-replayed; after every move the device block table is the host
mirror, shared pages are closed pages, and the pool's accounting holds."""
import pytest
import torch

import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
from sea_attention_amd.perlin_attention.attention_state import PerlinAttentionState as PS
from sea_attention_amd.perlin_attention.decode import DecodeSession

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_M, K = 256, 16


# ---- helpers (as in test_gpu_decode_paged.py) ----------------------------------------------------------------------------
class Cfg:
    def __init__(self, hidden, heads, max_pos):
        self.hidden_size, self.num_attention_heads, self.max_position_embeddings = hidden, heads, max_pos


def _mask(T, dtype):
    fp_min = torch.finfo(torch.float16).min / 2
    r = torch.arange(T, device=DEV)
    return ((r.view(1, T) > r.view(T, 1)) * fp_min).view(1, 1, T, T).to(dtype)


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


def _prompt(layer, H, d, L, dtype, seed):
    """An N = 1 cached forward over a random prompt of L rows: (state, key_prefix, value_prefix)."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn((1, H, L, d), device=DEV, generator=g).to(dtype)
    q = (x.float() * d ** -0.5).to(dtype)
    out = layer(None, None, None, query_layer=q, key_layer=x, value_layer=x, attention_mask=_mask(L, dtype))
    return out.state, x, x


class Rows:
    """The new rows of the steps: a different random row per slot and step, q = k * d^-0.5, k = v."""

    def __init__(self, N, H, d, dtype, seed):
        self.N, self.H, self.d, self.dtype = N, H, d, dtype
        self.g = torch.Generator(device=DEV).manual_seed(seed)

    def next(self):
        k = torch.randn((self.N, self.H, 1, self.d), device=DEV, generator=self.g).to(self.dtype)
        return (k.float() * self.d ** -0.5).to(self.dtype), k


def _step_both(sess, ref, rows, tag):
    q, k = rows.next()
    got = sess.step(q, k, k).clone()
    want = ref.step(q, k, k)
    assert torch.equal(got, want), (tag, (got.float() - want.float()).abs().max().item())
    assert torch.equal(sess.probs, ref.probs), tag
    assert torch.equal(sess.crow, ref.crow), tag
    cs, cr = sess.csr.col, ref.csr.col                           # (pending: the first read emits)
    for n in range(sess.N):
        nnz = int(ref.crow[n, 1].item())
        assert torch.equal(cs[n, :nnz], cr[n, :nnz]), (tag, n)
    _assert_pages(sess)


def _assert_pages(sess):
    """Device table = host mirror; a shared page is a closed page of every slot that names it, and holds exactly as many
    holders as slots name it; free pages + distinct pages in use = pool."""
    tab = sess.block_table.cpu()
    pr = sess.page_rows
    for n in range(sess.N):
        row = tab[n].tolist()
        assert row[:len(sess.pages[n])] == sess.pages[n] and all(e == -1 for e in row[len(sess.pages[n]):]), n
        L = sess.lengths[n]
        assert -(-L // pr) <= len(sess.pages[n]) <= -(-(L + 1) // pr), n
    named = {}
    for n, row in enumerate(sess.pages):
        assert len(set(row)) == len(row)
        for i, pg in enumerate(row):
            named.setdefault(pg, []).append((n, i))
    for pg, where in named.items():
        assert sess.allocator.holders(pg) == len(where), pg
        if len(where) > 1:
            assert all(i < sess.lengths[n] // pr for n, i in where), (pg, where)      # closed in every holder
    assert sess.shared_pages == sorted(pg for pg, w in named.items() if len(w) > 1)
    assert sess.free_pages + len(named) == sess.allocator.pool_pages


def _assert_same_sequences(sess, ref):
    assert sess.lengths == ref.lengths
    for n in range(sess.N):
        got, want = sess.export_state(n), ref.export_state(n)
        assert torch.equal(got.states[PS.PERFORMER].image, want.states[PS.PERFORMER].image), n
        assert torch.equal(got.states[PS.CNN].rows_c8, want.states[PS.CNN].rows_c8), n
        kp, vp = sess.sequence_kv(n)
        kc, vc = ref.sequence_kv(n)
        assert torch.equal(kp, kc) and torch.equal(vp, vc), n


def _ref_reorder(ref, parents):
    """The parent map on a contiguous session without fork code: export every parent first, then admit."""
    saved = {p: (ref.export_state(p),) + ref.sequence_kv(p) for i, p in enumerate(parents) if p != i}
    for i, p in enumerate(parents):
        if p != i:
            ref.admit(i, *saved[p])


def _chunk(d, dtype):
    return 64 if d == 64 else 32


# (dtype, H, d, page_rows as a multiple of the Performer chunk): every dtype, head size and page size of the paged session
CONFIGS = [(torch.bfloat16, 8, 64, 1), (torch.float16, 8, 64, 2), (torch.bfloat16, 8, 80, 2), (torch.float16, 8, 80, 1),
           (torch.bfloat16, 8, 128, 1), (torch.float16, 8, 128, 2)]
IDS = [f"{str(c[0])[6:]}-d{c[2]}-page{c[3]}chunk" for c in CONFIGS]
GRAPH = pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])


# ---- fork at seeding: N copies of one prompt against a session seeded N times with it ----------------------------------
@GRAPH
@pytest.mark.parametrize("dtype,H,d,mult", CONFIGS, ids=IDS)
def test_fork_at_seeding_equals_copies_of_the_prompt(dtype, H, d, mult, use_graph):
    chunk = _chunk(d, dtype)
    pr = mult * chunk
    LA = 2 * pr - chunk - 2                                     # the steps cross a chunk boundary and a page boundary
    steps = chunk + 4
    capacity = 3 * pr + steps + 16
    layer = _layer(H, d, capacity + 4, dtype)
    with torch.no_grad():
        A = _prompt(layer, H, d, LA, dtype, seed=1)
        others = [_prompt(layer, H, d, L, dtype, seed=2 + i) for i, L in enumerate([40, 3 * pr + 5, 9])]
        ref = DecodeSession.from_sequences(layer.attention, [A] * 4, capacity, use_graph=use_graph)
        sess = DecodeSession.from_sequences(layer.attention, [A] + others, capacity, use_graph=use_graph, page_rows=pr,
                                            pool_pages=4 * (-(-capacity // pr)) + 4)
        captures = getattr(sess, "captures", 0)
        free0 = sess.free_pages
        own = len(sess.pages[0])
        sess.fork(0, [1, 2, 3])
        assert sess.lengths == [LA] * 4
        # the other slots' pages went back; each fork holds A's closed pages and a copy of its open page
        assert sess.shared_pages == sorted(sess.pages[0][:-1])
        assert all(p[:-1] == sess.pages[0][:-1] and p[-1] != sess.pages[0][-1] for p in sess.pages[1:])
        assert sess.free_pages == sess.allocator.pool_pages - (own + 3)
        assert sess.free_pages > free0
        _assert_pages(sess)
        _assert_same_sequences(sess, ref)
        rows = Rows(4, H, d, dtype, seed=5)
        for i in range(steps):
            _step_both(sess, ref, rows, f"step {i}")
        _assert_same_sequences(sess, ref)
    assert getattr(sess, "captures", 0) == captures


# ---- fork mid-decode: at every position of the page --------------------------------------------------------------------
# (first length, steps before the fork): the fork sees L = 2 page_rows (a seeded prefix: an empty open page), 2 page_rows + 1,
# 2 page_rows - 1, and 2 page_rows right after a step that filled a page (no open page: the forks share every page)
WHEN = {"r0": (0, 0), "r1": (-2, 3), "rlast": (-4, 3), "filled": (-3, 3)}


@GRAPH
@pytest.mark.parametrize("when", list(WHEN))
@pytest.mark.parametrize("dtype,H,d,mult", CONFIGS, ids=IDS)
def test_fork_mid_decode_equals_admit_of_the_exported_source(dtype, H, d, mult, when, use_graph):
    chunk = _chunk(d, dtype)
    pr = mult * chunk
    off, before = WHEN[when]
    lengths = [2 * pr + off, 50, pr + 7, 3 * pr - 1]
    after = chunk + 3
    capacity = max(lengths) + before + after + 8
    layer = _layer(H, d, capacity + 4, dtype)
    with torch.no_grad():
        pre = [_prompt(layer, H, d, L, dtype, seed=11 + i) for i, L in enumerate(lengths)]
        ref = DecodeSession.from_sequences(layer.attention, pre, capacity, use_graph=use_graph)
        sess = DecodeSession.from_sequences(layer.attention, pre, capacity, use_graph=use_graph, page_rows=pr,
                                            pool_pages=4 * (-(-capacity // pr)) + 4)
        captures = getattr(sess, "captures", 0)
        rows = Rows(4, H, d, dtype, seed=23)
        for i in range(before):
            _step_both(sess, ref, rows, f"before, step {i}")
        L = sess.lengths[0]
        assert L % pr == {"r0": 0, "r1": 1, "rlast": pr - 1, "filled": 0}[when]
        open_page = L < len(sess.pages[0]) * pr
        assert open_page == (when != "filled")
        sess.fork(0, [2, 3])
        for dst in (2, 3):
            ref.admit(dst, ref.export_state(0), *ref.sequence_kv(0))
        if open_page:
            assert sess.shared_pages == sorted(sess.pages[0][:-1])
        else:                                                   # every page shared, no copy; the next step grows each slot
            assert sess.pages[2] == sess.pages[3] == sess.pages[0] and sess.shared_pages == sorted(sess.pages[0])
        _assert_pages(sess)
        _assert_same_sequences(sess, ref)
        for i in range(after):
            _step_both(sess, ref, rows, f"after, step {i}")
        _assert_same_sequences(sess, ref)
    assert getattr(sess, "captures", 0) == captures


# ---- reorder: beam search's parent maps, repeated -----------------------------------------------------------------------
MAPS = [[0, 1, 2, 3], [1, 0, 2, 3], [1, 2, 0, 3], [0, 0, 0, 0], [3, 3, 1, 0], [2, 0, 1, 1]]


@GRAPH
@pytest.mark.parametrize("dtype,H,d,mult", CONFIGS, ids=IDS)
def test_reorder_equals_export_then_admit(dtype, H, d, mult, use_graph):
    chunk = _chunk(d, dtype)
    pr = mult * chunk
    lengths = [pr - 2, 2 * pr, 9, 3 * pr - 3]
    per_map = 3
    capacity = max(lengths) + 2 * len(MAPS) * per_map + 8
    layer = _layer(H, d, capacity + 4, dtype)
    with torch.no_grad():
        pre = [_prompt(layer, H, d, L, dtype, seed=31 + i) for i, L in enumerate(lengths)]
        ref = DecodeSession.from_sequences(layer.attention, pre, capacity, use_graph=use_graph)
        sess = DecodeSession.from_sequences(layer.attention, pre, capacity, use_graph=use_graph, page_rows=pr,
                                            pool_pages=4 * (-(-capacity // pr)) + 4)
        captures = getattr(sess, "captures", 0)
        rows = Rows(4, H, d, dtype, seed=37)
        for rep in range(2):
            for j, parents in enumerate(MAPS):
                if parents == list(range(4)):
                    pages, free = [list(p) for p in sess.pages], sess.free_pages
                    table = sess.block_table.clone()
                    sess.reorder(parents)                       # identity: nothing moves, nothing is taken
                    assert sess.pages == pages and sess.free_pages == free and torch.equal(sess.block_table, table)
                else:
                    sess.reorder(parents)
                    _ref_reorder(ref, parents)
                _assert_pages(sess)
                _assert_same_sequences(sess, ref)
                for i in range(per_map):
                    _step_both(sess, ref, rows, f"rep {rep}, map {j}, step {i}")
        _assert_same_sequences(sess, ref)
    assert getattr(sess, "captures", 0) == captures


# ---- release after fork: admit into a fork gives back its private pages only -------------------------------------------
@GRAPH
@pytest.mark.parametrize("dtype,H,d,mult", [CONFIGS[0], CONFIGS[5]], ids=[IDS[0], IDS[5]])
def test_admit_into_a_fork_releases_its_private_pages_only(dtype, H, d, mult, use_graph):
    chunk = _chunk(d, dtype)
    pr = mult * chunk
    LA = 3 * pr + 5
    capacity = LA + 4 * chunk
    layer = _layer(H, d, capacity + 4, dtype)
    with torch.no_grad():
        A = _prompt(layer, H, d, LA, dtype, seed=41)
        B = _prompt(layer, H, d, 20, dtype, seed=42)
        ref = DecodeSession.from_sequences(layer.attention, [A] * 4, capacity, use_graph=use_graph)
        sess = DecodeSession.from_sequences(layer.attention, [A, B, B, B], capacity, use_graph=use_graph, page_rows=pr,
                                            pool_pages=16)
        captures = getattr(sess, "captures", 0)
        sess.fork(0, [1, 2, 3])
        rows = Rows(4, H, d, dtype, seed=43)
        for i in range(3):
            _step_both(sess, ref, rows, f"forked, step {i}")
        shared = sess.shared_pages
        private = [pg for pg in sess.pages[2] if pg not in shared]
        assert len(private) == 1 and len(shared) == 3
        free = sess.free_pages
        C = _prompt(layer, H, d, 30, dtype, seed=44)             # one page
        sess.admit(2, *C)
        ref.admit(2, *C)
        assert sess.pages[2] == private                         # its own page, given back, is taken again
        assert sess.shared_pages == shared and sess.free_pages == free
        assert all(sess.allocator.holders(pg) == 3 for pg in shared)
        _assert_pages(sess)
        for i in range(chunk + 2):
            _step_both(sess, ref, rows, f"after admit, step {i}")
        _assert_same_sequences(sess, ref)
        # the last holders let go: the shared pages come free only when the source lets go too
        for slot in (1, 3):
            sess.admit(slot, *C)
        assert sess.shared_pages == []
        assert all(sess.allocator.holders(pg) == 1 for pg in sess.pages[0])
        _assert_pages(sess)
    assert getattr(sess, "captures", 0) == captures


# ---- refusals: nothing changes, and the session decodes on ---------------------------------------------------------------
def _snapshot(sess):
    return ([list(p) for p in sess.pages], list(sess.lengths), sess.free_pages, sess.block_table.clone(), sess.ctr32.clone(),
            sess.image.clone(), sess.x_ring.clone(), sess.y1_ring.clone(), sess.kv_cache.clone(),
            {pg: sess.allocator.holders(pg) for pg in range(sess.allocator.pool_pages)})


def _assert_unchanged(sess, snap):
    now = _snapshot(sess)
    assert now[0] == snap[0] and now[1] == snap[1] and now[2] == snap[2] and now[9] == snap[9]
    for a, b in zip(now[3:9], snap[3:9]):
        assert torch.equal(a, b)


@GRAPH
def test_fork_and_reorder_refusals(use_graph):
    dtype, H, d, pr = torch.bfloat16, 8, 64, 64
    lengths = [70, 130, 20, 200]                               # 2 + 3 + 1 + 4 pages; pool of 12: 2 free
    capacity = 320
    layer = _layer(H, d, capacity + 4, dtype)
    with torch.no_grad():
        pre = [_prompt(layer, H, d, L, dtype, seed=51 + i) for i, L in enumerate(lengths)]
        ref = DecodeSession.from_sequences(layer.attention, pre, capacity, use_graph=use_graph)
        sess = DecodeSession.from_sequences(layer.attention, pre, capacity, use_graph=use_graph, page_rows=pr, pool_pages=12)
        rows = Rows(4, H, d, dtype, seed=53)
        _step_both(sess, ref, rows, "first step")
        snap = _snapshot(sess)
        assert sess.free_pages == 2
        with pytest.raises(RuntimeError, match=r"page pool exhausted: slot\(s\) \[0, 1, 2\]"):
            sess.fork(3, [0, 1, 2])                             # three open-page copies, two free pages
        with pytest.raises(RuntimeError, match=r"slot\(s\) \[0, 2, 3\]"):
            sess.reorder([1, 1, 0, 2])
        with pytest.raises(IndexError):
            sess.fork(4, [0])
        with pytest.raises(IndexError):
            sess.fork(0, [1, -1])
        with pytest.raises(IndexError):
            sess.reorder([0, 1, 2, 4])
        with pytest.raises(ValueError, match="distinct"):
            sess.fork(1, [0, 1])
        with pytest.raises(ValueError, match="distinct"):
            sess.fork(1, [2, 2])
        with pytest.raises(ValueError, match="4 slots"):
            sess.reorder([0, 1, 2])
        _assert_unchanged(sess, snap)
        for i in range(3):
            _step_both(sess, ref, rows, f"after the refusals, step {i}")
        # a fork that fits still goes through afterwards
        sess.fork(1, [2])
        ref.admit(2, ref.export_state(1), *ref.sequence_kv(1))
        _assert_pages(sess)
        _step_both(sess, ref, rows, "after a fork")
        for call in (lambda: ref.fork(0, [1]), lambda: ref.reorder([1, 0, 2, 3])):       # contiguous ragged
            with pytest.raises(ValueError, match="paging is required"):
                call()
        uniform = DecodeSession(layer.attention, pre[0][0], pre[0][1], pre[0][2], capacity, use_graph=False)
        with pytest.raises(ValueError, match="paging is required"):
            uniform.reorder([0])
