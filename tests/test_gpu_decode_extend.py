"""-m gpu: `DecodeSession.extend(slot, q, k, v)` -- one slot of a ragged session takes many rows at once, keeping the closed
pages it shares.  The reference is never the code under test: an N = 1 CONTIGUOUS plain session whose slot was `admit`ted with
the state and K / V of the module's cached forward over prefix + suffix (the route that exists without `extend`:
`export_state` + `sequence_kv` + forward + `admit`), then stepped with the same rows.  Every comparison is `torch.equal`:
the context rows `extend` returns, the exported image and window, K / V, lengths, and the context rows, CSR rows and columns of
at least 12 later steps, which cross a Performer chunk boundary and a page boundary.  Eager and graph-replayed; contiguous,
paged (page = 1 and 2 chunks) and multi-token sessions; bf16 and fp16.  No tolerances anywhere."""
import pytest
import torch

from sea_attention_amd.perlin_attention import ops
from sea_attention_amd.perlin_attention.attention_state import PerlinAttentionState as PS
from sea_attention_amd.perlin_attention.decode import DecodeSession
from test_gpu_decode_ragged import _layer, _mask, _prefill, _sequences
from test_gpu_decode_rows import CASES as ROWS_CASES, _assert_slot, _csr_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAPH = pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
SHAPES = [(c[0], c[1], c[2]) for c in ROWS_CASES]               # the (dtype, H, d) of the pause tests
LATER = 12


def _chunk(d):
    return 64 if d == 64 else 32                                 # the Performer chunk (from_sequences' docstring)


class Ref:
    """The N = 1 contiguous plain session one slot is compared with, and the row stream (x, q) both read."""

    def __init__(self, layer, stream, pre, capacity):
        self.layer, self.capacity, (self.x, self.q) = layer, capacity, stream
        self.sess = DecodeSession.from_sequences(layer.attention, [pre], capacity, use_graph=False)

    @property
    def length(self):
        return self.sess.lengths[0]

    def rows(self, s):
        L = self.length
        return self.q[:, :, L:L + s], self.x[:, :, L:L + s]

    def step(self):
        q, k = self.rows(1)
        return self.sess.step(q, k, k)

    def extend(self, s):
        """The existing route: export, the cached forward over the suffix, admit.  Returns the forward's context rows.  A
        suffix that fills the capacity cannot be admitted (`admit` wants room for a step): that reference is a fresh
        contiguous session with room to spare -- its state and K / V do not depend on the capacity, and no step follows."""
        L, sess = self.length, self.sess
        st, T = sess.export_state(0), self.length + s
        fwd = self.layer(None, None, None, query_layer=self.q[:, :, L:T], key_layer=self.x[:, :, :T], value_layer=self.x[:, :, :T],
                         attention_mask=_mask(s, T, self.x.dtype), last_state=st)
        if T < self.capacity:
            sess.admit(0, fwd.state, self.x[:, :, :T], self.x[:, :, :T])
        else:
            self.sess = DecodeSession.from_sequences(self.layer.attention, [(fwd.state, self.x[:, :, :T], self.x[:, :, :T])],
                                                     self.capacity + 8, use_graph=False)
        return fwd.context_layer


def _rig(H, d, dtype, prefixes, rows, capacity, use_graph, none=(), seed=7, same_prompt=False, **kw):
    """A batch session over `prefixes` and a Ref per slot; every stream has prefix + `rows` rows."""
    layer = _layer(H, d, capacity + 16, dtype)
    seqs = _sequences(H, d, prefixes, rows, dtype, seed)
    if same_prompt:                                              # every stream continues slot 0's prompt with rows of its own
        x0, q0 = seqs[0]
        P = prefixes[0]
        seqs = [(torch.cat([x0[:, :, :P], x[:, :, P:]], 2), torch.cat([q0[:, :, :P], q[:, :, P:]], 2)) for x, q in seqs]
    pre = [_prefill(layer, x, q, L) for (x, q), L in zip(seqs, prefixes)]
    sess = DecodeSession.from_sequences(layer.attention, [None if n in none else p for n, p in enumerate(pre)], capacity,
                                        use_graph=use_graph, **kw)
    refs = [None if n in none else Ref(layer, seqs[n], pre[n], capacity) for n in range(len(prefixes))]
    return layer, seqs, pre, sess, refs


def _step(sess, refs, tag):
    """One one-row step of the batch; every slot that takes part against its reference's step."""
    before, out = list(sess.lengths), sess.paused
    q = torch.cat([r.rows(1)[0] if r is not None and not o else torch.full_like(refs[0].q[:, :, :1], float("nan"))
                   for r, o in zip(refs, out)])
    k = torch.cat([r.rows(1)[1] if r is not None and not o else torch.full_like(refs[0].x[:, :, :1], float("nan"))
                   for r, o in zip(refs, out)])
    got = sess.step(q, k, k).clone()
    crow, col = sess.csr.crow.cpu(), sess.csr.col.cpu()
    for n, ref in enumerate(refs):
        if out[n]:
            assert not got[n].any() and crow[n].tolist() == [0, 0] and sess.lengths[n] == before[n], (tag, n)
            continue
        c = ref.step()
        assert torch.equal(got[n:n + 1], c), (tag, n, before[n], (got[n:n + 1].float() - c.float()).abs().max().item())
        z = int(ref.sess.csr.crow[0, 1])
        assert crow[n].tolist() == [0, z], (tag, n, before[n], crow[n].tolist(), z)
        assert torch.equal(col[n, :z], ref.sess.csr.col[0, :z].cpu()), (tag, n, before[n], "columns")
        assert sess.lengths[n] == before[n] + 1 == ref.length, (tag, n)


def _extend(sess, refs, n, s, tag=""):
    """`extend` slot n by its stream's next s rows; the rows and the slot's state against the reference's."""
    ref = refs[n]
    L, pages_before = sess.lengths[n], list(sess.pages[n]) if sess.paged else None
    assert L == ref.length
    q, k = ref.rows(s)
    got = sess.extend(n, q, k, k)
    want = ref.extend(s)
    assert tuple(got.shape) == (1, s, sess.H * sess.D) and got.dtype == want.dtype
    assert torch.equal(got, want), (tag, n, L, s, (got.float() - want.float()).abs().max().item())
    assert sess.lengths[n] == L + s
    _assert_slot(sess, n, ref.sess)
    if sess.paged:
        pr = sess.page_rows
        assert len(sess.pages[n]) == -(-min(L + s + 1, sess.capacity) // pr), (tag, n, L, s, sess.pages[n])
        assert sess.pages[n][:L // pr] == pages_before[:L // pr], (tag, n, "closed pages")
        assert sess.block_table[n].tolist() == sess.pages[n] + [-1] * (sess.block_table.shape[1] - len(sess.pages[n])), (tag, n)
    return got


def _plan(C, pr):
    """(length before the call, suffix rows) per slot.  pr: the page (a contiguous session: one chunk, for the lengths only)."""
    return [(9, 1),                               # one row
            (C + 5, C - 11),                      # below a chunk: to 2C - 6, so that the later steps complete the chunk (and a page)
            (2 * C + 9, C - 9),                   # exactly to a chunk boundary, 3C (a page boundary at page = chunk only)
            (pr + 11, pr - 11),                   # exactly to a page boundary, 2 pages: the next step opens a page
            (pr - 2, 2 * pr + 7),                 # crosses three page boundaries; more rows than both rings hold
            (2 * pr, 5)]                          # stands ON a page boundary before the call: the slot has no open page


# ---- 1. every kind of suffix, every kind of session -----------------------------------------------------------------------
LAYOUTS = {None: "contiguous", 1: "page=chunk", 2: "page=2chunk", "rows8": "max_step_rows"}
SESSIONS = [(*shape, pages) for shape in SHAPES for pages in (None, 1, 2)] + [(*SHAPES[0], "rows8"), (*SHAPES[4], "rows8")]


@GRAPH
@pytest.mark.parametrize("dtype,H,d,pages", SESSIONS, ids=[f"{str(c[0])[6:]}-{c[1]}-{c[2]}-{LAYOUTS[c[3]]}" for c in SESSIONS])
def test_extend_is_bitwise_the_admitted_reference(dtype, H, d, pages, use_graph):
    C = _chunk(d)
    pr = C * (pages if isinstance(pages, int) else 1)
    plan = _plan(C, pr)
    capacity = max(L + s for L, s in plan) + LATER + 4
    fill = (capacity - 20, 20)                                   # a suffix that fills the capacity
    plan.append(fill)
    N = len(plan)
    kw = dict(page_rows=pr) if isinstance(pages, int) else dict(max_step_rows=8) if pages == "rows8" else {}
    rows8 = pages == "rows8"
    with torch.no_grad():
        # every slot starts one row short and takes one step first: slot 5 FILLS its page by it (the slot that "has none"), and
        # the step leaves pending columns behind, which `extend` emits before the counters move
        layer, seqs, pre, sess, refs = _rig(H, d, dtype, [L - 1 for L, _ in plan], capacity, capacity, use_graph, **kw)
        assert C == ops.performer_chunk_rows(d, layer.attention.performer.projection_matrix.shape[0], dtype)
        if rows8:
            q = torch.cat([r.rows(1)[0] for r in refs])
            k = torch.cat([r.rows(1)[1] for r in refs])
            sess.step(q, k, k)
            for r in refs:
                r.step()
        else:
            _step(sess, refs, "first")
        assert sess.lengths == [L for L, _ in plan]
        if sess.paged:
            assert len(sess.pages[5]) == 2 and sess.lengths[5] == 2 * pr        # no open page
        caps = getattr(sess, "captures", 0)
        sess.pause([0, 3])                                       # a paused slot is extended as a paused slot
        for n, (L, s) in enumerate(plan):
            _extend(sess, refs, n, s)
            assert sess.paused == [m in (0, 3) for m in range(N)] and sess.empty == [False] * N
        assert sess.lengths == [L + s for L, s in plan] and sess.lengths[N - 1] == capacity
        sess.resume([0, 3])
        q, k = torch.cat([r.rows(1)[0] for r in refs]), torch.cat([r.rows(1)[1] for r in refs])
        with pytest.raises(RuntimeError, match=rf"capacity {capacity} reached by slot\(s\) \[{N - 1}\]"):
            sess.step(q, k, k)
        sess.pause([N - 1])                                      # the full slot sits out from here on
        crossed_chunk = crossed_page = False
        if rows8:
            for i in range(LATER // 2):                          # two rows per step; the references one row at a time
                before = list(sess.lengths)
                q = torch.cat([r.rows(2)[0] for r in refs[:-1]] + [torch.full_like(refs[0].q[:, :, :2], float("nan"))])
                k = torch.cat([r.rows(2)[1] for r in refs[:-1]] + [torch.full_like(refs[0].x[:, :, :2], float("nan"))])
                got = sess.step(q, k, k).clone()
                rows_csr = _csr_rows(sess, 2)
                for n, ref in enumerate(refs[:-1]):
                    for j in range(2):
                        c = ref.step()
                        assert torch.equal(got[n, j], c[0, 0]), ("rows", i, n, j)
                        z = int(ref.sess.csr.crow[0, 1])
                        assert torch.equal(rows_csr[n][j], ref.sess.csr.col[0, :z].cpu()), ("rows CSR", i, n, j)
                    crossed_chunk |= (before[n] + 2) // C > before[n] // C
        else:
            for i in range(LATER):
                before = list(sess.lengths)
                _step(sess, refs, f"later {i}")
                crossed_chunk |= any((L + 1) % C == 0 for L in before[:-1])
                crossed_page |= any(L % pr == 0 for L in before[:-1])       # that step's row opened a page
            assert crossed_page
        assert crossed_chunk
        for n, ref in enumerate(refs):
            _assert_slot(sess, n, ref.sess)
        assert getattr(sess, "captures", 0) == caps + (1 if rows8 and use_graph else 0)   # (the two-row graph; none for extend)
        if rows8:
            sess.extend(0, *(refs[0].rows(3)[i] for i in (0, 1, 1)))
            with pytest.raises(ValueError, match="no step to undo"):      # an extend ends the chance to rewind
                sess.rewind([0] * N)


# ---- 2. the parked prompt: fork, extend each copy, resume -----------------------------------------------------------------
def test_page_arithmetic_of_the_parked_prompt():
    """The issue's example on the CPU: P = 4000, 64-row pages, seven copies extended by 200 rows each."""
    P, pr, s, copies = 4000, 64, 200, 7
    closed = P // pr
    extended = closed + 1 + copies * (-(-(P + s + 1) // pr) - closed)
    admitted = -(-(P + 1) // pr) + copies * -(-(P + s + 1) // pr)
    assert (closed, extended, admitted) == (62, 91, 525)


@GRAPH
@pytest.mark.parametrize("dtype,H,d", [(torch.bfloat16, 8, 64), (torch.float16, 8, 128)])
def test_parked_prompt_fork_extend_resume(dtype, H, d, use_graph):
    P, pr, N = 200, 64, 4
    suffix = {1: 1, 2: 70, 3: 30}                                # one row; across the page boundary at 256; inside the open page
    capacity = P + max(suffix.values()) + LATER + 4
    with torch.no_grad():
        layer, seqs, pre, sess, refs = _rig(H, d, dtype, [P] * N, capacity, capacity, use_graph, none=(1, 2, 3), same_prompt=True,
                                            page_rows=pr)
        pool = sess.allocator.pool_pages
        caps = getattr(sess, "captures", 0)
        sess.pause(0)
        closed = list(sess.pages[0][:P // pr])
        assert len(closed) == 3 and len(sess.pages[0]) == 4
        prompt_pages, prompt = list(sess.pages[0]), sess.export_state(0)
        prompt_kv = sess.sequence_kv(0)
        sess.fork(0, [1, 2, 3])
        for n, s in suffix.items():
            refs[n] = Ref(layer, seqs[n], pre[0], capacity)
            _extend(sess, refs, n, s, "copy")
            assert sess.pages[n][:3] == closed
        assert sess.paused == [True] * N
        sess.resume([1, 2, 3])
        # shared: exactly the prompt's closed pages; held: those, slot 0's open page, and each copy's own pages from the open
        # index on -- ceil((P + s + 1) / page_rows) - closed: 1 + 2 + 1 (201 -> 4 pages, 270 -> 5, 230 -> 4)
        assert sess.shared_pages == sorted(closed)
        own = {n: -(-(P + s + 1) // pr) - len(closed) for n, s in suffix.items()}
        assert own == {1: 1, 2: 2, 3: 1}
        assert sess.free_pages == pool - (len(closed) + 1 + sum(own.values())) == pool - 8
        assert all(sess.allocator.holders(pg) == N for pg in closed)
        for i in range(LATER):
            _step(sess, refs, f"copies {i}")
        assert sess.lengths == [P] + [P + s + LATER for s in suffix.values()]
        assert sess.shared_pages == sorted(closed)
        own = {n: -(-(P + s + LATER + 1) // pr) - len(closed) for n, s in suffix.items()}
        assert sess.free_pages == pool - (len(closed) + 1 + sum(own.values()))
        for n in suffix:
            _assert_slot(sess, n, refs[n].sess)
        # slot 0 is still the prompt: pages, export and K / V untouched
        assert sess.pages[0] == prompt_pages and sess.paused[0]
        now = sess.export_state(0)
        assert torch.equal(now.states[PS.PERFORMER].image, prompt.states[PS.PERFORMER].image)
        assert torch.equal(now.states[PS.CNN].rows_c8, prompt.states[PS.CNN].rows_c8)
        assert all(torch.equal(a, b) for a, b in zip(sess.sequence_kv(0), prompt_kv))
        _assert_slot(sess, 0, refs[0].sess)
        assert getattr(sess, "captures", 0) == caps


# ---- 3. the other slots keep every bit --------------------------------------------------------------------------------------
def _buffers(sess):
    out = dict(image=sess.image, x_ring=sess.x_ring, y1_ring=sess.y1_ring, ctr32=sess.ctr32, kv_cache=sess.kv_cache)
    if sess.paged:
        out["block_table"] = sess.block_table
    return {k: v.clone() for k, v in out.items()}


def _host(sess):
    state = [list(sess.lengths), sess.paused, sess.empty, getattr(sess, "captures", 0)]
    if sess.paged:
        alloc = sess.allocator
        state += [[list(p) for p in sess.pages], list(alloc._free), dict(alloc._holders)]
    return state


@GRAPH
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_every_other_slot_is_bitwise_what_it_was(paged, use_graph):
    dtype, H, d, pr = torch.bfloat16, 8, 64, 64
    prefixes, capacity, slot, s = [60, 100, 130, 40], 330, 1, 150
    with torch.no_grad():
        layer, seqs, pre, sess, refs = _rig(H, d, dtype, prefixes, 160, capacity, use_graph, none=(3,),
                                            **(dict(page_rows=pr) if paged else {}))
        for i in range(3):
            _step(sess, refs, f"warm {i}")
        sess.pause([2])
        before = _buffers(sess)
        L = sess.lengths[slot]
        old_pages = list(sess.pages[slot]) if paged else None
        _extend(sess, refs, slot, s)
        after = _buffers(sess)
        N = sess.N
        others = [n for n in range(N) if n != slot]
        for name in ("x_ring", "y1_ring", "ctr32") + (("block_table",) if paged else ()):
            assert torch.equal(after[name][others], before[name][others]), name
        assert torch.equal(after["image"].view(N, -1)[others], before["image"].view(N, -1)[others])
        assert after["ctr32"][slot].tolist() == [L + s, L + s + 1, L + s]
        if paged:
            mine = set(sess.pages[slot][L // pr:])               # the open page and the new ones: all `extend` may write
            rest = [pg for pg in range(sess.allocator.pool_pages) if pg not in mine]
            assert torch.equal(after["kv_cache"][:, rest], before["kv_cache"][:, rest])
            assert sess.pages[slot][:len(old_pages)] == old_pages
            assert after["block_table"][slot, :len(old_pages)].tolist() == old_pages
            o = sess.pages[slot][L // pr]                        # the open page: its rows below L stay
            assert torch.equal(after["kv_cache"][:, o, :, :L % pr], before["kv_cache"][:, o, :, :L % pr])
        else:
            assert torch.equal(after["kv_cache"][:, others], before["kv_cache"][:, others])
            assert torch.equal(after["kv_cache"][:, slot, :, :L], before["kv_cache"][:, slot, :, :L])
        sess.resume([2])
        for i in range(3):
            _step(sess, refs, f"after {i}")
        for n in range(3):
            _assert_slot(sess, n, refs[n].sess)


# ---- 4. refusals change nothing -----------------------------------------------------------------------------------------------
@GRAPH
def test_refusals_change_nothing(use_graph):
    dtype, H, d, pr = torch.bfloat16, 8, 64, 64
    prefixes, capacity = [60, 100, 40], 300
    with torch.no_grad():
        layer, seqs, pre, sess, refs = _rig(H, d, dtype, prefixes, 210, capacity, use_graph, none=(2,), page_rows=pr, pool_pages=5)
        _step(sess, refs, "first")
        q, k = refs[0].rows(4)

        def refused(exc, match, *args):
            bufs, host = _buffers(sess), _host(sess)
            with pytest.raises(exc, match=match):
                sess.extend(*args)
            now = _buffers(sess)
            assert all(torch.equal(now[name], bufs[name]) for name in bufs), (match, [n for n in bufs if not torch.equal(now[n], bufs[n])])
            assert _host(sess) == host, match

        refused(ValueError, "slot 2 is empty", 2, q, k, k)
        refused(IndexError, "slot 3 outside", 3, q, k, k)
        refused(IndexError, "slot -1 outside", -1, q, k, k)
        refused(ValueError, r"\(1, 8, s, 64\)", 0, torch.cat([q, q]), torch.cat([k, k]), torch.cat([k, k]))    # N = 2
        refused(ValueError, r"\(1, 8, s, 64\)", 0, q[..., :32], k[..., :32], k[..., :32])
        refused(ValueError, r"\(1, 8, s, 64\)", 0, q, k[:, :, :3], k)
        refused(ValueError, r"\(1, 8, s, 64\)", 0, q[:, :, :0], k[:, :, :0], k[:, :, :0])                        # s = 0
        refused(ValueError, r"\(1, 8, s, 64\)", 0, q[0], k[0], k[0])
        refused(ValueError, "torch.bfloat16 rows on cuda", 0, q.float(), k.float(), k.float())
        refused(ValueError, "torch.bfloat16 rows on cuda", 0, q.half(), k.half(), k.half())
        refused(ValueError, "torch.bfloat16 rows on cuda", 0, q.cpu(), k.cpu(), k.cpu())
        big = refs[1].rows(capacity - sess.lengths[1] + 1)
        refused(ValueError, r"pass the capacity of 300", 1, big[0], big[1], big[1])
        # the pool: 5 pages, slot 0 holds 1 and slot 1 two; 61 + 140 rows want ceil(202 / 64) = 4 pages, 3 new ones of 2 free
        assert sess.free_pages == 2
        many = refs[0].rows(140)
        refused(RuntimeError, r"page pool exhausted: slot 0 needs 3 new page\(s\)", 0, many[0], many[1], many[1])
        # a shared open page (no supported path leads here: `fork` gives every copy an open page of its own)
        open_page = sess.pages[0][sess.lengths[0] // pr]
        sess.allocator.share([open_page])
        refused(RuntimeError, rf"open page {open_page} has other holders", 0, q, k, k)
        sess.allocator.give_back([open_page])
        caps = getattr(sess, "captures", 0)
        for s in (4, 1, 60):                                     # and what is allowed goes through, without a capture
            _extend(sess, refs, 0, s)
        assert getattr(sess, "captures", 0) == caps == (1 if use_graph else 0)
        assert sess.free_pages == 1                              # 126 rows: 2 pages
        for i in range(3):
            _step(sess, refs, f"after {i}")
        uni = DecodeSession(layer.attention, *pre[0], capacity=80, use_graph=False)
        with pytest.raises(ValueError, match="ragged"):
            uni.extend(0, q, k, k)
