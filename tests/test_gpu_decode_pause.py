"""-m gpu: decode slots that sit out steps (`DecodeSession.pause` / `resume` / `release`, `None` entries of `from_sequences`).
The oracle is the session that already exists: for a schedule of steps with pauses, slot n of the batch session must be
bitwise (`torch.equal`) an N = 1 plain `from_sequences` session of the same prefix that is stepped only at the steps where
slot n took part -- context rows, CSR rows and columns, lengths, exported image and window, K / V, and every later step.
A slot that sits out is fed NaN rows throughout (nothing may read them), returns zeros and an empty CSR row, and costs no
capture.  Eager and graph-replayed; contiguous, paged and multi-token sessions.  No tolerances anywhere."""
import random

import pytest
import torch

from sea_attention_amd.perlin_attention import ops
from sea_attention_amd.perlin_attention.decode import DecodeSession
from test_gpu_decode_ragged import CASES, _layer, _prefill, _sequences
from test_gpu_decode_rows import CASES as ROWS_CASES, SCHEDULE, _assert_slot, _csr_rows

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRAPH = pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
# (H, d) of the existing cases (d = 64 / 80 / 128, one H = 40, both dtypes) with the multi-token tests' lengths: 8 = the CNN's
# reach, a slot just below a Performer chunk boundary (= a page boundary at page_rows = chunk), either side of T_src = 256 / 512
assert [(c[0], c[1], c[2]) for c in CASES] == [(c[0], c[1], c[2]) for c in ROWS_CASES]
SHAPES = ROWS_CASES


def _chunk(layer, d, dtype):
    return ops.performer_chunk_rows(d, layer.attention.performer.projection_matrix.shape[0], dtype)


class Rig:
    """A batch session and, per slot, the N = 1 plain session (`ref`) and the row stream (`seq`) it is compared with."""

    def __init__(self, H, d, lengths, rows, dtype, use_graph, none=(), seed=7, capacity=None, **kw):
        self.H, self.d, self.dtype, self.use_graph = H, d, dtype, use_graph
        self.capacity = capacity or max(lengths) + rows + 4
        self.layer = _layer(H, d, self.capacity + 4, dtype)
        self.seqs = _sequences(H, d, lengths, rows, dtype, seed)
        with torch.no_grad():
            self.pre = [_prefill(self.layer, x, q, L) for (x, q), L in zip(self.seqs, lengths)]
            self.sess = DecodeSession.from_sequences(self.layer.attention, [None if n in none else p for n, p in enumerate(self.pre)],
                                                     self.capacity, use_graph=use_graph, **kw)
            self.refs = [None if n in none else self.plain(p) for n, p in enumerate(self.pre)]

    def plain(self, pre):
        return DecodeSession.from_sequences(self.layer.attention, [pre], self.capacity, use_graph=False)

    def captures(self):
        return getattr(self.sess, "captures", 0)

    def rows(self, s=1):
        """The s new rows of every slot from its own position; NaN for the slots that sit out."""
        sess = self.sess
        q = torch.cat([qq[:, :, L:L + s] for (_x, qq), L in zip(self.seqs, sess.lengths)]).clone()
        k = torch.cat([x[:, :, L:L + s] for (x, _q), L in zip(self.seqs, sess.lengths)]).clone()
        for n, out in enumerate(sess.paused):
            if out:
                q[n], k[n] = float("nan"), float("nan")
        return q, k

    def step(self, tag=""):
        """One step of the batch session; the slots that take part against their references, the others zeros / empty."""
        sess = self.sess
        out, before = sess.paused, list(sess.lengths)
        assert all(o for o, e in zip(out, sess.empty) if e), "an empty slot sits out"
        q, k = self.rows()
        got = sess.step(q, k, k).clone()
        crow, col = sess.csr.crow.cpu(), sess.csr.col.cpu()
        for n in range(sess.N):
            if out[n]:
                assert not got[n].any() and not torch.isnan(got[n]).any(), (tag, n, "context of a sitting-out slot")
                assert crow[n].tolist() == [0, 0], (tag, n, crow[n].tolist())
                assert sess.lengths[n] == before[n], (tag, n)
                continue
            x, qq = self.seqs[n]
            L, ref = before[n], self.refs[n]
            c = ref.step(qq[:, :, L:L + 1], x[:, :, L:L + 1], x[:, :, L:L + 1])
            assert torch.equal(got[n:n + 1], c), (tag, n, L, (got[n:n + 1].float() - c.float()).abs().max().item())
            z = int(ref.csr.crow[0, 1])
            assert crow[n].tolist() == [0, z], (tag, n, L, crow[n].tolist(), z)
            assert torch.equal(col[n, :z], ref.csr.col[0, :z].cpu()), (tag, n, L, "columns")
            assert sess.lengths[n] == L + 1 == ref.lengths[0], (tag, n)
        return got

    def check_slots(self):
        for n, ref in enumerate(self.refs):
            if not self.sess.empty[n]:
                _assert_slot(self.sess, n, ref)


# ---- 1. a schedule of pauses and resumes ----------------------------------------------------------------------------------
@GRAPH
@pytest.mark.parametrize("pages", [None, 1, 2], ids=["contiguous", "page=chunk", "page=2chunk"])
@pytest.mark.parametrize("dtype,H,d,lengths", SHAPES)
def test_schedule_of_pauses_is_bitwise_the_single_sessions(dtype, H, d, lengths, pages, use_graph):
    steps, rng = 40, random.Random(1234)
    N = len(lengths)
    C = 64 if d == 64 else 32                                    # the Performer chunk (from_sequences' docstring)
    kw = {} if pages is None else dict(page_rows=pages * C)
    rig = Rig(H, d, lengths, steps, dtype, use_graph, **kw)
    sess = rig.sess
    assert C == _chunk(rig.layer, d, dtype)
    # b: the slot closest below a chunk boundary (a page boundary too at page_rows = chunk); it is paused when it stands ON it
    b = min(range(N), key=lambda n: C - lengths[n] % C)
    to_boundary = C - lengths[b] % C
    assert b != 0 and to_boundary <= 8
    others = [n for n in range(N) if n not in (0, b)]
    hold_b = range(to_boundary, to_boundary + 6)                 # steps b sits out, standing on its boundary
    all_out = range(22, 25)                                      # a stretch with every slot paused
    want = {0}                                                   # slot 0 sits out the very first step
    caps = None
    with torch.no_grad():
        for i in range(steps):
            if i == 3:
                want.discard(0)
            if i == to_boundary:
                assert sess.lengths[b] % C == 0
                want |= {b, others[0]}
            if i == to_boundary + 6:
                want -= {b, others[0]}                           # two resumed in the same call
            if i in all_out:
                now = set(range(N))
            else:
                if i > to_boundary + 6 and rng.random() < 0.4:   # seeded random toggles (never everybody: that is the stretch)
                    n = rng.randrange(N)
                    want ^= {n}
                    if len(want) == N:
                        want.discard(n)
                now = set(want)
            cur = {n for n, p in enumerate(sess.paused) if p}
            if now - cur:
                sess.pause(sorted(now - cur))
            if cur - now:
                sess.resume(sorted(cur - now))
            assert sess.paused == [n in now for n in range(N)] and sess.empty == [False] * N
            if i in hold_b:
                assert sess.paused[b]
            free = sess.free_pages
            rig.step(f"step {i}")
            if i in all_out:
                assert sess.free_pages == free and sess.lengths == [r.lengths[0] for r in rig.refs]
            if i == 0:
                caps = rig.captures()
        assert rig.captures() == caps == (1 if use_graph else 0)
        assert all(r.lengths[0] > L for r, L in zip(rig.refs, lengths)), "every slot took part in some steps"
        rig.check_slots()
        sess.resume(range(N))
        rig.step("everybody again")
        rig.check_slots()


# ---- 2. pool accounting ---------------------------------------------------------------------------------------------------
@GRAPH
def test_a_paused_slot_takes_no_page_and_release_returns_the_unshared_ones(use_graph):
    dtype, H, d, pr = torch.bfloat16, 8, 64, 64
    lengths = [60, 100, 126]                                     # pages of the prefixes (+ the next row): 1 + 2 + 2
    rig = Rig(H, d, lengths, 24, dtype, use_graph, page_rows=pr, pool_pages=6)
    sess = rig.sess
    with torch.no_grad():
        assert sess.free_pages == 1
        for i in range(4):                                       # slot 2 opens its third page at 128: the pool is used up
            rig.step(f"fill {i}")
        assert sess.free_pages == 0 and sess.lengths == [64, 104, 130]
        sess.pause([0])                                          # slot 0 stands on a page boundary: its next row needs a page
        for i in range(10):                                      # ... which nobody takes while it sits out
            rig.step(f"paused at the boundary {i}")
            assert sess.free_pages == 0 and len(sess.pages[0]) == 1
        sess.resume([0])                                         # the parent's behaviour: every slot steps, the pool is exhausted
        state = (list(sess.lengths), [list(p) for p in sess.pages])
        q, k = rig.rows()
        with pytest.raises(RuntimeError, match=r"page pool exhausted: slot\(s\) \[0\]"):
            sess.step(q, k, k)
        assert (sess.lengths, sess.pages) == state and sess.paused == [False] * 3
        sess.pause([0])
        rig.step("after the refusal")
        mine = list(sess.pages[2])
        assert sess.shared_pages == [] and len(mine) == 3
        sess.release([2])
        assert sess.free_pages == 3 and sess.pages[2] == [] and sess.empty == [False, False, True]
        assert all(sess.allocator.holders(pg) == 0 for pg in mine)
        sess.resume([0])
        rig.step("slot 0 grows into a returned page")
        assert sess.free_pages == 2 and len(sess.pages[0]) == 2
        rig.check_slots()


# ---- 3. a full slot does not stop the batch -------------------------------------------------------------------------------
@GRAPH
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
def test_a_full_slot_that_is_paused_does_not_stop_the_batch(paged, use_graph):
    dtype, H, d = torch.float16, 8, 128
    lengths = [8, 30, 20]
    rig = Rig(H, d, lengths, 12, dtype, use_graph, capacity=34, **(dict(page_rows=32) if paged else {}))
    sess = rig.sess
    with torch.no_grad():
        for i in range(4):
            rig.step(f"fill {i}")
        assert sess.lengths[1] == sess.capacity
        q, k = rig.rows()
        with pytest.raises(RuntimeError, match=r"cache capacity 34 reached by slot\(s\) \[1\]"):
            sess.step(q, k, k)
        sess.pause([1])
        for i in range(5):
            rig.step(f"the others go on {i}")
        sess.resume([1])
        q, k = rig.rows()
        with pytest.raises(RuntimeError, match=r"cache capacity 34 reached by slot\(s\) \[1\]"):
            sess.step(q, k, k)
        sess.pause([1])
        rig.step("and on")
        rig.check_slots()


# ---- 4. a parked prompt -----------------------------------------------------------------------------------------------------
@GRAPH
@pytest.mark.parametrize("dtype,H,d", [(torch.bfloat16, 8, 64), (torch.bfloat16, 8, 80)])
def test_parked_prompt_is_forked_from_as_requests_arrive(dtype, H, d, use_graph):
    L, pr, N, steps = 150, 64, 4, 12
    rig = Rig(H, d, [L] * N, steps, dtype, use_graph, none=(1, 2, 3), page_rows=pr)
    sess = rig.sess
    prompt = rig.pre[0]
    # every sample continues the PROMPT with rows of its own: slot n's stream is the prompt's prefix + its own new rows
    x0, q0 = rig.seqs[0]
    rig.seqs = [(torch.cat([x0[:, :, :L], x[:, :, L:]], 2), torch.cat([q0[:, :, :L], q[:, :, L:]], 2)) for x, q in rig.seqs]
    with torch.no_grad():
        assert sess.empty == [False, True, True, True] and sess.paused == [False, True, True, True]
        caps = rig.captures()
        sess.pause(0)                                            # parked: no step moves it
        closed = sorted(sess.pages[0][:L // pr])
        sess.fork(0, [1, 2])
        assert sess.paused == [True, True, True, True] and sess.empty == [False, False, False, True]
        sess.resume([1, 2])
        rig.refs[1], rig.refs[2] = rig.plain(prompt), rig.plain(prompt)
        for i in range(5):
            rig.step(f"two samples {i}")
        assert sess.shared_pages == closed                       # the prompt's closed pages, held once
        sess.fork(0, [3])
        sess.resume([3])
        rig.refs[3] = rig.plain(prompt)
        for i in range(5):
            rig.step(f"three samples {i}")
        assert sess.shared_pages == closed and sess.lengths == [L, L + 10, L + 10, L + 5]
        assert rig.captures() == caps
        rig.refs[0] = rig.plain(prompt)                          # slot 0 is still the prompt
        rig.check_slots()
        held = {pg for row in sess.pages for pg in row}
        assert sess.free_pages == sess.allocator.pool_pages - len(held)
        sess.release([1, 2, 3])
        assert sess.shared_pages == [] and sess.free_pages == sess.allocator.pool_pages - len(sess.pages[0])
        _assert_slot(sess, 0, rig.refs[0])
        sess.release(0)
        assert sess.free_pages == sess.allocator.pool_pages and sess.empty == [True] * N
        rig.step("nobody home")


# ---- 5. empty slots and admit -----------------------------------------------------------------------------------------------
@GRAPH
@pytest.mark.parametrize("paged", [False, True], ids=["contiguous", "paged"])
@pytest.mark.parametrize("dtype,H,d,lengths", [SHAPES[0], SHAPES[2], SHAPES[4]])
def test_empty_slots_and_admit(dtype, H, d, lengths, paged, use_graph):
    rig = Rig(H, d, lengths, 16, dtype, use_graph, none=(1, 3), **(dict(page_rows=64) if paged else {}))
    sess, streams = rig.sess, list(rig.seqs)
    with torch.no_grad():
        assert sess.empty == [False, True, False, True] and sess.lengths[1] == 0
        for i in range(3):
            rig.step(f"two empty {i}")
        caps = rig.captures()
        assert caps == (1 if use_graph else 0)
        sess.admit(1, *rig.pre[1])
        rig.refs[1] = rig.plain(rig.pre[1])
        assert sess.empty == [False, False, False, True] and sess.paused == [False, False, False, True]
        for i in range(4):
            rig.step(f"admitted {i}")
        rig.check_slots()
        sess.release([1])
        assert sess.empty[1] and sess.lengths[1] == 0
        rig.step("released")
        sess.admit(1, *rig.pre[3])                               # another sequence into the released slot
        rig.seqs[1], rig.refs[1] = streams[3], rig.plain(rig.pre[3])
        sess.pause([0])
        sess.admit(0, *rig.pre[1])                               # an admit into a paused slot makes it active too
        rig.seqs[0], rig.refs[0] = streams[1], rig.plain(rig.pre[1])
        assert sess.paused == [False, False, False, True]
        for i in range(4):
            rig.step(f"admitted again {i}")
        assert rig.captures() == caps
        rig.check_slots()


# ---- 6. multi-token sessions ------------------------------------------------------------------------------------------------
@GRAPH
@pytest.mark.parametrize("dtype,H,d,lengths", SHAPES)
def test_multi_token_steps_and_rewind_with_paused_slots(dtype, H, d, lengths, use_graph):
    rows = sum(s for s, _ in SCHEDULE) + 8
    rig = Rig(H, d, lengths, rows, dtype, use_graph, none=(0,), max_step_rows=8)
    sess, rng, N = rig.sess, random.Random(99), len(lengths)
    with torch.no_grad():
        for it, (s, mode) in enumerate(SCHEDULE):
            live = [n for n in range(N) if not sess.empty[n]]
            if it == 0:
                sess.pause([1])                                  # paused for the very first step
            elif it == 4:
                sess.pause(live)                                 # everybody sits out an 8-row step
            else:
                sess.resume(live)
                out = [n for n in live if rng.random() < 0.4]
                sess.pause(out[:len(live) - 1])
            paused, before = sess.paused, list(sess.lengths)
            q, k = rig.rows(s)
            got = sess.step(q, k, k).clone()
            assert tuple(got.shape) == (N, s, H * d)
            rows_csr = _csr_rows(sess, s)
            for n in range(N):
                if paused[n]:
                    assert not got[n].any() and not torch.isnan(got[n]).any() and all(r.numel() == 0 for r in rows_csr[n]), (it, n)
            drop = [0 if paused[n] else (s if mode == "all" else 0 if mode == "none" else rng.choice([0, s, rng.randint(0, s)]))
                    for n in range(N)]
            sat = [n for n in range(N) if paused[n]]
            if sat:                                              # a slot that sat out has nothing to drop: refused, nothing changed
                bad = list(drop)
                bad[sat[0]] = 1
                with pytest.raises(ValueError, match="sat out"):
                    sess.rewind(bad)
                assert sess.lengths == [L if p else L + s for L, p in zip(before, paused)]
            sess.rewind(drop)
            kept = [L if p else L + s - dr for L, dr, p in zip(before, drop, paused)]
            assert sess.lengths == kept
            for n in live:                                       # oracle B: the kept rows, one at a time, in a plain session
                x, qq = rig.seqs[n]
                for j in range(kept[n] - before[n]):
                    p = before[n] + j
                    c = rig.refs[n].step(qq[:, :, p:p + 1], x[:, :, p:p + 1], x[:, :, p:p + 1])
                    assert torch.equal(got[n, j], c[0, 0]), ("kept context", it, n, j)
                    z = int(rig.refs[n].csr.crow[0, 1])
                    assert torch.equal(rows_csr[n][j], rig.refs[n].csr.col[0, :z].cpu()), ("kept CSR row", it, n, j)
                _assert_slot(sess, n, rig.refs[n])               # paused slots: unchanged
        sess.resume([n for n in range(N) if not sess.empty[n]])
        q, k = rig.rows(2)
        sess.step(q, k, k)
        sess.pause([1])                                          # a pause ends the chance to rewind
        with pytest.raises(ValueError, match="no step to undo"):
            sess.rewind([0] * N)


# ---- 7. the emit + unfused launch pair --------------------------------------------------------------------------------------
@GRAPH
@pytest.mark.parametrize("dtype,H,d,lengths", [SHAPES[0], SHAPES[2]])       # (H = 40: the emit is a launch of its own)
def test_unfused_attention_session(dtype, H, d, lengths, use_graph):
    rig = Rig(H, d, lengths, 14, dtype, use_graph, none=(2,), fused_attention=False)
    sess = rig.sess
    with torch.no_grad():
        sess.pause([0])
        for i in range(12):
            if i == 3:
                sess.resume([0])
            if i == 5:
                sess.pause([1, 3])
            if i == 6:
                sess.pause([0])                                  # everybody sits out
            if i == 8:
                sess.resume([0, 1, 3])
            rig.step(f"step {i}")
        rig.check_slots()


# ---- 8. refusals ------------------------------------------------------------------------------------------------------------
@GRAPH
def test_refusals_change_nothing(use_graph):
    dtype, H, d, lengths = torch.bfloat16, 8, 64, [8, 70, 40]
    rig = Rig(H, d, lengths, 28, dtype, use_graph, none=(2,), page_rows=64)
    sess = rig.sess

    def refused(exc, match, call, *args):
        state = (list(sess.lengths), sess.paused, sess.empty, [list(p) for p in sess.pages], sess.free_pages)
        with pytest.raises(exc, match=match):
            call(*args)
        assert state == (list(sess.lengths), sess.paused, sess.empty, [list(p) for p in sess.pages], sess.free_pages)
        rig.step(f"after the refused {call.__name__}{args}")

    with torch.no_grad():
        rig.step("first")
        for call in (sess.pause, sess.resume, sess.release):
            refused(IndexError, r"slot\(s\) \[3\]", call, [0, 3])
            refused(IndexError, r"slot\(s\) \[-1\]", call, -1)
        refused(ValueError, r"resume: slot\(s\) \[2\] are empty", sess.resume, [0, 2])
        refused(ValueError, "empty", sess.export_state, 2)
        refused(ValueError, "empty", sess.sequence_kv, 2)
        refused(ValueError, "empty", sess.fork, 2, [0])
        refused(ValueError, r"\[2\] are empty", sess.reorder, [2, 1, 2])
        sess.pause([1])
        sess.pause([1])                                          # twice is harmless
        sess.pause([2])
        sess.release([2])                                        # so is pausing / releasing an empty slot
        assert sess.paused == [False, True, True] and sess.empty == [False, False, True]
        rig.step("paused twice")
        sess.reorder([1, 1, 2])                                  # the paused state travels with the contents
        assert sess.paused == [True, True, True]
        rig.seqs[0], rig.refs[0] = rig.seqs[1], rig.plain(rig.pre[1])
        x, q = rig.seqs[1]
        for p in range(lengths[1], sess.lengths[1]):             # (the fresh reference catches up with slot 1's steps)
            rig.refs[0].step(q[:, :, p:p + 1], x[:, :, p:p + 1], x[:, :, p:p + 1])
        sess.resume([0])
        rig.step("the copy goes on, its parent stays")
        rig.check_slots()
        # a uniform session has one shared position: nothing can sit out
        st, kp, vp = rig.pre[0]
        uni = DecodeSession(rig.layer.attention, st, kp, vp, capacity=20, use_graph=False)
        for call in (uni.pause, uni.resume, uni.release):
            with pytest.raises(ValueError, match="ragged"):
                call([0])
        assert uni.paused == [False] and uni.empty == [False]


def test_from_sequences_needs_one_real_sequence():
    layer = _layer(8, 64, 64, torch.bfloat16)
    with pytest.raises(ValueError, match="at least one"):
        DecodeSession.from_sequences(layer.attention, [None, None], 32)
