"""-m gpu: multi-token steps and rewind of a ragged session (`DecodeSession.from_sequences(..., max_step_rows=S)`).
Oracle A: every row of an s-row step, kept or dropped, is bitwise the cached forward over those s rows from the state exported
before the step (context and estimated probabilities).  Oracle B: after each rewind every slot is bitwise an N = 1 plain
session (max_step_rows=None) that stepped only the kept rows one at a time -- lengths, exported image and window, K / V,
the kept rows' context and CSR rows and columns -- and so is every later step.  Eager and graph-replayed."""
import random

import pytest
import torch

from sea_attention_amd.perlin_attention.attention_state import PerlinAttentionState as PS
from sea_attention_amd.perlin_attention.decode import DecodeSession
from test_gpu_decode_ragged import _layer, _mask, _prefill, _sequences

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _rows(seqs, pos, s):
    """The s new rows of every slot from its own position: q, k (= v), (N, H, s, d)."""
    q = torch.cat([q[:, :, p:p + s] for (_x, q), p in zip(seqs, pos)])
    k = torch.cat([x[:, :, p:p + s] for (x, _q), p in zip(seqs, pos)])
    return q, k


def _build(H, d, lengths, capacity, dtype, use_graph, S=8, seed=7):
    layer = _layer(H, d, capacity + 4, dtype)
    seqs = _sequences(H, d, lengths, capacity - min(lengths), dtype, seed)
    with torch.no_grad():
        pre = [_prefill(layer, x, q, L) for (x, q), L in zip(seqs, lengths)]
        sess = DecodeSession.from_sequences(layer.attention, pre, capacity, use_graph=use_graph, max_step_rows=S)
        refs = [DecodeSession.from_sequences(layer.attention, [p], capacity, use_graph=False) for p in pre]
    return layer, seqs, pre, sess, refs


def _oracle_a(layer, seqs, sess, got, exported, before, s, dtype):
    for n, st in enumerate(exported):
        x, qq = seqs[n]
        L = before[n]
        fwd = layer(None, None, None, query_layer=qq[:, :, L:L + s], key_layer=x[:, :, :L + s], value_layer=x[:, :, :L + s],
                    attention_mask=_mask(s, L + s, dtype), last_state=st)
        assert torch.equal(got[n:n + 1], fwd.context_layer), ("context", n, L, s)
        assert torch.equal(sess.probs[n:n + 1], fwd.estimated_attention_probs_m), ("probs", n, L, s)


def _csr_rows(sess, s):
    crow, col = sess.csr.crow.cpu(), sess.csr.col.cpu()
    return [[col[n, crow[n, j]:crow[n, j + 1]] for j in range(s)] for n in range(sess.N)]


def _oracle_b(sess, refs, seqs, got, rows_csr, before, kept):
    """Step every plain reference through its kept rows; compare the kept rows and then the slot's whole state."""
    for n, ref in enumerate(refs):
        x, qq = seqs[n]
        for j in range(kept[n] - before[n]):
            p = before[n] + j
            c = ref.step(qq[:, :, p:p + 1], x[:, :, p:p + 1], x[:, :, p:p + 1])
            assert torch.equal(got[n, j], c[0, 0]), ("kept context", n, j)
            z = int(ref.csr.crow[0, 1])
            assert torch.equal(rows_csr[n][j], ref.csr.col[0, :z].cpu()), ("kept CSR row", n, j)
        _assert_slot(sess, n, ref)


def _assert_slot(sess, n, ref):
    assert sess.lengths[n] == ref.lengths[0], (n, sess.lengths[n], ref.lengths[0])
    a, b = sess.export_state(n), ref.export_state(0)
    assert torch.equal(a.states[PS.PERFORMER].image, b.states[PS.PERFORMER].image), ("image", n)
    assert torch.equal(a.states[PS.CNN].rows_c8, b.states[PS.CNN].rows_c8), ("window", n)
    for u, v in zip(sess.sequence_kv(n), ref.sequence_kv(0)):
        assert torch.equal(u, v), ("K / V", n)


def _run(layer, seqs, sess, refs, schedule, dtype, rng, check_a=True):
    for s, mode in schedule:
        before = list(sess.lengths)
        exported = [sess.export_state(n) for n in range(sess.N)] if check_a else None
        q, k = _rows(seqs, before, s)
        got = sess.step(q, k, k).clone()
        if check_a:
            _oracle_a(layer, seqs, sess, got, exported, before, s, dtype)
        rows_csr = _csr_rows(sess, s)
        if mode == "all":
            drop = [s] * sess.N
        elif mode == "none":
            drop = [0] * sess.N
        else:
            drop = [rng.choice([0, s, rng.randint(0, s)]) for _ in range(sess.N)]
        sess.rewind(drop)
        kept = [L + s - dr for L, dr in zip(before, drop)]
        assert sess.lengths == kept
        _oracle_b(sess, refs, seqs, got, rows_csr, before, kept)


# lengths: 8 = the CNN's reach; just below a Performer chunk boundary (64 at d = 64, 32 at d = 80 / 128: rewinds fall back
# across it); either side of T_src = 256 and 512 (pixel widths 1 -> 2 -> 3)
CASES = [(torch.bfloat16, 8, 64, [8, 250, 508, 60]),
         (torch.float16, 32, 64, [8, 61, 255, 510, 126]),
         (torch.bfloat16, 40, 64, [8, 254, 505, 62]),            # 80 channels
         (torch.bfloat16, 8, 80, [8, 29, 251, 509]),
         (torch.float16, 8, 128, [8, 30, 253, 506]),
         (torch.bfloat16, 32, 128, [8, 28, 259, 507])]
SCHEDULE = [(5, "rand"), (8, "all"), (3, "rand"), (1, "rand"), (8, "rand"), (2, "none"), (5, "rand"), (8, "rand")]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype,H,d,lengths", CASES)
def test_rows_match_cached_forward_and_plain_session(dtype, H, d, lengths, use_graph):
    capacity = max(lengths) + sum(s for s, _ in SCHEDULE) + 8
    layer, seqs, pre, sess, refs = _build(H, d, lengths, capacity, dtype, use_graph)
    with torch.no_grad():
        _run(layer, seqs, sess, refs, SCHEDULE, dtype, random.Random(1234))
    if use_graph:
        assert sess.captures == len({s for s, _ in SCHEDULE})


def test_rewind_everything_restores_the_pre_step_export():
    dtype, H, d, lengths = torch.bfloat16, 8, 64, [8, 60, 63, 250]
    capacity = 300
    layer, seqs, pre, sess, refs = _build(H, d, lengths, capacity, dtype, True)
    with torch.no_grad():
        for s in (8, 5, 1):
            before = [sess.export_state(n) for n in range(sess.N)]
            kv = [sess.sequence_kv(n) for n in range(sess.N)]
            L = list(sess.lengths)
            q, k = _rows(seqs, L, s)
            sess.step(q, k, k)
            sess.rewind([s] * sess.N)
            assert sess.lengths == L
            for n in range(sess.N):
                a = sess.export_state(n)
                assert torch.equal(a.states[PS.PERFORMER].image, before[n].states[PS.PERFORMER].image), (s, n)
                assert torch.equal(a.states[PS.CNN].rows_c8, before[n].states[PS.CNN].rows_c8), (s, n)
                for u, v in zip(sess.sequence_kv(n), kv[n]):
                    assert torch.equal(u, v)


def test_one_row_steps_equal_the_plain_session_and_captures():
    dtype, H, d, lengths = torch.float16, 8, 64, [8, 62, 255]
    capacity = 300
    layer, seqs, pre, sess, _refs = _build(H, d, lengths, capacity, dtype, True)
    with torch.no_grad():
        plain = DecodeSession.from_sequences(layer.attention, pre, capacity)
        for i in range(4):                                   # s = 1 on S = 8: the plain session's rows, bit for bit
            q, k = _rows(seqs, sess.lengths, 1)
            got = sess.step(q, k, k).clone()
            assert torch.equal(got, plain.step(q, k, k))
            assert torch.equal(sess.probs, plain.probs) and torch.equal(sess.csr.crow, plain.crow)
        assert sess.captures == 1
        for s in (2, 2, 4, 1, 4):
            q, k = _rows(seqs, sess.lengths, s)
            sess.step(q, k, k)
        assert sess.captures == 3                            # once per distinct s
        sess.rewind([1, 0, 4])
        assert sess.captures == 3
        x, qq = seqs[1]
        sess.admit(1, *_prefill(layer, x, qq, 40))
        assert sess.captures == 3


def test_admit_after_rewind_and_rewind_after_admit():
    dtype, H, d, lengths = torch.bfloat16, 8, 64, [8, 61, 100]
    capacity = 200
    layer, seqs, pre, sess, refs = _build(H, d, lengths, capacity, dtype, True)
    rng = random.Random(5)
    with torch.no_grad():
        _run(layer, seqs, sess, refs, [(5, "rand")], dtype, rng, check_a=False)
        x, qq = seqs[0]
        new = _prefill(layer, x, qq, 30)
        sess.admit(0, *new)                                  # after a rewind: works
        refs[0] = DecodeSession.from_sequences(layer.attention, [new], capacity, use_graph=False)
        _assert_slot(sess, 0, refs[0])
        q, k = _rows(seqs, sess.lengths, 3)
        sess.step(q, k, k)
        sess.admit(2, *_prefill(layer, *seqs[2], 50))
        with pytest.raises(ValueError, match="no step to undo"):
            sess.rewind([0, 0, 0])                           # after an admit: refused


def test_opt_1_3b_round():
    """OPT-1.3B shape (H = 32, d = 64, bf16), N = 8, lengths 1000 .. 4000, one s = 4 step: oracles A and B."""
    dtype, H, d = torch.bfloat16, 32, 64
    lengths = [1000 + 3000 * i // 7 for i in range(8)]
    capacity = max(lengths) + 16
    layer, seqs, pre, sess, refs = _build(H, d, lengths, capacity, dtype, True, seed=11)
    with torch.no_grad():
        _run(layer, seqs, sess, refs, [(4, "rand"), (4, "rand")], dtype, random.Random(8))


def test_rows_refusals():
    dtype, H, d, lengths = torch.bfloat16, 8, 64, [8, 60]
    capacity = 80
    layer, seqs, pre, sess, refs = _build(H, d, lengths, capacity, dtype, True, S=4)
    with torch.no_grad():
        with pytest.raises(ValueError, match="max_step_rows"):
            DecodeSession.from_sequences(layer.attention, pre, capacity, max_step_rows=9)
        with pytest.raises(ValueError, match="contiguous"):
            DecodeSession.from_sequences(layer.attention, pre, capacity, max_step_rows=4, page_rows=64)
        with pytest.raises(ValueError, match="contiguous"):
            DecodeSession.from_sequences(layer.attention, pre, capacity, max_step_rows=4, fused_attention=False)
        plain = DecodeSession.from_sequences(layer.attention, pre, capacity)
        q, k = _rows(seqs, plain.lengths, 2)
        with pytest.raises(ValueError, match="one row per step"):
            plain.step(q, k, k)
        with pytest.raises(ValueError, match="max_step_rows"):
            plain.rewind([0, 0])
        with pytest.raises(ValueError, match="no step to undo"):
            sess.rewind([0, 0])
        refusals = [
            (lambda: sess.step(*(_rows(seqs, sess.lengths, 5)[i] for i in (0, 1, 1))), ValueError, "1 .. 4"),
            (lambda: sess.step(q[:1], k[:1], k[:1]), ValueError, "step: q, k, v"),
            (lambda: sess.step(q, k[:, :, :1], k), ValueError, "step: q, k, v"),
            (lambda: sess.step(q.float(), k.float(), k.float()), ValueError, "GPU"),
        ]
        for fn, exc, msg in refusals:
            with pytest.raises(exc, match=msg):
                fn()
        rng = random.Random(3)
        _run(layer, seqs, sess, refs, [(4, "rand")], dtype, rng, check_a=False)
        before = list(sess.lengths)
        q, k = _rows(seqs, before, 4)
        got = sess.step(q, k, k).clone()
        rows_csr = _csr_rows(sess, 4)
        for drop, msg in (([0], "counts for 2 slots"), ([5, 0], "outside 0 .. 4"), ([-1, 0], "outside 0 .. 4")):
            with pytest.raises(ValueError, match=msg):
                sess.rewind(drop)
        sess.rewind([1, 2])
        _oracle_b(sess, refs, seqs, got, rows_csr, before, [before[0] + 3, before[1] + 2])
        with pytest.raises(ValueError, match="no step to undo"):
            sess.rewind([0, 0])                              # twice
        _run(layer, seqs, sess, refs, [(3, "none")], dtype, rng, check_a=False)
        # capacity: slot 1 at 60 + ... within 80; a step that would pass it is refused naming the slot
        while sess.lengths[1] + 4 <= capacity:
            _run(layer, seqs, sess, refs, [(4, "none")], dtype, rng, check_a=False)
        with pytest.raises(RuntimeError, match=r"slot\(s\) \[1\]"):
            sess.step(*(_rows(seqs, [0, 0], 4)[i] for i in (0, 1, 1)))
        rest = capacity - sess.lengths[1]
        if rest:
            _run(layer, seqs, sess, refs, [(rest, "none")], dtype, rng, check_a=False)
