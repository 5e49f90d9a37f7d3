"""-m gpu: `DecodeSession(..., attention_probs=True)` -- the module's `partial_attention_probs` (row_scale * softmax per CSR
entry) from graph-replayed decode steps.  Oracle: the cached forward over the same rows, continued from the state exported
before the step, with `attention.return_attention_probs = True`: values and row starts bit for bit; the column ids after
re-encoding -- a session encodes head * capacity + key (its launches have static arguments), the forward head * T_src + key.
H = 8, bf16, lengths [8, 61, 250] (the last one crosses T_src = 256 during the run), capacity 300."""
import pytest
import torch

from sea_attention_amd import opt_plumbing as P
from sea_attention_amd.perlin_attention import get_default_config, register_default_config
from sea_attention_amd.perlin_attention.decode import DecodeSession
from test_gpu_decode_ragged import _layer, _mask, _prefill, _sequences

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, LENGTHS, CAPACITY = 8, [8, 61, 250], 300


def _build(d, dtype, steps, seed=7, **kw):
    layer = _layer(H, d, CAPACITY + 4, dtype)
    seqs = _sequences(H, d, LENGTHS, steps, dtype, seed)
    with torch.no_grad():
        pre = [_prefill(layer, x, q, L) for (x, q), L in zip(seqs, LENGTHS)]
        sess = DecodeSession.from_sequences(layer.attention, pre, CAPACITY, **kw)
    return layer, seqs, pre, sess


def _rows(seqs, pos, s=1):
    q = torch.cat([q[:, :, p:p + s] for (_x, q), p in zip(seqs, pos)])
    k = torch.cat([x[:, :, p:p + s] for (x, _q), p in zip(seqs, pos)])
    return q, k


def _wire(ap):
    """The handle read the way a caller of the reference reads `partial_attention_probs`."""
    return ap.crow_indices().cpu(), ap.col_indices().cpu(), ap.values().cpu()


def _forward_probs(layer, seqs, n, state, L, s, dtype):
    x, qq = seqs[n]
    at = layer.attention
    at.return_attention_probs = True
    try:
        fwd = layer(None, None, None, query_layer=qq[:, :, L:L + s], key_layer=x[:, :, :L + s], value_layer=x[:, :, :L + s],
                    attention_mask=_mask(s, L + s, dtype), last_state=state)
    finally:
        at.return_attention_probs = False
    return fwd.partial_attention_probs


def _assert_slot(wire, n, want, capacity, T_src, tag):
    crow_s, col_s, val_s = (t[n] for t in wire)
    crow_f, col_f, val_f = want.crow_indices()[0].cpu(), want.col_indices()[0].cpu(), want.values()[0].cpu()
    assert torch.equal(crow_s, crow_f), (tag, n, "crow")
    z = int(crow_f[-1])
    assert z > 0 and val_f.shape[0] == z
    assert val_s.dtype == val_f.dtype and torch.equal(val_s[:z], val_f), (tag, n, "values", (val_s[:z] - val_f).abs().max().item())
    assert torch.equal((col_s[:z] // capacity) * T_src + col_s[:z] % capacity, col_f), (tag, n, "columns")
    assert bool((val_s[z:] == 0).all()) and bool((col_s[z:] == 0).all()), (tag, n, "padding")      # the wire format's zero fill


def _steps_against_forward(layer, seqs, sess, steps, dtype, tag):
    with torch.no_grad():
        for i in range(steps):
            before = list(sess.lengths)
            exported = [sess.export_state(n) for n in range(sess.N)]
            q, k = _rows(seqs, before)
            sess.step(q, k, k)
            ap = sess.attention_probs
            assert ap is not None and ap.col_is_pending == sess.csr.col_is_pending
            assert ap.crow is sess.csr.crow and ap.vals.data_ptr() == sess._probs_buf.data_ptr()
            wire = _wire(ap)                                                 # (every step: also on replayed ones)
            assert not ap.col_is_pending and not sess.csr.col_is_pending     # reading the columns emitted them, as for session.csr
            for n in range(sess.N):
                want = _forward_probs(layer, seqs, n, exported[n], before[n], 1, dtype)
                _assert_slot(wire, n, want, sess.capacity, before[n] + 1, f"{tag} step {i}")


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_session_probs_equal_the_cached_forward(use_graph):
    dtype, steps = torch.bfloat16, 10
    layer, seqs, pre, sess = _build(64, dtype, steps, use_graph=use_graph, attention_probs=True)
    assert tuple(sess._probs_buf.shape) == (3, sess.z_cap) and sess._probs_buf.dtype == torch.float32
    assert sess.attention_probs is None                                      # an output of a step: none yet
    _steps_against_forward(layer, seqs, sess, steps, dtype, "d64")
    assert sess.lengths[2] > 256 > LENGTHS[2]
    if use_graph:
        assert sess.captures == 1


@pytest.mark.parametrize("d,dtype", [(80, torch.bfloat16), (128, torch.float16)])
def test_session_probs_other_head_sizes(d, dtype):
    layer, seqs, pre, sess = _build(d, dtype, 7, attention_probs=True)
    _steps_against_forward(layer, seqs, sess, 7, dtype, f"d{d}")
    assert sess.captures == 1


def test_session_probs_paged_equal_contiguous():
    dtype, steps = torch.bfloat16, 8
    layer, seqs, pre, a = _build(64, dtype, steps, attention_probs=True)
    with torch.no_grad():
        b = DecodeSession.from_sequences(layer.attention, pre, CAPACITY, page_rows=64, attention_probs=True)
        assert b.paged
        for i in range(steps):
            q, k = _rows(seqs, a.lengths)
            ca = a.step(q, k, k).clone()
            cb = b.step(q, k, k)
            assert torch.equal(ca, cb), i
            assert b.attention_probs.col_is_pending
            for x, y in zip(_wire(a.attention_probs), _wire(b.attention_probs)):
                assert torch.equal(x, y), i
    assert a.captures == b.captures == 1


def test_session_probs_multi_row_steps_and_rewind():
    dtype, d = torch.bfloat16, 64
    layer, seqs, pre, sess = _build(d, dtype, 16, max_step_rows=4, attention_probs=True)
    assert tuple(sess._probs_buf.shape) == (3, 4 * sess.z_cap)
    with torch.no_grad():
        for j, s in enumerate([4, 1, 3, "rewind", 2]):
            if s == "rewind":
                sess.rewind([2, 0, 0])
                assert sess.attention_probs is not None                      # (an output of the last step: rewind leaves it alone)
                continue
            before = list(sess.lengths)
            exported = [sess.export_state(n) for n in range(sess.N)]
            q, k = _rows(seqs, before, s)
            sess.step(q, k, k)
            assert sess.attention_probs.T_dst == s and sess.attention_probs.col_is_pending
            wire = _wire(sess.attention_probs)
            for n in range(sess.N):
                want = _forward_probs(layer, seqs, n, exported[n], before[n], s, dtype)
                _assert_slot(wire, n, want, sess.capacity, before[n] + s, f"rows step {j} ({s} rows)")
    assert sess.lengths == [LENGTHS[0] + 8, LENGTHS[1] + 10, LENGTHS[2] + 10] and sess.captures == 4   # graphs for s = 4, 1, 3, 2


def test_session_probs_unfused_attention_equal_fused():
    dtype, steps = torch.bfloat16, 8
    layer, seqs, pre, a = _build(64, dtype, steps, attention_probs=True)
    with torch.no_grad():
        b = DecodeSession.from_sequences(layer.attention, pre, CAPACITY, fused_attention=False, attention_probs=True)
        for i in range(steps):
            q, k = _rows(seqs, a.lengths)
            ca = a.step(q, k, k).clone()
            cb = b.step(q, k, k)
            assert torch.equal(ca, cb), i
            assert a.attention_probs.col_is_pending and not b.attention_probs.col_is_pending
            for x, y in zip(_wire(a.attention_probs), _wire(b.attention_probs)):
                assert torch.equal(x, y), i


def test_session_probs_paused_slot_has_an_empty_row():
    dtype, steps = torch.bfloat16, 6
    layer, seqs, pre, a = _build(64, dtype, steps, attention_probs=True)
    with torch.no_grad():
        b = DecodeSession.from_sequences(layer.attention, pre, CAPACITY, attention_probs=True)     # the twin: nobody pauses
        for i in range(steps):
            if i == 2:
                a.pause(1)
            if i == 4:
                a.resume(1)
            pos_a, pos_b = list(a.lengths), list(b.lengths)
            assert pos_a[0] == pos_b[0] and pos_a[2] == pos_b[2]
            qa, ka = _rows(seqs, pos_a)
            qb, kb = _rows(seqs, pos_b)
            a.step(qa, ka, ka)
            b.step(qb, kb, kb)
            wa, wb = _wire(a.attention_probs), _wire(b.attention_probs)
            sitting = 2 <= i < 4
            if sitting:
                assert wa[0][1].tolist() == [0, 0], i                        # slot 1: an empty row
                assert bool((wa[1][1] == 0).all()) and bool((wa[2][1] == 0).all()), i
            for n in (0, 2):
                z = int(wb[0][n, -1])
                assert z > 0 and torch.equal(wa[0][n], wb[0][n]), (i, n)
                assert torch.equal(wa[1][n, :z], wb[1][n, :z]) and torch.equal(wa[2][n, :z], wb[2][n, :z]), (i, n)
    assert a.captures == 1 and a.lengths[1] == LENGTHS[1] + steps - 2


def test_session_without_probs_is_unchanged():
    dtype, steps = torch.bfloat16, 4
    layer, seqs, pre, a = _build(64, dtype, steps, attention_probs=False)
    with torch.no_grad():
        b = DecodeSession.from_sequences(layer.attention, pre, CAPACITY)
        u = DecodeSession(layer.attention, pre[2][0], pre[2][1], pre[2][2], CAPACITY, attention_probs=False)
        assert a._probs_buf is None and u._probs_buf is None and u.attention_probs is None
        for i in range(steps):
            q, k = _rows(seqs, a.lengths)
            ca = a.step(q, k, k).clone()
            cb = b.step(q, k, k)
            assert torch.equal(ca, cb), i
            assert a.attention_probs is None and b.attention_probs is None
            assert a.csr.col_is_pending and b.csr.col_is_pending
    assert a.captures == b.captures == 1


@pytest.fixture
def restore_default():
    old = get_default_config()
    yield
    register_default_config(old)


def test_opt_block_returns_attentions_from_the_graph_path(restore_default):
    """`decode_graph_attentions` beside `decode_graph_capacity`: a one-token call with output_attentions=True stays on the
    replayed session and returns what the regular cached forward returns (ids re-encoded from the capacity)."""
    from sea_attention_amd.perlin_attention.decode import SessionState
    dev, dtype = "cuda", torch.bfloat16
    cfg = P.perlin_config_from_options(perlin_k=16, perlin_predictor_length=256, perlin_performer_nb_feature_factor=8,
                                       perlin_context_output_method="mix")
    cfg.use_cache = True
    torch.manual_seed(5)
    blk = P.SeaOPTAttention(4 * 64, 4, max_position_embeddings=160).to(dev, dtype).eval()
    blk.benchmarking = True
    blk.perlin_self_attention.attention.context_layer_dtype = dtype
    assert blk.decode_graph_attentions is False
    N, T0, new = 2, 100, 5
    T = T0 + new
    x = torch.randn(N, T, 4 * 64, device=dev, dtype=dtype)

    def run(capacity, attentions):
        blk.decode_graph_capacity, blk.decode_graph_attentions, blk._decode_session = capacity, attentions, None
        rows, probs, kinds = [], [], []
        with torch.no_grad():
            _, _, past = blk(x[:, :T0], attention_mask=P.causal_additive_mask(N, T0, T0, dtype, dev))
            for pos in range(T0, T):
                y, att, past = blk(x[:, pos:pos + 1], past_key_value=past, output_attentions=True,
                                   attention_mask=P.causal_additive_mask(N, 1, pos + 1, dtype, dev))
                assert att is not None
                rows.append(y.clone())
                probs.append((att.crow_indices().cpu(), att.col_indices().cpu(), att.values().cpu()))
                kinds.append(isinstance(past[2], SessionState))
        return rows, probs, kinds

    ref_rows, ref_probs, ref_kinds = run(None, False)
    cap = T + 4
    fb_rows, fb_probs, fb_kinds = run(cap, False)                    # unset: exactly the fallback of before
    assert ref_kinds == fb_kinds == [False] * new and blk._decode_session is None
    got_rows, got_probs, kinds = run(cap, True)
    assert kinds == [True] * new and blk._decode_session.captures == 1
    for i in range(new):
        T_src = T0 + i + 1
        assert torch.equal(got_rows[i], ref_rows[i]) and torch.equal(fb_rows[i], ref_rows[i]), i
        (crow_g, col_g, val_g), (crow_r, col_r, val_r) = got_probs[i], ref_probs[i]
        assert torch.equal(crow_g, crow_r), i
        for n in range(N):
            z = int(crow_r[n, -1])
            assert z > 0 and torch.equal(val_g[n, :z], val_r[n, :z]), (i, n)
            assert torch.equal((col_g[n, :z] // cap) * T_src + col_g[n, :z] % cap, col_r[n, :z]), (i, n)
        for a, b in zip(fb_probs[i], ref_probs[i]):
            assert torch.equal(a, b), i
