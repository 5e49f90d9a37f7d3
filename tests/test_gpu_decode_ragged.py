"""-m gpu: decoding sequences of DIFFERENT lengths in one session (`DecodeSession.from_sequences`).  Every row of a ragged
session must be bitwise the row of that sequence's own N = 1 session (which test_decode_session.py holds to the cached
forward): context, estimated probabilities, CSR row and columns -- eagerly launched and graph-replayed."""
import pytest
import torch

import sea_attention_amd as S
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention
from sea_attention_amd.perlin_attention.attention_state import PerlinAttentionState as PS
from sea_attention_amd.perlin_attention.decode import DecodeSession

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_M, K = 256, 16


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


def _step_refs(refs, seqs, pos):
    """One step of every N = 1 reference session: (context, probs, crow) copies."""
    out = []
    for ref, (x, q), p in zip(refs, seqs, pos):
        c = ref.step(q[:, :, p:p + 1], x[:, :, p:p + 1], x[:, :, p:p + 1]).clone()
        out.append((c, ref.probs.clone(), ref.crow.clone()))
    return out


def _assert_rows(sess, got, want, tag):
    for n, (c, probs, crow) in enumerate(want):
        assert torch.equal(got[n:n + 1], c), (tag, n, (got[n:n + 1].float() - c.float()).abs().max().item())
        assert torch.equal(sess.probs[n:n + 1], probs), (tag, n)
        assert torch.equal(sess.crow[n:n + 1], crow), (tag, n)


def _setup(H, d, lengths, steps, capacity, dtype, use_graph=True, fused_attention=True, seed=7):
    layer = _layer(H, d, capacity + 4, dtype)
    seqs = _sequences(H, d, lengths, steps, dtype, seed)
    with torch.no_grad():
        pre = [_prefill(layer, x, q, L) for (x, q), L in zip(seqs, lengths)]
        refs = [DecodeSession(layer.attention, st, kp, vp, capacity=capacity, use_graph=use_graph, fused_attention=fused_attention)
                for st, kp, vp in pre]
        sess = DecodeSession.from_sequences(layer.attention, pre, capacity, use_graph=use_graph, fused_attention=fused_attention)
    return layer, seqs, pre, refs, sess


# lengths: 8 = the CNN's reach; either side of T_M = 256 (pixel widths differ inside the batch); a Performer chunk boundary
# crossed during the run (64 for d = 64, 32 for d = 80 / 128); the longest sequence fills the caches to capacity - 1
CASES = [(torch.bfloat16, 8, 64, [8, 250, 300, 60]),
         (torch.float16, 32, 64, [8, 61, 255, 262, 40, 300, 120, 9]),
         (torch.bfloat16, 40, 64, [8, 254, 290, 62]),            # 80 channels: the emit is a launch of its own
         (torch.bfloat16, 8, 80, [8, 29, 251, 280]),
         (torch.float16, 8, 128, [8, 30, 253, 260]),
         (torch.bfloat16, 32, 128, [8, 28, 259, 100])]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype,H,d,lengths", CASES)
def test_ragged_rows_equal_single_sequence_sessions(dtype, H, d, lengths, use_graph):
    steps = 6
    capacity = max(lengths) + steps                                           # the longest sequence writes row capacity - 1
    layer, seqs, pre, refs, sess = _setup(H, d, lengths, steps, capacity, dtype, use_graph=use_graph)
    assert sess.ragged and sess.fused_cnn and (sess.graph is not None) == use_graph
    assert tuple(sess.ctr32.shape) == (len(lengths), 3) and sess.lengths == lengths
    with torch.no_grad():
        for i in range(steps):
            pos = [L + i for L in lengths]
            q, k = _batch_rows(seqs, pos)
            got = sess.step(q, k, k)
            _assert_rows(sess, got, _step_refs(refs, seqs, pos), f"step {i}")
    assert sess.lengths == [L + steps for L in lengths]
    assert sess.ctr32[:, 0].tolist() == sess.lengths and sess.ctr32[:, 1].tolist() == [L + 1 for L in sess.lengths]
    for n, ref in enumerate(refs):
        assert torch.equal(sess.image.view(len(lengths), -1)[n], ref.image)
        assert torch.equal(sess.win[n:n + 1], ref.win)
    with pytest.raises(RuntimeError, match="capacity"):                     # the longest sequence has filled its cache
        sess.step(q, k, k)


def test_ragged_with_equal_lengths_equals_the_uniform_session():
    dtype, H, d, L, steps, N = torch.bfloat16, 8, 64, 250, 10, 3
    layer = _layer(H, d, L + steps + 4, dtype)
    g = torch.Generator(device=DEV).manual_seed(3)
    x = torch.randn((N, H, L + steps, d), device=DEV, generator=g).to(dtype)
    q = (x.float() * d ** -0.5).to(dtype)
    with torch.no_grad():
        uni = DecodeSession(layer.attention, _prefill(layer, x, q, L)[0], x[:, :, :L], x[:, :, :L], capacity=L + steps + 1)
        pre = [_prefill(layer, x[n:n + 1], q[n:n + 1], L) for n in range(N)]
        rag = DecodeSession.from_sequences(layer.attention, pre, L + steps + 1)
        assert not uni.ragged and tuple(uni.ctr32.shape) == (3,)
        for i in range(steps):
            r = slice(L + i, L + i + 1)
            a = uni.step(q[:, :, r], x[:, :, r], x[:, :, r]).clone()
            b = rag.step(q[:, :, r], x[:, :, r], x[:, :, r])
            assert torch.equal(a, b), i
            assert torch.equal(uni.probs, rag.probs) and torch.equal(uni.crow, rag.crow), i
        assert torch.equal(uni.image, rag.image) and torch.equal(uni.win, rag.win)
        assert torch.equal(uni.kv_cache, rag.kv_cache)


@pytest.mark.parametrize("H,d", [(8, 64), (40, 64), (8, 80)])
def test_ragged_attention_forms_and_pending_columns(H, d):
    """fused_attention=True (the attention launch expands the pixels, columns pending) and False (emit + unfused launch) give
    the same bits; each sequence's pending columns, read on two different replayed steps, are its N = 1 session's."""
    dtype, lengths, steps = torch.bfloat16, [8, 70, 258, 31], 5
    capacity = max(lengths) + steps + 2
    layer, seqs, pre, refs, a = _setup(H, d, lengths, steps, capacity, dtype)
    with torch.no_grad():
        b = DecodeSession.from_sequences(layer.attention, pre, capacity, fused_attention=False)
        assert a.fused_attention and not b.fused_attention
        for i in range(steps):
            pos = [L + i for L in lengths]
            q, k = _batch_rows(seqs, pos)
            ga = a.step(q, k, k).clone()
            gb = b.step(q, k, k)
            assert torch.equal(ga, gb), i
            assert torch.equal(a.crow, b.crow) and torch.equal(a.probs, b.probs), i
            _step_refs(refs, seqs, pos)
            if i in (1, steps - 1):                                      # two different replayed steps
                assert a.csr.t_src_stride > 0 and a.csr.col_is_pending
                ca = a.csr.col                                           # first read: the ragged emit runs now
                for n, ref in enumerate(refs):
                    nnz = int(a.crow[n, 1].item())
                    assert nnz > 0 and nnz == int(ref.crow[0, 1].item())
                    assert torch.equal(ca[n, :nnz], ref.csr.col[0, :nnz]), (i, n)
                    assert torch.equal(b.csr.col[n, :nnz], ca[n, :nnz]), (i, n)


def test_ragged_export_state_equals_the_single_sequence_export():
    dtype, H, d, lengths, steps = torch.bfloat16, 8, 64, [8, 120, 262], 4
    capacity = max(lengths) + steps + 2
    layer, seqs, pre, refs, sess = _setup(H, d, lengths, steps, capacity, dtype, seed=21)
    with torch.no_grad():
        for i in range(steps):
            pos = [L + i for L in lengths]
            q, k = _batch_rows(seqs, pos)
            sess.step(q, k, k)
            _step_refs(refs, seqs, pos)
        with pytest.raises(ValueError, match="export_state\\(slot\\)"):
            sess.export_state()
        for n, ref in enumerate(refs):
            got, want = sess.export_state(n), ref.export_state()
            assert got.seq_len == want.seq_len == lengths[n] + steps
            assert torch.equal(got.states[PS.PERFORMER].image, want.states[PS.PERFORMER].image)
            assert torch.equal(got.states[PS.CNN].rows_c8, want.states[PS.CNN].rows_c8)


def test_ragged_export_then_cached_forward_next_row():
    """export_state(slot) after some steps, then one cached-forward step on the next row: equals the session's next row."""
    dtype, H, d, lengths, steps = torch.bfloat16, 8, 64, [8, 120, 262], 4
    capacity = max(lengths) + steps + 3
    layer, seqs, pre, refs, sess = _setup(H, d, lengths, steps + 1, capacity, dtype, seed=23)
    with torch.no_grad():
        for i in range(steps):
            q, k = _batch_rows(seqs, [L + i for L in lengths])
            sess.step(q, k, k)
        exported = [sess.export_state(n) for n in range(len(lengths))]
        nxt = [L + steps for L in lengths]
        q, k = _batch_rows(seqs, nxt)
        got = sess.step(q, k, k).clone()
        for n, st in enumerate(exported):
            x, qq = seqs[n]
            hi = nxt[n] + 1
            fwd = layer(None, None, None, query_layer=qq[:, :, hi - 1:hi], key_layer=x[:, :, :hi], value_layer=x[:, :, :hi],
                        attention_mask=_mask(1, hi, dtype), last_state=st)
            assert torch.equal(got[n:n + 1], fwd.context_layer), n


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_ragged_admit_replaces_one_slot(use_graph):
    dtype, H, d, lengths, steps = torch.bfloat16, 8, 64, [8, 200, 262, 63], 4
    capacity = 400
    layer, seqs, pre, refs, sess = _setup(H, d, lengths, 2 * steps, capacity, dtype, use_graph=use_graph, seed=31)
    captures = getattr(sess, "captures", 0)
    with torch.no_grad():
        for i in range(steps):
            pos = [L + i for L in lengths]
            q, k = _batch_rows(seqs, pos)
            got = sess.step(q, k, k)
            _assert_rows(sess, got, _step_refs(refs, seqs, pos), f"step {i}")
        # slot 1 starts over on a new prompt of 300 rows
        L_new = 300
        (x_new, q_new), = _sequences(H, d, [L_new], steps, dtype, seed=99)
        st_new = _prefill(layer, x_new, q_new, L_new)
        sess.admit(1, *st_new)
        assert sess.lengths[1] == L_new and getattr(sess, "captures", 0) == captures
        refs[1] = DecodeSession(layer.attention, *st_new, capacity=capacity, use_graph=use_graph)
        seqs[1] = (x_new, q_new)
        start = [L + steps for L in lengths]
        start[1] = L_new
        for i in range(steps):
            pos = [p + i for p in start]
            q, k = _batch_rows(seqs, pos)
            got = sess.step(q, k, k)
            _assert_rows(sess, got, _step_refs(refs, seqs, pos), f"after admit, step {i}")
    assert getattr(sess, "captures", 0) == captures


def test_ragged_refusals(monkeypatch):
    dtype, H, d = torch.bfloat16, 8, 64
    layer = _layer(H, d, 300, dtype)
    seqs = _sequences(H, d, [40, 50], 0, dtype, seed=5)
    with torch.no_grad():
        pre = [_prefill(layer, x, q, x.shape[2]) for x, q in seqs]
        with pytest.raises(ValueError, match="no room"):                        # L_i >= capacity
            DecodeSession.from_sequences(layer.attention, pre, 50, use_graph=False)
        with pytest.raises(ValueError, match="at least one"):
            DecodeSession.from_sequences(layer.attention, [], 64, use_graph=False)
        (xs, qs), = _sequences(H, d, [5], 0, dtype, seed=6)                    # shorter than the CNN's reach (8 rows)
        with pytest.raises(ValueError, match="reach"):
            DecodeSession.from_sequences(layer.attention, pre + [_prefill(layer, xs, qs, 5)], 64, use_graph=False)
        st, kp, vp = pre[0]
        with pytest.raises(ValueError, match="exactly its prefix"):
            DecodeSession.from_sequences(layer.attention, [(st, kp[:, :, :30], vp[:, :, :30])], 64, use_graph=False)
        with pytest.raises(ValueError, match="N = 1"):
            DecodeSession.from_sequences(layer.attention, [(st, torch.cat([kp, kp]), torch.cat([vp, vp]))], 64, use_graph=False)
        with pytest.raises(ValueError, match="D = 64"):                          # mismatched head size / dtype
            DecodeSession.from_sequences(layer.attention, [pre[0], (st, kp[..., :32], vp[..., :32])], 64, use_graph=False)
        with pytest.raises(ValueError, match="bfloat16"):
            DecodeSession.from_sequences(layer.attention, [pre[0], (st, kp.half(), vp.half())], 64, use_graph=False)
        sess = DecodeSession.from_sequences(layer.attention, pre, 64, use_graph=False)
        with pytest.raises(IndexError):
            sess.admit(2, *pre[0])
        uni = DecodeSession(layer.attention, *pre[0], capacity=64, use_graph=False)
        with pytest.raises(ValueError, match="ragged"):
            uni.admit(0, *pre[1])
    # fp32 data
    layer32 = _layer(H, d, 300, torch.float32)
    (x, q), = _sequences(H, d, [40], 0, torch.float32, seed=7)
    with torch.no_grad():
        with pytest.raises(ValueError, match="16-bit"):
            DecodeSession.from_sequences(layer32.attention, [(None, x, x)], 64, use_graph=False)
    # H > 40: beyond the fused CNN launch
    layer44 = _layer(44, d, 300, dtype)
    (x, q), = _sequences(44, d, [40], 0, dtype, seed=8)
    with torch.no_grad():                                       # (refused before the state is read)
        with pytest.raises(ValueError, match="fused CNN launch"):
            DecodeSession.from_sequences(layer44.attention, [(None, x, x)], 64, use_graph=False)
    # the deeper (three-convolution) predictor
    monkeypatch.setenv("PERLIN_HOTFIX_OPT_DEEPER", "1")
    layer3 = _layer(H, d, 300, dtype)
    (x, q), = _sequences(H, d, [40], 0, dtype, seed=9)
    with torch.no_grad():
        with pytest.raises(ValueError, match="3 convolutions"):
            DecodeSession.from_sequences(layer3.attention, [(None, x, x)], 64, use_graph=False)
