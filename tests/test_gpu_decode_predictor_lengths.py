"""-m gpu: decode sessions at the predictor lengths below 256 (T_M = 64 / 96 / 128: the reference's grid).  The fused CNN + tail
+ selection launch runs its general-length tail there (csrc/sea_topk.hip: tail_select_row_gen in decode_cnn_tail_select_kernel /
_rows_kernel), the uniform session's round-4 launches the decode form of the general-length tail + selection kernel, and the
one-row decode attention runs below T_m = 256 inside a session.

Nothing here is compared with another form of the session alone.  The references are
  * the STATELESS forward over the whole sequence (`use_cache=False`; its general-length kernels are pinned to the oracle and
    the golden fixtures by test_gpu_grid.py / test_gpu_golden.py): every context row and probability row bit for bit;
  * the oracle's `resize_m_to_t_csr` on the step's own kept-pixel bits: crow / col of every step, read on every step;
  * an fp64 softmax on the CPU over the oracle's columns for the context of one case (the Reference of
    test_gpu_decode_reference.py, copied).
The ragged variants (paging + fork, multi-row steps + rewind, pause / resume, extend) are held to the contiguous one-row
ragged session, which is itself held to the stateless forward in this file."""
import pytest
import torch

import sea_attention_amd as S
from oracle import sea_oracle as O
from sea_attention_amd.perlin_attention import PerlinAttentionConfig, PerlinSelfAttention, ops
from sea_attention_amd.perlin_attention.attention_state import PerlinAttentionState as PS
from sea_attention_amd.perlin_attention.decode import DecodeSession

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = 64
STEPS = 8
# fp32 context against the fp64 reference (test_gpu_decode_reference.py's bound; outputs O(1)): max |err| over the 8 steps of
# test_uniform_session_context_matches_fp64 observed 8.7e-8 on MI355X
TOL32 = 2e-6


class Cfg:
    def __init__(self, hidden, heads, max_pos):
        self.hidden_size, self.num_attention_heads, self.max_position_embeddings = hidden, heads, max_pos


def _mask(N, T_dst, T_src, dtype):
    fp_min = torch.finfo(torch.float16).min / 2
    rows = torch.arange(T_src - T_dst, T_src, device=DEV).view(T_dst, 1)
    m = ((torch.arange(T_src, device=DEV).view(1, T_src) > rows) * fp_min).view(1, 1, T_dst, T_src)
    return m.expand(N, 1, T_dst, T_src).contiguous().to(dtype)


def _layer(H, d, T_M, k, max_pos, dtype, use_cache):
    S.seed(42)
    pc = PerlinAttentionConfig(k=k, attention_predictor_length=T_M, performer_nb_factor=8, causal=True, k_flatten=True,
                               k_flatten_dim='causal_batch', context_output_method='mix', use_cache=use_cache)
    layer = PerlinSelfAttention(Cfg(H * d, H, max_pos), pc).to(DEV).to(dtype).eval()
    for m in layer.modules():
        if hasattr(m, 'benchmarking'):
            m.benchmarking = True
    layer.attention.force_torch_estimator = False
    # steps J-L on ONE kernel ("auto" plans per launch: equal to rounding, not to the bit -- test_kv_cache.py); fp32 context
    layer.attention.sparse_kernel = "gather"
    return layer


def _pair(H, d, T_M, k, max_pos, dtype):
    """The stateless layer and the cached one, same weights."""
    full = _layer(H, d, T_M, k, max_pos, dtype, use_cache=False)
    cached = _layer(H, d, T_M, k, max_pos, dtype, use_cache=True)
    cached.load_state_dict(full.state_dict())
    return full, cached


def _forward(layer, q, x, lo, hi, state=None):
    N = x.shape[0]
    return layer(None, None, None, query_layer=q[:, :, lo:hi], key_layer=x[:, :, :hi], value_layer=x[:, :, :hi],
                 attention_mask=_mask(N, hi - lo, hi, x.dtype), last_state=state)


# ---- the oracle's columns (copied from test_gpu_decode_reference.py) ---------------------------------------------------
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
        N, H, T_dst, Dh = q.shape
        self.keys = {}
        for n in range(N):
            for t in range(T_dst):
                ids = col[n, int(crow[n, t]):int(crow[n, t + 1])]
                hs = torch.div(ids, T_cap, rounding_mode="floor")
                for h in range(H):
                    self.keys[n, h, t] = ids[hs == h] - h * T_cap
        self.out = torch.zeros((N, H, T_dst, Dh), dtype=torch.float64)
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


def _step_columns(sess, T_src, what):
    """The step's kept pixels are the oracle's top-k of the map the step returned, and its crow / col the oracle's
    interpolation of those bits for a T_src-long sequence.  Reads `.col`."""
    N, H, k, T_M = sess.N, sess.H, sess.k, sess.T_M
    csr = sess.csr
    assert csr is not None, what
    mask = unpack_bits(csr.bits, H, T_M)
    probs = sess.probs.reshape(N, H, 1, T_M).float().cpu()
    assert torch.equal(mask, O.grouped_topk_mask(probs, sess.keep_table[T_src - 1:T_src].cpu())), (what, "bits")
    crow_o, col_o = oracle_columns(mask, k, T_src, sess.capacity)
    assert torch.equal(csr.crow.cpu().long(), crow_o), (what, "crow")
    col = csr.col.cpu().long()
    for n in range(N):
        z = int(crow_o[n, -1])
        assert z > 0 and torch.equal(col[n, :z], col_o[n, :z]), (what, "col", n)
    return crow_o, col_o


# ---- the stateless reference of a uniform case, computed once per (case, prefix) ----------------------------------------
_UNIFORM = {}


def _uniform_reference(dtype, H, T_M, k, L, N, deeper=False):
    key = (dtype, H, T_M, k, L, N, deeper)
    if key not in _UNIFORM:
        T = L + STEPS
        full, cached = _pair(H, D, T_M, k, T + 3, dtype)
        S.seed(1000 + L)
        x = torch.randn((N, H, T, D), device=DEV).to(dtype)
        q = (x.float() * D ** -0.5).to(dtype)
        with torch.no_grad():
            ref = _forward(full, q, x, 0, T)
            pre = _forward(cached, q, x, 0, L)
            end = _forward(cached, q, x, 0, T)                               # the cached forward's state after every row
        _UNIFORM[key] = dict(cached=cached, x=x, q=q, ctx=ref.context_layer.clone(),
                             probs=ops.realize(ref.estimated_attention_probs_m).clone(), state=pre.state, end=end.state)
    return _UNIFORM[key]


def _run_uniform(r, L, use_graph, columns=True, fused_cnn=True):
    x, q, T = r["x"], r["q"], L + STEPS
    at = r["cached"].attention
    with torch.no_grad():
        sess = DecodeSession(at, r["state"], x[:, :, :L], x[:, :, :L], capacity=T + 3, use_graph=use_graph)
        assert (sess.graph is not None) == use_graph and sess.fused_cnn == fused_cnn and sess.T_M == at.pconfig.attention_predictor_length
        widths = set()
        for i in range(STEPS):
            hi = L + i + 1
            got = sess.step(q[:, :, hi - 1:hi], x[:, :, hi - 1:hi], x[:, :, hi - 1:hi])
            assert torch.isfinite(got.float()).all()
            want = r["ctx"][:, hi - 1:hi]
            assert got.dtype == want.dtype and torch.equal(got, want), (i, (got.float() - want.float()).abs().max().item())
            assert torch.equal(sess.probs, r["probs"][:, :, hi - 1:hi]), (i, "probs")
            if columns:
                _step_columns(sess, hi, f"step {i}")
            widths.add(-(-hi // sess.T_M))
        assert sess.length == T
        assert torch.equal(sess.image, r["end"].states[PS.PERFORMER].image)
        assert torch.equal(sess.win, r["end"].states[PS.CNN].rows_c8)
    return sess, widths


def _prefixes(T_M):
    """T_M - 3: the 8 steps cross T_M (pixel widths 1 -> 2) and, except at T_M = 96, a Performer chunk boundary (64 rows) --
    there a prefix of 61 crosses the chunk boundary; 2 T_M - 3 (widths 2 -> 3) at T_M = 64."""
    return [T_M - 3] + ([61] if T_M == 96 else []) + ([2 * T_M - 3] if T_M == 64 else [])


# (dtype, H, T_M, k, N)
UNIFORM = [(torch.bfloat16, 4, 64, 8, 2),        # E = 1, one channel tile
           (torch.float16, 12, 96, 16, 2),       # OPT-125m's heads, W4 = 24, masked lanes
           (torch.bfloat16, 8, 128, 16, 2),
           (torch.float16, 32, 128, 16, 1),      # four channel tiles
           (torch.bfloat16, 40, 64, 8, 1)]       # 80 channels: the emit is its own launch
UNIFORM_L = [c + (L,) for c in UNIFORM for L in _prefixes(c[2])]
# ceil(w / T_M) reaches and passes k (every kept pixel thinned; z_cap and the keep table at their k-limited end)
UNIFORM_L.append((torch.bfloat16, 4, 64, 4, 1, 4 * 64 - 3))


def _uid(c):
    return f"{'bf16' if c[0] == torch.bfloat16 else 'fp16'}-H{c[1]}-TM{c[2]}-k{c[3]}-L{c[5]}"


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype,H,T_M,k,N,L", UNIFORM_L, ids=[_uid(c) for c in UNIFORM_L])
def test_uniform_session_rows_equal_the_stateless_forward(dtype, H, T_M, k, N, L, use_graph):
    """Every step: the context row and `session.probs` are the stateless forward's rows bit for bit, the kept pixels the
    oracle's top-k of that map, crow / col the oracle's interpolation of them; after the last step the Performer image and the
    CNN window are the cached forward's state."""
    assert ops.decode_cnn_supported(2 * H, H, T_M, dtype)
    r = _uniform_reference(dtype, H, T_M, k, L, N)
    sess, widths = _run_uniform(r, L, use_graph)
    assert len(widths) == 2 or L == 61, "the steps cross a multiple of T_M"
    if k == 4:
        assert max(widths) > k                                              # thinned pixels


def test_uniform_session_context_matches_fp64(monkeypatch):
    """(bf16, H = 8, T_M = 128): the fp32 context of every step against the fp64 reference over the oracle's columns, within
    TOL32 -- the one-row decode attention below T_m = 256 inside a session.  The row scale, the average and the mix the step
    handed to the attention launch are taken from that call (an eager session: every step makes it)."""
    dtype, H, T_M, k, N = torch.bfloat16, 8, 128, 16, 2
    L = T_M - 3
    r = _uniform_reference(dtype, H, T_M, k, L, N)
    x, q, T = r["x"], r["q"], L + STEPS
    seen = []
    real = ops.sparse_attention

    def spy(q_in, kc, vc, csr, **kw):
        seen.append((q_in, kc, vc, {n: kw.get(n) for n in ("row_scale", "avg", "mix")}))
        return real(q_in, kc, vc, csr, **kw)
    monkeypatch.setattr(ops, "sparse_attention", spy)
    worst = 0.0
    with torch.no_grad():
        sess = DecodeSession(r["cached"].attention, r["state"], x[:, :, :L], x[:, :, :L], capacity=T + 3, use_graph=False)
        for i in range(STEPS):
            hi = L + i + 1
            seen.clear()
            got = sess.step(q[:, :, hi - 1:hi], x[:, :, hi - 1:hi], x[:, :, hi - 1:hi])
            assert got.dtype == torch.float32 and len(seen) == 1
            crow_o, col_o = _step_columns(sess, hi, f"step {i}")
            q_in, kc, vc, epi = seen[0]
            assert epi["avg"] is not None and epi["mix"] is not None
            ref = Reference(q_in, kc, vc, crow_o, col_o, sess.capacity, **epi)
            o32 = got.view(N, 1, H, D).permute(0, 2, 1, 3)
            err = (o32.double().cpu() - ref.out).abs().max().item()
            worst = max(worst, err)
            assert torch.isfinite(o32).all() and err <= TOL32, (i, err)
            assert ref.sensitivity(hi) >= 10 * TOL32, (i, "a wrong key would pass")
    print(f"[decode-predictor-lengths] observed fp32 max|err| vs fp64 over {STEPS} steps = {worst:.3e}")


# ---- the round-4 launches (deeper predictor body) -------------------------------------------------------------------------
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_round4_launches_equal_the_stateless_forward(monkeypatch, use_graph):
    """PERLIN_HOTFIX_OPT_DEEPER=1 (three convolutions): the uniform session runs the window convolutions and the DECODE form of
    the general-length tail + selection kernel (`sea_predictor_tail_select` with t_src_dev and crow_out at T_M = 128)."""
    monkeypatch.setenv("PERLIN_HOTFIX_OPT_DEEPER", "1")
    dtype, H, T_M, k, N = torch.bfloat16, 4, 128, 16, 1
    L = T_M - 3
    r = _uniform_reference(dtype, H, T_M, k, L, N, deeper=True)
    from sea_attention_amd.perlin_attention.attention_state import cnn_lookback
    assert cnn_lookback(r["cached"].attention.attention_predictor_cnn) == 12
    sess, widths = _run_uniform(r, L, use_graph, fused_cnn=False)
    assert sess.win.shape[1] == 12 and len(widths) == 2


# ---- ragged sessions ------------------------------------------------------------------------------------------------------
_RAGGED = {}


def _ragged_reference(dtype, H, T_M, k, lengths, steps, ext=None):
    """Per sequence: x / q of L_i + steps rows, the stateless forward over all of them, the prefill over the first L_i.
    `ext` = (i, rows): sequence i's tensors carry `rows` more rows (an extension)."""
    key = (dtype, H, T_M, k, tuple(lengths), steps, ext)
    if key not in _RAGGED:
        cap = max(lengths) + steps + (ext[1] if ext else 0) + 2
        full, cached = _pair(H, D, T_M, k, cap + 2, dtype)
        g = torch.Generator(device=DEV).manual_seed(7)
        seqs = []
        with torch.no_grad():
            for i, L in enumerate(lengths):
                T = L + steps + (ext[1] if ext and ext[0] == i else 0)
                x = torch.randn((1, H, T, D), device=DEV, generator=g).to(dtype)
                q = (x.float() * D ** -0.5).to(dtype)
                ref = _forward(full, q, x, 0, T)
                pre = _forward(cached, q, x, 0, L)
                seqs.append(dict(x=x, q=q, L=L, ctx=ref.context_layer.clone(), probs=ops.realize(ref.estimated_attention_probs_m).clone(),
                                 pre=(pre.state, x[:, :, :L], x[:, :, :L])))
        _RAGGED[key] = dict(cached=cached, seqs=seqs, capacity=cap)
    return _RAGGED[key]


def _rows(seqs, pos, s=1):
    """Rows pos[n] .. pos[n] + s of every sequence, stacked: q, k (= v), (N, H, s, d)."""
    return (torch.cat([sq["q"][:, :, p:p + s] for sq, p in zip(seqs, pos)]), torch.cat([sq["x"][:, :, p:p + s] for sq, p in zip(seqs, pos)]))


def _lengths(T_M):
    return [8, T_M - 2, 2 * T_M - 3, 61]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("dtype,H,T_M,k", [(torch.bfloat16, 8, 128, 16), (torch.float16, 12, 96, 16)], ids=["bf16-H8-TM128", "fp16-H12-TM96"])
def test_ragged_rows_equal_each_sequences_stateless_forward(dtype, H, T_M, k, use_graph):
    """Lengths 8 (the CNN's reach), either side of T_M and of 2 T_M, and 61 (a Performer chunk boundary crossed): every row of
    every slot is that sequence's stateless forward, bit for bit."""
    lengths, steps = _lengths(T_M), 6
    r = _ragged_reference(dtype, H, T_M, k, lengths, steps)
    seqs = r["seqs"]
    with torch.no_grad():
        sess = DecodeSession.from_sequences(r["cached"].attention, [sq["pre"] for sq in seqs], r["capacity"], use_graph=use_graph)
        assert sess.ragged and sess.fused_cnn and sess.T_M == T_M and (sess.graph is not None) == use_graph
        for i in range(steps):
            pos = [L + i for L in lengths]
            q, kx = _rows(seqs, pos)
            got = sess.step(q, kx, kx)
            for n, (sq, p) in enumerate(zip(seqs, pos)):
                assert torch.equal(got[n:n + 1], sq["ctx"][:, p:p + 1]), (i, n, (got[n:n + 1] - sq["ctx"][:, p:p + 1]).abs().max().item())
                assert torch.equal(sess.probs[n:n + 1], sq["probs"][:, :, p:p + 1]), (i, n, "probs")
        assert sess.lengths == [L + steps for L in lengths]


RAG = (torch.bfloat16, 8, 128, 16)


def _contiguous_rows(r, order, steps, first=None):
    """The contiguous one-row ragged session over sequences seqs[order[n]] (slot n), `steps` steps: [(ctx, probs, crow)] per
    step, cloned.  `first`: the row each slot starts from (default: its prefix length)."""
    seqs = [r["seqs"][i] for i in order]
    out = []
    with torch.no_grad():
        sess = DecodeSession.from_sequences(r["cached"].attention, [sq["pre"] for sq in seqs], r["capacity"])
        for i in range(steps):
            q, kx = _rows(seqs, [sq["L"] + i for sq in seqs])
            got = sess.step(q, kx, kx)
            out.append((got.clone(), sess.probs.clone(), sess.crow.clone()))
    return out


def _same(sess, got, want, slots, tag, row=0):
    ctx, probs, crow = want
    for n in slots:
        assert torch.equal(got[n:n + 1, row:row + 1], ctx[n:n + 1]), (tag, n)
        assert torch.equal(sess.probs[n:n + 1, :, row:row + 1], probs[n:n + 1]), (tag, n, "probs")


def test_ragged_paged_fork_into_a_released_slot():
    """page_rows = 64: one step, slot 3 released, slot 1 (127 rows: an open page to copy, a closed page to share) forked into
    it, three steps (slot 1 and its copy cross the page boundary at 128 on different rows): every slot bitwise the contiguous
    session whose slot 3 was sequence 1 from the start."""
    dtype, H, T_M, k = RAG
    lengths, steps = _lengths(T_M), 4
    r = _ragged_reference(dtype, H, T_M, k, lengths, steps)
    seqs = r["seqs"]
    # after the fork slot 3 takes sequence 3's rows (the copies diverge); the contiguous twin: sequence 1 in slot 3, same rows
    with torch.no_grad():
        twin = DecodeSession.from_sequences(r["cached"].attention, [seqs[i]["pre"] for i in (0, 1, 2, 1)], r["capacity"])
        sess = DecodeSession.from_sequences(r["cached"].attention, [sq["pre"] for sq in seqs], r["capacity"], page_rows=64)
        assert sess.paged and not twin.paged
        q, kx = _rows(seqs, lengths)
        sess.step(q, kx, kx)
        qt, kt = _rows([seqs[i] for i in (0, 1, 2, 1)], [lengths[i] for i in (0, 1, 2, 1)])
        twin.step(qt, kt, kt)
        sess.release([3])
        sess.fork(1, [3])
        assert sess.lengths[3] == lengths[1] + 1 and sess.slot_pages.shared()
        for i in range(1, steps):
            q, kx = _rows(seqs, [L + i for L in lengths])
            got = sess.step(q, kx, kx)
            want = twin.step(q, kx, kx)
            assert torch.equal(got, want), (i, (got - want).abs().max().item())
            assert torch.equal(sess.probs, twin.probs) and torch.equal(sess.crow, twin.crow), i
            # slots 0 .. 2 against the stateless forward as well
            for n in range(3):
                assert torch.equal(got[n:n + 1], seqs[n]["ctx"][:, lengths[n] + i:lengths[n] + i + 1]), (i, n)


def test_ragged_multi_row_steps_and_rewind():
    """max_step_rows = 4: steps of 4, 1 and 3 rows, then rewind([2, 0, 0, 0]) and one more step -- every row bitwise the
    contiguous one-row session's (slot 0 takes its row 6 again after the rewind)."""
    dtype, H, T_M, k = RAG
    lengths, steps = _lengths(T_M), 9
    r = _ragged_reference(dtype, H, T_M, k, lengths, steps)
    seqs, N = r["seqs"], 4
    one = _contiguous_rows(r, range(N), steps)
    with torch.no_grad():
        sess = DecodeSession.from_sequences(r["cached"].attention, [sq["pre"] for sq in seqs], r["capacity"], max_step_rows=4)
        done = 0
        for s in (4, 1, 3):
            q, kx = _rows(seqs, [L + done for L in lengths], s)
            got = sess.step(q, kx, kx)
            assert tuple(got.shape) == (N, s, H * D)
            for j in range(s):
                _same(sess, got, one[done + j], range(N), f"rows {done}+{j}", row=j)
            done += s
        sess.rewind([2, 0, 0, 0])
        assert sess.lengths == [lengths[0] + 6] + [L + 8 for L in lengths[1:]]
        q, kx = _rows(seqs, sess.lengths)
        got = sess.step(q, kx, kx)
        _same(sess, got, one[6], [0], "slot 0 after the rewind")
        _same(sess, got, one[8], [1, 2, 3], "the other slots")


def test_ragged_pause_and_resume_across_two_steps():
    dtype, H, T_M, k = RAG
    lengths, steps = _lengths(T_M), 5
    r = _ragged_reference(dtype, H, T_M, k, lengths, steps)
    seqs, N = r["seqs"], 4
    one = _contiguous_rows(r, range(N), steps)
    others = [0, 2, 3]
    with torch.no_grad():
        sess = DecodeSession.from_sequences(r["cached"].attention, [sq["pre"] for sq in seqs], r["capacity"])
        behind = 0                                                          # steps slot 1 has sat out
        for i in range(steps):
            if i == 1:
                sess.pause([1])
            if i == 3:
                sess.resume([1])
            sitting = i in (1, 2)
            pos = [L + i - (behind if n == 1 else 0) for n, L in enumerate(lengths)]
            q, kx = _rows(seqs, pos)
            got = sess.step(q, kx, kx)
            _same(sess, got, one[i], others, f"step {i}")
            if sitting:
                assert not got[1].any() and int(sess.crow[1, 1]) == 0, i
                behind += 1
            else:
                _same(sess, got, one[i - behind], [1], f"step {i}, slot 1")
        assert sess.lengths[1] == lengths[1] + steps - 2


def test_ragged_extend_of_a_forked_slot():
    """A paged session with an empty slot: slot 1 forked into it, the copy extended by 70 rows at once (across a page boundary
    and a Performer chunk boundary).  The 70 rows are the stateless forward's; the three steps behind them are bitwise the
    contiguous session built from a prefill of all 126 + 70 rows."""
    dtype, H, T_M, k = RAG
    lengths, steps, E = _lengths(T_M), 3, 70
    r = _ragged_reference(dtype, H, T_M, k, lengths, steps, ext=(1, E))
    seqs = r["seqs"]
    s1, L1 = seqs[1], lengths[1]
    with torch.no_grad():
        long_pre = _forward(r["cached"], s1["q"], s1["x"], 0, L1 + E)
        twin = DecodeSession.from_sequences(r["cached"].attention, [seqs[0]["pre"], s1["pre"], seqs[2]["pre"],
                                                                    (long_pre.state, s1["x"][:, :, :L1 + E], s1["x"][:, :, :L1 + E])], r["capacity"])
        sess = DecodeSession.from_sequences(r["cached"].attention, [seqs[0]["pre"], s1["pre"], seqs[2]["pre"], None], r["capacity"],
                                            page_rows=64)
        sess.fork(1, [3])
        rows = slice(L1, L1 + E)
        got = sess.extend(3, s1["q"][:, :, rows], s1["x"][:, :, rows], s1["x"][:, :, rows])
        assert torch.equal(got, s1["ctx"][:, rows]), (got - s1["ctx"][:, rows]).abs().max().item()
        assert sess.lengths == [lengths[0], L1, lengths[2], L1 + E]
        four = [seqs[0], s1, seqs[2], s1]
        for i in range(steps):
            pos = [lengths[0] + i, L1 + i, lengths[2] + i, L1 + E + i]
            q, kx = _rows(four, pos)
            a = sess.step(q, kx, kx)
            b = twin.step(q, kx, kx)
            assert torch.equal(a, b), (i, (a - b).abs().max().item())
            assert torch.equal(sess.probs, twin.probs) and torch.equal(sess.crow, twin.crow), i
            assert torch.equal(a[3:4], s1["ctx"][:, pos[3]:pos[3] + 1]), i


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_longer_predictor_lengths_and_other_head_sizes_are_refused():
    dtype, H, k, L = torch.bfloat16, 4, 16, 40
    x = torch.randn((1, H, L, D), device=DEV).to(dtype)
    q = (x.float() * D ** -0.5).to(dtype)
    layer = _layer(H, D, 384, k, 64, dtype, use_cache=True)
    with torch.no_grad():
        out = _forward(layer, q, x, 0, L)
        for build in (lambda: DecodeSession(layer.attention, out.state, x, x, capacity=48, use_graph=False),
                      lambda: DecodeSession.from_sequences(layer.attention, [(out.state, x, x)], 48, use_graph=False)):
            with pytest.raises(ValueError, match=r"T_M <= 256 \(got T_M = 384\).*W4 = T_M / 4 <= 64 in ConvRowC8.*T_m <= 256 in the one-row"):
                build()
    # d = 128 at T_M = 128: the one-launch MLP serves other predictor lengths at d = 64 only, so the cached forward leaves no
    # state a session continues
    x = torch.randn((1, H, L, 128), device=DEV).to(dtype)
    q = (x.float() * 128 ** -0.5).to(dtype)
    layer = _layer(H, 128, 128, k, 64, dtype, use_cache=True)
    with torch.no_grad():
        out = _forward(layer, q, x, 0, L)
        with pytest.raises((AssertionError, ValueError), match="HIP estimator"):
            DecodeSession(layer.attention, out.state, x, x, capacity=48, use_graph=False)
        with pytest.raises(ValueError, match="HIP estimator"):
            DecodeSession.from_sequences(layer.attention, [(out.state, x, x)], 48, use_graph=False)
