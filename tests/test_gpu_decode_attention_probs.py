"""-m gpu: the per-entry probabilities (`partial_attention_probs`: row_scale * softmax, one fp32 per CSR slot) out of the DECODE
forms of `sea_sparse_attention` -- sparse_attn_decode1_kernel for one new row (contiguous and paged), the DEC instantiations
of sparse_attn_rows_kernel / sparse_attn_rows80_kernel for 2..8 rows and for fp32 data.

The shapes are `CASES_A` of test_gpu_decode_reference.py: the smallest at which these kernels branch (see there).  Per case
everything is computed once (`_case`) and shared by the tests:

  1. bitwise: the fused decode launch with probabilities leaves the handle pending, returns the context of the launch without
     them, and its values equal, slot by slot, those of emit + the plain kernel (the route that served `want_probs` before);
  2. no stray writes into a buffer pre-filled with a sentinel (padded slots of a ragged head total, empty heads, the slots
     behind the rows), every written value in [0, row_scale];
  3. against an fp64 softmax over the oracle's columns;
  4. paged K / V: bitwise the contiguous call;
  5. a sequence that sits out writes nothing and changes no bit of the other.
"""
import functools

import pytest
import torch

from sea_attention_amd.perlin_attention import ops
from test_gpu_decode_reference import CASES_A, Reference, _caches, _case_id, _selection, oracle_columns

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
T_M = 256
SENT = -7.0              # what a probability can never be: the buffers are pre-filled with it
PAD = 5                  # slots of the buffers behind z_cap (probs_stride_n > col_stride_n)
# fp32 probabilities against the fp64 reference (p * row_scale, values in [0, 1]): max |err| of emit + the plain kernel -- the
# route that served `want_probs` before the fused decode forms did, `parent` below -- over every case of CASES_A observed
# 9.54e-8 on MI355X (fp16-d64-rows1-T1100-k4); the bound is 4 x that.  The margin is for other seeds only: the fused decode
# forms execute the same instructions on the same operands
TOL_P = 3.8e-7


def _handle(sel, H, T_cap, k, z_cap, ts, pending, items=None):
    cut = (lambda t: t) if items is None else (lambda t: t[items[0]:items[1]].contiguous())
    return ops.csr_from_selection(cut(sel.bits), cut(sel.row_nnz), cut(sel.head_off), H, T_M, T_cap, k, True, z_cap,
                                  t_src_dev=ts, defer_emit=pending)


def _sentinel(N, z_cap):
    return torch.full((N, z_cap + PAD), SENT, dtype=torch.float32, device=DEV)


def _slot_ranges(crow, head_off):
    """[(n, t, h, beg, end)] of every (row, head): its slots inside `col[n]` / `probs[n]`."""
    N, T_dst, H1 = head_off.shape
    return [(n, t, h, int(crow[n, t] + head_off[n, t, h]), int(crow[n, t] + head_off[n, t, h + 1]))
            for n in range(N) for t in range(T_dst) for h in range(H1 - 1)]


@functools.lru_cache(maxsize=None)
def _case(i):
    dtype, d, T_dst, T_src, k, keep_count, heavy = CASES_A[i]
    N, H = 2, 4 if heavy else 8
    T_cap = T_src + 40
    sel, mask = _selection(dtype, N, H, T_dst, T_src, k, keep_count, heavy, seed=T_src + 7 * T_dst + d)
    z_cap = max(int(sel.crow[:, -1].max().item()), 1)
    kk, vv = _caches(N, H, T_src, T_cap, d, dtype)
    q = (torch.randn((N, H, T_dst, d), device=DEV) * d ** -0.5).to(dtype)
    rs = torch.rand((N, H, T_dst), device=DEV) * 0.5 + 0.5
    mix = torch.rand((N, H, T_dst), device=DEV) * 0.5 + 0.5
    avg = torch.randn((N, H, T_dst, d), device=DEV).to(dtype)
    epi = dict(row_scale=rs, avg=avg, mix=mix)
    ts = torch.full((N, 1), T_src, dtype=torch.int32, device=DEV)          # a length per sequence
    c = dict(N=N, H=H, T_cap=T_cap, z_cap=z_cap, sel=sel, mask=mask, q=q, kk=kk, vv=vv, epi=epi, ts=ts,
             crow=sel.crow.cpu().long(), head_off=sel.head_off.cpu().long(), rs=rs.cpu())
    # the fused decode launch: without probabilities, with them (a fresh zero-filled tensor), into a sentinel buffer
    h0 = _handle(sel, H, T_cap, k, z_cap, ts, True)
    c["ctx_plain"] = ops.sparse_attention(q, kk, vv, h0, path="gather", keep_columns_pending=True, **epi)
    h1 = _handle(sel, H, T_cap, k, z_cap, ts, True)
    assert h1.t_src_stride > 0 and h1.col_is_pending
    c["ctx"], c["probs"] = ops.sparse_attention(q, kk, vv, h1, path="gather", want_probs=True, keep_columns_pending=True, **epi)
    c["pending_after"] = h1.col_is_pending
    h2 = _handle(sel, H, T_cap, k, z_cap, ts, True)
    buf = _sentinel(N, z_cap)
    c["ctx_buf"], got = ops.sparse_attention(q, kk, vv, h2, path="gather", keep_columns_pending=True, probs_out=buf, **epi)
    assert got is buf
    c["buf"], c["pending_after_buf"] = buf.cpu(), h2.col_is_pending
    # the route that served want_probs before: a handle whose columns the emit launch wrote + the plain kernel
    hp = _handle(sel, H, T_cap, k, z_cap, ts, False)
    assert not hp.col_is_pending
    c["ctx_parent"], pp = ops.sparse_attention(q, kk, vv, hp, path="gather", want_probs=True, **epi)
    c["parent"] = pp.cpu()
    c["probs"] = c["probs"].cpu()
    torch.cuda.synchronize()
    return c


@functools.lru_cache(maxsize=None)
def _reference_probs(i):
    """fp64 p * row_scale of every non-empty (n, h, t), in column order: {(n, h, t): tensor}, over the ORACLE's columns."""
    dtype, d, T_dst, T_src, k, keep_count, heavy = CASES_A[i]
    c = _case(i)
    crow_o, col_o = oracle_columns(c["mask"], k, T_src, c["T_cap"])
    assert torch.equal(crow_o, c["crow"])
    ref = Reference(c["q"], c["kk"], c["vv"], crow_o, col_o, c["T_cap"], row_scale=c["epi"]["row_scale"])
    out = {}
    for (n, h, t), keys in ref.keys.items():
        p = ref.head(n, h, t, keys)[1]
        if p is not None:
            out[n, h, t] = p * ref.rs[n, h, t]
    return out


IDS = [_case_id(c) for c in CASES_A]


@pytest.mark.parametrize("i", range(len(CASES_A)), ids=IDS)
def test_fused_decode_probs_bitwise(i):
    c = _case(i)
    assert c["pending_after"] and c["pending_after_buf"], "the fused decode form did not serve the launch (columns were emitted)"
    assert torch.equal(c["ctx"], c["ctx_plain"]) and torch.equal(c["ctx_buf"], c["ctx_plain"])
    assert torch.equal(c["ctx_parent"], c["ctx_plain"])
    rows = 0
    for n, t, h, beg, end in _slot_ranges(c["crow"], c["head_off"]):
        assert torch.equal(c["probs"][n, beg:end], c["parent"][n, beg:end]), (n, t, h)
        assert torch.equal(c["buf"][n, beg:end], c["parent"][n, beg:end]), (n, t, h)
        rows += end > beg
    assert rows > 0


@pytest.mark.parametrize("i", range(len(CASES_A)), ids=IDS)
def test_fused_decode_probs_no_stray_writes(i):
    dtype, d, T_dst, T_src, k, keep_count, heavy = CASES_A[i]
    c = _case(i)
    buf, crow, N = c["buf"], c["crow"], c["N"]
    for n in range(N):
        lo, hi = int(crow[n, 0]), int(crow[n, T_dst])
        assert lo == 0 and bool((buf[n, :lo] == SENT).all()) and bool((buf[n, hi:] == SENT).all()), n
        assert hi < buf.shape[1]
    # inside the rows: exactly the slots of the heads' ranges, each finite and in [0, row_scale of its (n, h, t)]
    covered = torch.zeros_like(buf, dtype=torch.bool)
    empty_heads = 0
    for n, t, h, beg, end in _slot_ranges(crow, c["head_off"]):
        if end == beg:
            empty_heads += 1
            continue
        assert not bool(covered[n, beg:end].any())
        covered[n, beg:end] = True
        v = buf[n, beg:end]
        assert bool(torch.isfinite(v).all()) and float(v.min()) >= 0.0 and float(v.max()) <= float(c["rs"][n, h, t]), (n, t, h)
    assert torch.equal(covered, buf != SENT)
    per_head = c["head_off"][..., 1:] - c["head_off"][..., :-1]
    if heavy:
        assert empty_heads > 0 and int(per_head[N - 1, :, 1].max()) == 0     # the empty head: nothing of its own to write
    if T_src == 517:
        assert bool((per_head % 4 != 0).any())                               # padded slots behind a head's last entry


@pytest.mark.parametrize("i", range(len(CASES_A)), ids=IDS)
def test_fused_decode_probs_match_fp64(i):
    c = _case(i)
    ref = _reference_probs(i)
    worst_parent = worst = 0.0
    seen = 0
    for n, t, h, beg, end in _slot_ranges(c["crow"], c["head_off"]):
        if end == beg:
            assert (n, h, t) not in ref
            continue
        want = ref[n, h, t]
        assert want.numel() == end - beg
        got = c["buf"][n, beg:end].double()
        worst = max(worst, float((got - want).abs().max()))
        worst_parent = max(worst_parent, float((c["parent"][n, beg:end].double() - want).abs().max()))
        total = float(got.sum())
        assert abs(total - float(c["rs"][n, h, t])) <= TOL_P * (end - beg), (n, t, h, total)
        seen += 1
    print(f"[decode-probs] {IDS[i]}: max|err| vs fp64: fused decode {worst:.3e}, emit + plain kernel {worst_parent:.3e}")
    assert seen > 0 and worst <= TOL_P, worst


# ---- 4. paged ------------------------------------------------------------------------------------------------------------
PAGED = [(torch.float16, 64, 257, 16, 61, False), (torch.bfloat16, 80, 257, 16, 61, False), (torch.float16, 128, 257, 16, 61, False),
         (torch.bfloat16, 64, 3000, 64, 341, True), (torch.float16, 80, 3000, 64, 341, True), (torch.bfloat16, 128, 3000, 64, 341, True)]


@pytest.mark.parametrize("dtype,d,T_src,k,keep_count,heavy", PAGED,
                         ids=[_case_id((c[0], c[1], 1) + c[2:]) for c in PAGED])
def test_paged_decode_probs_equal_contiguous(dtype, d, T_src, k, keep_count, heavy):
    page_rows, N, H, T_dst = 64, 2, 4 if heavy else 8, 1
    T_cap = -(-(T_src + 40) // page_rows) * page_rows
    sel, _mask = _selection(dtype, N, H, T_dst, T_src, k, keep_count, heavy, seed=T_src + d)
    z_cap = max(int(sel.crow[:, -1].max().item()), 1)
    kk, vv = _caches(N, H, T_src, T_cap, d, dtype)
    q = (torch.randn((N, H, T_dst, d), device=DEV) * d ** -0.5).to(dtype)
    rs = torch.rand((N, H, T_dst), device=DEV) * 0.5 + 0.5
    ts = torch.full((N, 1), T_src, dtype=torch.int32, device=DEV)
    # the rows scattered into a shuffled pool (three pages more than the sequences name)
    n_tab = T_cap // page_rows
    P = N * n_tab + 3
    g = torch.Generator().manual_seed(T_src + d)
    table = torch.randperm(P, generator=g)[:N * n_tab].view(N, n_tab)
    pool = torch.full((2, P, H, page_rows, d), float("nan"), dtype=dtype, device=DEV)
    idx = table.reshape(-1).to(DEV)
    pool[0, idx] = kk.view(N, H, n_tab, page_rows, d).transpose(1, 2).reshape(N * n_tab, H, page_rows, d)
    pool[1, idx] = vv.view(N, H, n_tab, page_rows, d).transpose(1, 2).reshape(N * n_tab, H, page_rows, d)
    table = table.to(torch.int32).to(DEV)
    hc, hp = _handle(sel, H, T_cap, k, z_cap, ts, True), _handle(sel, H, T_cap, k, z_cap, ts, True)
    bc, bp = _sentinel(N, z_cap), _sentinel(N, z_cap)
    oc, _ = ops.sparse_attention(q, kk, vv, hc, row_scale=rs, path="gather", keep_columns_pending=True, probs_out=bc)
    op, _ = ops.sparse_attention(q, pool[0], pool[1], hp, row_scale=rs, path="gather", keep_columns_pending=True, probs_out=bp,
                                 block_table=table)
    assert hc.col_is_pending and hp.col_is_pending
    assert torch.isfinite(op).all() and torch.equal(op, oc)
    assert torch.equal(bp, bc)
    z = sel.crow[:, -1].cpu()
    assert all(bool((bp[n, :int(z[n])] != SENT).all()) and bool((bp[n, int(z[n]):] == SENT).all()) for n in range(N))


# ---- 5. a sequence that sits out -----------------------------------------------------------------------------------------
SITS_OUT = [3, 6, 9, 10, 14, 15]          # decode1 (d = 64 heavy, d = 80 ragged totals), DEC rows 3 (d = 80) and 8 (d = 128), fp32 rows 1 and 3


@pytest.mark.parametrize("i", SITS_OUT, ids=[IDS[i] for i in SITS_OUT])
def test_sitting_out_sequence_writes_nothing(i):
    dtype, d, T_dst, T_src, k, keep_count, heavy = CASES_A[i]
    c = _case(i)
    N, H, T_cap, z_cap, sel, q, kk, vv = (c[x] for x in ("N", "H", "T_cap", "z_cap", "sel", "q", "kk", "vv"))
    rs = c["epi"]["row_scale"]
    ts = torch.tensor([[~T_src], [T_src]], dtype=torch.int32, device=DEV)   # sequence 0 sits out (DecodeSession's complement form)
    both, alone = _handle(sel, H, T_cap, k, z_cap, ts, True), _handle(sel, H, T_cap, k, z_cap, ts[1:2], True, items=(1, 2))
    bb, ba = _sentinel(N, z_cap), _sentinel(1, z_cap)
    ob, _ = ops.sparse_attention(q, kk, vv, both, row_scale=rs, path="gather", keep_columns_pending=True, probs_out=bb)
    oa, _ = ops.sparse_attention(q[1:2], kk[1:2], vv[1:2], alone, row_scale=rs[1:2].contiguous(), path="gather",
                                 keep_columns_pending=True, probs_out=ba)
    assert both.col_is_pending and alone.col_is_pending
    assert bool((ob[0] == 0).all()) and bool((bb[0] == SENT).all())
    assert torch.equal(ob[1:2], oa) and torch.equal(bb[1:2], ba)
    assert bool((ba[0, :int(c["crow"][1, -1])] != SENT).all())
