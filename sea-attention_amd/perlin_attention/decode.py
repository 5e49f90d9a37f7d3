"""Single-token decoding of one SEA attention layer as a replayed HIP graph.

The reference generates one position per forward (src/main/opt_generate.py:131 -> the `use_cache` branches of
perlin_attention/attention.py + attention_state.py).  `PerlinAttention._forward_cached` is that path on the HIP
kernels: a dozen launches per position whose arguments change with the position (T_src, the value-embedding row, K_t,
tensor shapes that grow), so the step is bound by the host enqueueing them.

`DecodeSession` freezes everything position-dependent into DEVICE memory instead:

  * K / V caches of a fixed capacity; the new row is written at a device-resident index,
  * the Performer state image and the predictor CNN's window are updated in place,
  * the three kernels that need the position read it from a device int32
    (the decode forms of `sea_performer_causal_step`, `sea_predictor_tail_select`, `sea_csr_emit`, include/sea_hip.h),
  * column ids are encoded against the cache capacity, so the fused attention launch has static arguments.

The whole step is then captured ONCE with `torch.cuda.graph` and replayed per token.  Round 4: the framework glue around
the kernels (three input copies, index_copy_, cat + copy of the CNN window, row scan, two counter adds: eleven ~4.5 us
launches, 50 of a position's 130 us) is two launches now -- `sea_decode_stage` in front of the replay (the only launch whose
arguments change: it takes the caller's q row and appends k / v to the caches) and `sea_c8_window_shift` at its end (it
also advances the two device counters); the MLP writes the new CNN row straight behind the window and the tail + selection
launch writes the one-row `crow` itself.  Results are bitwise those of `_forward_cached` called position by position
(tests/test_decode_session.py).

Round 5: conv1, conv2, tail + selection and the window shift -- four launches, 37 of a position's 95 us at batch 1, all of it
fixed cost (each convolution staged its 74 KB weight image into LDS to convolve a 25-row window of which one row is new) --
are ONE launch, `sea_decode_cnn_tail_select`: a workgroup per sequence computes the one new row of each convolution (the
earlier rows it needs, t - 2 and t - 4, live in two small rings: the MLP's previous outputs and conv1's previous outputs),
runs the unchanged tail + selection on it and advances the device counters.  Nothing is shifted any more: a ring slot is
position % ring size.  Still bitwise (`csrc/sea_convfrag.hpp: conv_row_c8` reproduces the convolution kernel's operand
placement and k order).  Shapes outside that kernel (three-convolution bodies, H > 40) keep the round-4 launches.
Round 5, later: the attention launch of a position is the decode form of `sea_sparse_attention` -- the gather kernel expands the one
row's kept pixels itself (row widths from the device counter), its idle lane groups warm the K / V rows of the expanded lists
-- so the CSR row's column ids are not on the critical path any more (no emit phase / launch; `session.csr.col` emits on
its first read after each step: a replayed step re-arms the handle).  `fused_attention=False` keeps the emit + unfused launch
pair (bitwise the same context).  Column ids are head * capacity + key, and the capacity never changes a bit: a thinned
pixel's keys are stepped in fp32 on the key alone, the head offset is added as an integer (include/sea_hip.h, sea_csr_emit).

Sequences at different positions (`DecodeSession.from_sequences`): the counters are an (N, 3) block, a row per sequence, and
every launch of the step takes their row stride (the per-sequence form of its operator, include/sea_hip.h).  Each of those
kernels serves one sequence per workgroup, so a sequence's position is one scalar load from its row; the step is bitwise N
sessions of N = 1.
`admit` puts a new prompt into one slot between steps (continuous batching) without a new capture: the graph holds pointers
to the session's buffers only.

Paged K / V (`from_sequences(..., page_rows=...)`): one pool of fixed-size pages, (2, P, H, page_rows, D), shared by all
slots, and a device block table (N, ceil(capacity / page_rows)) int32 naming each sequence's pages in order.  Pages are
handed out on the host: seeding or `admit` gives a slot the pages of its prefix plus the next row, `step` a new page to
every slot whose next row starts one (written into the device table in stream order, no host synchronise).  The three
launches that touch K / V take the block table as an argument; keys and column ids stay logical (head * capacity + key), so
every result is bitwise the contiguous ragged session's.  page_rows is a power of two and a multiple of the Performer chunk: the
rows a chunk-aligned step walks again lie in one page.
Who owns what: `PageAllocator` is the pool's free list and holder counts; `SlotPages` (host only, no torch) owns the slots'
page lists and every decision about them -- what seeding, `admit`, `step`, `extend`, `release`, `fork` and `reorder` take,
share and give back, and each refusal, made before anything changes (tests/test_decode_slot_pages.py runs it without a
GPU).  `DecodeSession` owns the device: it applies what `SlotPages` returns to the block table and the pool, and keeps
`lengths`, the paused / empty flags and the counter rows.  `session.pages` and `session.allocator` are `SlotPages`' own.

Fork and beam reorder (`fork`, `reorder`; paged ragged sessions, between steps): during a step only the stage writes K / V, row
`seen` of each slot, in the slot's last ("open") page; every page below it is immutable while the sequence lives.  So a slot
may continue as a copy of another by sharing that slot's closed pages (the allocator counts holders) and copying only its
small state -- Performer image slice, rings, counter row, block-table row -- and its open page: one `sea_decode_fork` call
(include/sea_hip.h), snapshot semantics for swaps, cycles and many-to-one parent maps.

Multi-token steps and rewind (`from_sequences(..., max_step_rows=S)`, contiguous K / V, S <= 8): `step` takes s = 1 .. S new
rows of every slot, (N, H, s, D) -> context (N, s, H*D), and `rewind(drop)` removes the last drop[n] rows of that step from
slot n again (speculative decoding: the target verifies a draft's s tokens in one step and drops the rejected ones).  A graph
per distinct s, captured on first use over views of buffers allocated once for S.  The per-sequence forms of the Performer,
the MLP, the attention and the emit take s rows already; `sea_decode_stage` takes them through its `rows` argument and
`sea_decode_cnn_tail_select` through its multi-row form (`y1_scratch`: a workgroup per (sequence, row), recomputing the conv1
rows of this step that its row needs into its own scratch).  Rewind is host work plus one counter copy: the rings keep
LB + S x rows and 2 dil + S conv1 rows, so a slot read after any rewind is still where it was, K / V rows past the kept length are overwritten by the next stage before
anything reads them, and the Performer image -- which changes only when a chunk completes, at most once per step (s <= 8 <=
chunk) -- is copied aside before a step that completes one and copied back when the rewind falls below that boundary.  A
rewound slot is bitwise a plain session that stepped only the kept rows.

Slots that sit out steps (`pause`, `resume`, `release`; `None` entries of `from_sequences`; ragged sessions): the captured
graph has a fixed grid and static arguments, so "slot n does nothing this step" is a fact in device memory -- the slot's
counter row holds the bitwise complement of its values, (~seen, ~tsrc, ~tsrc_done): negative, which no live sequence reaches,
and every launch that carries per-sequence state already loads one of the three.  Its workgroups leave by a block-uniform
early-out on that scalar: the stage writes no K / V row, the Performer touches neither the image nor a page, the CNN launch
leaves the rings alone and writes an empty selection row (crow [0, 0], so the emit writes nothing), the attention stores zeros
(include/sea_hip.h, at each entry).  The CNN workgroup still takes its ticket -- the last one advances the counters and resets
the ticket -- and the advance skips negative rows.  The true position lives in the host mirror `lengths`; `pause` / `resume`
/ `release` rewrite the counter block with one small stream-ordered copy, as `rewind` does, so `captures` does not move.  A
paused slot keeps everything (a parked prompt: `pause` it, `fork` from it as requests arrive -- `sea_decode_fork` decodes the
source's `seen` for the open page and copies the counters as they are, so the copy is paused too -- then `resume` the copies);
`release` also drops the sequence and gives its pages back: the slot is EMPTY (counters ~0, length 0) until `admit`, `fork` or
`reorder` fills it.  Capacity and page growth look at the slots that take part only.  The slots that do take part are
bitwise what they are without the others (tests/test_gpu_decode_pause.py).  The emit + unfused attention pair
(`fused_attention=False`) knows only an empty CSR row, whose context is the average mix; there the zeros of sitting-out slots
are small fills behind the step.

Many rows into one slot between steps (`extend(slot, q, k, v)`; ragged sessions, eager, no capture): a forked request is the
shared prompt plus a suffix of its own, tens to hundreds of rows.  One row per replayed step is s replays; the cached forward
followed by `admit` re-seeds all L + s rows into fresh pages, and the slot stops sharing its parent's closed pages.  `extend`
runs the module's cached forward over the s rows against the slot's K / V, continued from the slot's own image and window --
DESIGN section 8: that path is bitwise the stateless forward for any piece sizes, and a step is that path one position at a
time, so the rows and every later step are bitwise what one-row steps give -- and files the result with ONE launch,
`sea_decode_append_rows`: K / V rows L .. L+s-1 into the slot's pages, the window and conv1 over it into the rings at
position % ring (what `_seed_slot` files for a prefix of L + s rows), the image slice, the counter row (the complement form when
the slot is paused: it stays paused).  The forward reads contiguous K / V: a paged slot's rows are gathered through its device
table row into a per-session scratch (`sea_decode_gather_rows`, no host-built index), a contiguous session hands out a view
of its cache.  Only rows >= L are written -- the open page and new pages, taken before anything is launched; table entries
below the open index, the closed pages a fork shares, are untouched.  The parked-prompt flow, complete: `pause` the prompt,
`fork` it as requests arrive, `extend` each copy by its request's rows, `resume` the copies, `release` them at EOS.

The attention probabilities of a step (`attention_probs=True` at construction, off by default): the module's
`partial_attention_probs` -- the per-entry row_scale * softmax values of the sparse attention, a `FlatCSR` with values -- from
the replayed step itself.  The session owns one static fp32 buffer, (N, z_cap), or (N, S * z_cap) with `max_step_rows` S, and
every attention launch of a step takes it as `probs_out` (`ops.sparse_attention`): the decode forms of `sea_sparse_attention`
write each entry's value at the slot its column has -- or would have: the columns stay pending -- so the capture holds no
extra launch and no fill node.  After every `step`, `session.attention_probs` is `session.csr.with_values(view of the buffer)`,
a new handle per step over the step's own structure (a replay re-arms `session.csr`; a handle kept from an earlier step sees
the buffer as later steps leave it).  Reading its `.col` / `.col_indices()` emits the columns exactly as `session.csr` does;
`.values()`, `.col_indices()` and `.crow_indices()` are the cached forward's `partial_attention_probs` for that position, bit for
bit (tests/test_gpu_decode_session_probs.py).  Slots that sit out have empty rows (their launch writes nothing).  The
probabilities are an OUTPUT of the last step, not state: `rewind`, `fork`, `reorder`, `extend` and `admit` neither read nor
change them.  Off (the default): no buffer, the same launches, the same `captures`, and `session.attention_probs` is None.
"""
from collections import deque
from typing import List, Optional

import torch

from .. import _lib
from . import ops
from .attention_state import CnnWindowState, CumAvgState, PerformerState, PerlinAttentionState, cnn_lookback


def _cnn_convs(at):
    """The predictor CNN body's convolutions (CausalConv2d modules)."""
    body = list(at.attention_predictor_cnn[1].module.net.children())
    return [body[i].module for i in range(0, len(body) - 2, 2)]


def _fused_cnn_ok(convs, C, H, T_M, dt, LB) -> bool:
    """Does `sea_decode_cnn_tail_select` serve this predictor (two 3 x 3 width-preserving convolutions of one dilation)?"""
    return (len(convs) == 2 and all(c.kernel_size == 3 and c.in_channels == C and c.out_channels == C
                                    and isinstance(c.dilation, int) and c.dilation == convs[0].dilation
                                    and c.padding[1] == c.dilation for c in convs)
            and ops.decode_cnn_supported(C, H, T_M, dt) and LB >= 4 * convs[0].dilation)   # (the y1 ring's seed: 2 dil rows)


def _predictor_length_error(T_M) -> Optional[str]:
    """Why a session cannot run at predictor length T_M (None: it can).  Two kernels of a position set the limit: the fused
    CNN launch convolves a row of W4 = T_M / 4 pixels in one pass (`ConvRowC8`: W4 <= 64), and the one-row decode attention
    keeps a row's pixel bounds for T_m <= 256.  Below that the reference's grid is served (`ops.DECODE_PREDICTOR_LENGTHS`: the
    lengths the fused CNN launch is instantiated and tested for)."""
    if T_M > 256:
        return (f"a decode session runs at predictor lengths T_M <= 256 (got T_M = {T_M}): W4 = T_M / 4 <= 64 in ConvRowC8 "
                "(one pass per row), T_m <= 256 in the one-row decode attention")
    if T_M not in ops.DECODE_PREDICTOR_LENGTHS:
        return (f"a decode session runs at the predictor lengths {' / '.join(str(t) for t in ops.DECODE_PREDICTOR_LENGTHS)} "
                f"(got T_M = {T_M})")
    return None


class PageAllocator:
    """Free list of a paged K / V pool's pages (host only; the device block table is the session's business).  Pages go out
    lowest index first at the start; pages given back are handed out again before any never-used one (most recently
    returned first), so a slot that is re-admitted reuses the pages it gave back.
    A page that is out has one or more holders (`share` adds one: a closed page named by several block tables after a fork);
    `give_back` drops one holder per page, and the page returns to the free list when its last holder gives it back."""

    def __init__(self, pool_pages: int):
        if pool_pages < 1:
            raise ValueError(f"a pool of {pool_pages} pages")
        self.pool_pages = int(pool_pages)
        self._free = deque(range(self.pool_pages))
        self._holders = {}                                                   # page -> holders (pages that are out)

    @property
    def free_pages(self) -> int:
        return len(self._free)

    def holders(self, page: int) -> int:
        """How many holders page `page` has (0: it is free)."""
        return self._holders.get(page, 0)

    def take(self, count: int) -> List[int]:
        """`count` pages, or RuntimeError (and nothing taken) when fewer are free."""
        if count > len(self._free):
            raise RuntimeError(f"page pool exhausted: {count} page(s) wanted, {len(self._free)} of {self.pool_pages} free")
        pages = [self._free.popleft() for _ in range(count)]
        for pg in pages:
            self._holders[pg] = 1
        return pages

    def share(self, pages) -> None:
        """One more holder for each of `pages` (a page may be named more than once); a page that is not out is refused
        with ValueError before any of them changes."""
        pages = list(pages)
        bad = [pg for pg in pages if pg not in self._holders]
        if bad:
            raise ValueError(f"pages {bad} are not out of this pool: only a page that is out can be shared")
        for pg in pages:
            self._holders[pg] += 1

    def give_back(self, pages) -> None:
        """Drop one holder of each page taken or shared before; a page named more often than it has holders (a double free,
        a foreign index) is refused with ValueError before any of them changes."""
        pages = list(pages)
        count = {}
        for pg in pages:
            count[pg] = count.get(pg, 0) + 1
        bad = [pg for pg, c in count.items() if c > self._holders.get(pg, 0)]
        if bad:
            raise ValueError(f"pages {bad} are not out of this pool (double free?)")
        for pg in reversed(pages):
            self._holders[pg] -= 1
            if self._holders[pg] == 0:
                del self._holders[pg]
                self._free.appendleft(pg)


class SlotPages:
    """Which pages of the pool each slot of a paged session names, and every decision about them: host only, plain lists,
    no torch.  `pages[n]` is slot n's pages in order (the host mirror of row n of the device block table, `n_tab` entries
    wide); `DecodeSession` applies what these methods return to the device.  A refusal (RuntimeError) has changed nothing."""

    def __init__(self, slots: int, capacity: int, page_rows: int, pool_pages: Optional[int] = None):
        self.page_rows, self.capacity = int(page_rows), int(capacity)
        self.n_tab = self.count(self.capacity)
        self.allocator = PageAllocator(slots * self.n_tab if pool_pages is None else pool_pages)
        self.pages = [[] for _ in range(slots)]

    def count(self, rows: int) -> int:
        """Pages that hold `rows` rows."""
        return -(-rows // self.page_rows)

    @property
    def free_pages(self) -> int:
        return self.allocator.free_pages

    def shared(self) -> List[int]:
        """The pages more than one slot holds, ascending."""
        return sorted({pg for row in self.pages for pg in row if self.allocator.holders(pg) > 1})

    def reclaimable(self, n: int) -> int:
        """Pages slot n gives back to the free list when it lets go of them: those it is the last holder of."""
        return sum(1 for pg in self.pages[n] if self.allocator.holders(pg) == 1)

    def open_page(self, n: int, L: int) -> int:
        """The page row L of slot n lies in (the slot's next row, when it stands at L), or -1: that row starts a new page."""
        o = L // self.page_rows
        return self.pages[n][o] if o < len(self.pages[n]) else -1

    def reseat(self, n: int, L: int) -> List[int]:
        """Slot n starts over on a prefix of L rows: its pages go back first, then it takes count(L + 1) -- the prefix and
        the row of the next step -- and returns them."""
        count, free, own = self.count(L + 1), self.free_pages, self.reclaimable(n)
        if count > free + own:
            raise RuntimeError(f"page pool exhausted: slot {n} needs {count} pages for a prefix of {L} rows, {free} free + {own} of its own")
        self.allocator.give_back(self.pages[n])
        self.pages[n] = self.allocator.take(count)
        return self.pages[n]

    def grow(self, lengths, sitting):
        """Before a step: a page for every slot that takes part and whose next row starts one.  Returns the new table
        entries [(slot, table index, page)]; RuntimeError naming the slots when the pool has too few."""
        want = [n for n, L in enumerate(lengths) if not sitting[n] and L >= len(self.pages[n]) * self.page_rows]
        if len(want) > self.free_pages:
            raise RuntimeError(f"page pool exhausted: slot(s) {want} need a new page, {self.free_pages} free")
        new = [(n, len(self.pages[n]), pg) for n, pg in zip(want, self.allocator.take(len(want)))]
        for n, _, pg in new:
            self.pages[n].append(pg)
        return new

    def extend_take(self, n: int, L: int, s: int) -> List[int]:
        """The pages slot n lacks for s more rows behind its L, up to the row of the next step and within the table.  They
        are taken but not yet slot n's: the session appends them to `pages[n]` once the rows are written, or `cancel`s them."""
        pg = self.open_page(n, L)
        if self.allocator.holders(pg) > 1:
            raise RuntimeError(f"extend: slot {n}'s open page {pg} has other holders; only closed pages are shared (fork gives "
                               "every copy an open page of its own)")
        want = self.count(min(L + s + 1, self.capacity)) - len(self.pages[n])
        if want > self.free_pages:
            raise RuntimeError(f"page pool exhausted: slot {n} needs {want} new page(s) for {s} more rows, {self.free_pages} free")
        return self.allocator.take(max(want, 0))

    def cancel(self, fresh) -> None:
        """Pages taken by `extend_take` / `move_plan` go back: the launch they were for did not happen."""
        self.allocator.give_back(list(fresh))

    def release(self, n: int) -> None:
        self.allocator.give_back(self.pages[n])
        self.pages[n] = []

    def move_plan(self, moves, lengths):
        """fork / reorder, before the launch.  moves: [(src, dst)], dst := src as it is now: the source's pages below its
        open page, shared, and a copy of the open page when there is one.  Returns dst -> (the source's open page, the fresh
        page of its copy) for those; every fresh page is taken here, before any old page goes back, so that no page the move
        frees is the target of a copy."""
        copies = [(dst, self.open_page(src, lengths[src])) for src, dst in moves]
        copies = [(dst, pg) for dst, pg in copies if pg >= 0]
        if len(copies) > self.free_pages:
            raise RuntimeError(f"page pool exhausted: slot(s) {[dst for dst, _ in copies]} need a copy of their source's open page, "
                               f"{self.free_pages} free")
        return {dst: (pg, new) for (dst, pg), new in zip(copies, self.allocator.take(len(copies)))}

    def move_commit(self, moves, lengths, new_open) -> None:
        """After the launch (`lengths` as `move_plan` saw them): the destinations' rows from a snapshot (swaps, cycles,
        many-to-one); shares before give-backs (a source's closed pages may be held by a moved slot only)."""
        old = [list(p) for p in self.pages]
        for src, dst in moves:
            closed = old[src][:lengths[src] // self.page_rows]
            self.allocator.share(closed)
            self.pages[dst] = closed + ([new_open[dst][1]] if dst in new_open else [])
        for _, dst in moves:
            self.allocator.give_back(old[dst])


class DecodeSession:
    """Built from the state of a cached forward (`PerlinAttentionOutput.state`, HIP estimator: 16-bit inference) and the
    K / V prefix that forward saw.  `step(q, k, v)` takes the NEW row of each tensor, (N, H, 1, D), and returns the
    context row (N, 1, H*D) -- a static buffer, overwritten by the next step.
    `from_sequences` builds a session whose sequences sit at different positions (`ragged`; host mirror `lengths`)."""

    ragged = False               # (class defaults: a uniform session's instance attributes are what they always were)
    lengths = None
    paged = False                # (from_sequences(..., page_rows=...): K / V in a page pool, see the module docstring)
    page_rows = None
    block_table = None
    max_step_rows = None         # (from_sequences(..., max_step_rows=S): steps of 1 .. S rows and `rewind`)
    _last_step = None            # (what `rewind` may undo: (s, lengths before, slots whose image was copied aside))
    _paused = None               # (ragged sessions: host mirrors of the slots that sit out steps / hold no sequence)
    _empty = None
    _extend_kv = None            # (paged sessions: `extend`'s contiguous K / V scratch (2, H, capacity, D), allocated on first use)
    csr = None                   # (the CSR row of the last step; none while `from_sequences` seeds its slots)
    attention_probs = None       # (attention_probs=True: the last step's per-entry probabilities, a FlatCSR with values)
    _probs_buf = None            # (their static fp32 buffer, (N, z_cap) or (N, S * z_cap): `probs_out` of the attention launches)
    _want_attention_probs = False

    def __init__(self, attention, state: PerlinAttentionState, key_prefix: torch.Tensor, value_prefix: torch.Tensor,
                 capacity: int, use_graph: bool = True, fused_attention: bool = True, attention_probs: bool = False):
        at = self.attention = attention
        self._want_attention_probs = bool(attention_probs)
        pc = at.pconfig
        assert pc.causal and not at.training, "decoding is the causal inference path"
        N, H, L, D = key_prefix.shape
        assert value_prefix.shape == key_prefix.shape and key_prefix.is_cuda
        assert state is not None and state.seq_len == L, "the state must have seen exactly the prefix"
        LB = cnn_lookback(at.attention_predictor_cnn)
        ps = state.states.get(PerlinAttentionState.PERFORMER)
        cs = state.states.get(PerlinAttentionState.CNN)
        assert ps is not None and ps.image is not None and cs is not None and torch.is_tensor(cs.rows_c8), \
            "the session continues a state written by the HIP estimator (16-bit inference, supported head size)"
        assert cs.rows_c8.shape[1] == LB, f"the prefix must be at least the predictor CNN's reach ({LB} rows)"
        assert L < capacity <= at.v_eye_learned_causal.shape[2], "capacity: beyond the prefix, within the value embedding"
        self.N, self.H, self.D, self.capacity = N, H, D, int(capacity)
        self.T_M = int(pc.attention_predictor_length)
        self.k = int(pc.k)
        dev, dt = key_prefix.device, key_prefix.dtype
        assert dt in (torch.float16, torch.bfloat16)
        why = _predictor_length_error(self.T_M)
        if why is not None:
            raise ValueError(why)
        assert ops.decode_tail_select_supported(cs.rows_c8, H, self.T_M), \
            "fused tail + selection shape (the decode form: 16-bit data, H <= 64, a row that fits the kernel's LDS plan)"
        self.image = ps.image.clone()                                        # Performer sums, updated in place
        # CNN input rows: the window (last LB rows) and, behind it, the row of the current position -- ONE buffer, so that the
        # MLP writes the new row in place (no cat) and the window moves by an in-place shift at the end of the step
        self.LB = LB
        # round 5: the fused CNN + tail + selection launch (module docstring).  x ring: the MLP's rows of the last LB positions,
        # row of position p in slot p % LB (what `win` holds, by position instead of by age); y1 ring: conv1's rows of the last
        # positions (8 slots: t - 2 dil and t - 4 dil... t must sit in distinct slots for dilation 2)
        convs = _cnn_convs(at)
        C = cs.rows_c8.shape[2] * 8
        self.fused_cnn = _fused_cnn_ok(convs, C, H, self.T_M, dt, LB)
        if self.fused_cnn:
            dil, RY = convs[0].dilation, 2 * 2 * convs[0].dilation + 1      # t, t - dil, t - 2 dil in distinct slots: 9 for dil 2
            row_shape = tuple(cs.rows_c8.shape[2:])
            pos = torch.arange(L - LB, L, device=dev)
            self.x_ring = torch.zeros((N, LB) + row_shape, dtype=dt, device=dev)
            self.x_ring[:, pos % LB] = cs.rows_c8                            # window row i is position L - LB + i
            self.y1_ring = torch.zeros((N, RY) + row_shape, dtype=dt, device=dev)
            y1, keep_rows = self._conv1_seed(cs.rows_c8)
            p1 = torch.arange(L - keep_rows, L, device=dev)
            self.y1_ring[:, p1 % RY] = y1[:, LB - keep_rows:]
            self.x_new = torch.zeros((N, 1) + row_shape, dtype=dt, device=dev)   # where the MLP writes the new row
            self.y2 = torch.zeros((N,) + row_shape, dtype=dt, device=dev)
            self.ticket = torch.zeros((1,), dtype=torch.int32, device=dev)
            self.xs = None
        else:                                                      # the round-4 launches: a window the step shifts by one row
            self.xs = torch.zeros((N, LB + 1) + tuple(cs.rows_c8.shape[2:]), dtype=dt, device=dev)
            self.xs[:, :LB] = cs.rows_c8
        # K and V caches are the two halves of ONE tensor and the two position counters two elements of one
        self.kv_cache = torch.zeros((2, N, H, capacity, D), dtype=dt, device=dev)
        self.k_cache, self.v_cache = self.kv_cache[0], self.kv_cache[1]
        self.k_cache[:, :, :L] = key_prefix
        self.v_cache[:, :, :L] = value_prefix
        # device counters: seen = rows the state has seen = cache row of the new token, tsrc = keys the new row sees; the
        # LAST launch of a step (the window shift) advances both
        # (third element, fused CNN launch only: T_src of the step that launch has just closed -- what the emit behind it reads)
        self.ctr32 = torch.tensor([L, L + 1, L + 1], dtype=torch.int32, device=dev)
        self.seen32 = self.ctr32[0:1]
        self.tsrc32 = self.ctr32[1:2]
        self.tsrc_done32 = self.ctr32[2:3]
        self.crow = torch.zeros((N, 2), dtype=torch.int32, device=dev)        # one-row CSR: [0, row total], written by the selection
        self.length = L                                                      # host mirror (bounds check only)
        self._static_buffers(dev, dt, fused_attention)
        if use_graph:
            self._capture()

    def _static_buffers(self, dev, dt, fused_attention):
        """What does not depend on the prefixes: the K_t table, the column bound, the step's input / output buffers."""
        at, N, H, D, capacity = self.attention, self.N, self.H, self.D, self.capacity
        # K_t of every reachable position (attention.py:849-866, the same fp32 expression as the stateless path) and
        # the largest CSR row any of them can emit
        keep_cpu, _ = at._decode_keep(H, capacity, capacity, self.T_M)
        self.keep_table = keep_cpu.to(dev)
        w = torch.arange(1, capacity + 1)
        per_pixel = torch.clamp_max(torch.div(w + self.T_M - 1, self.T_M, rounding_mode="floor"), self.k)
        bound = torch.minimum(keep_cpu.to(torch.long) * per_pixel, H * torch.minimum(w, torch.tensor(self.T_M * self.k)))
        self.z_cap = max(int(bound.max().item()), 1)
        self.q_in = torch.zeros((N, H, 1, D), dtype=dt, device=dev)
        self.ctx = torch.zeros((N, 1, H * D), dtype=at.context_layer_dtype or torch.float32, device=dev)
        self.fused_attention = bool(fused_attention)   # the attention launch's decode form (False: emit + the unfused launch)
        self.csr = None                                                      # the CSR row of the last step
        self._col_emit = None                                                # its pending-column state (graph replay re-arms it)
        self.graph: Optional[torch.cuda.CUDAGraph] = None
        self.probs = None                                                    # estimated attention probabilities of the last step
        if self._want_attention_probs:                                       # (module docstring: written in place, never cleared)
            self._probs_buf = torch.zeros((N, (self.max_step_rows or 1) * self.z_cap), dtype=torch.float32, device=dev)
        self._pinned, self._prep_generation = None, ops.prep_generation()

    @classmethod
    def from_sequences(cls, attention, sequences, capacity: int, use_graph: bool = True, fused_attention: bool = True,
                       page_rows: Optional[int] = None, pool_pages: Optional[int] = None, max_step_rows: Optional[int] = None,
                       attention_probs: bool = False):
        """A session over sequences of DIFFERENT lengths.  `sequences`: [(state, key_prefix, value_prefix), ...], each the
        output of an N = 1 cached forward, (1, H, L_i, D) with its own L_i.  Slot n of the batch is sequence n; `step` takes
        and returns (N, ...) rows as for a uniform session, and every row equals that sequence's own N = 1 session bit for
        bit.  Defined where the fused CNN launch runs (`ops.decode_cnn_supported`: two-convolution body, T_M in 64 / 96 / 128 /
        256 -- the reference's grid up to the 256 the decode kernels take --, H <= 40, 16-bit data); anything else raises
        ValueError, as do mismatched H / D / dtype, a prefix shorter than the CNN's reach
        and L_i >= capacity.
        `page_rows`: K / V in a pool of `pool_pages` pages of that many rows (default: enough for every slot at capacity; it
        may be far fewer), bitwise the contiguous session.  page_rows is a power of two and a multiple of the Performer chunk
        (`ops.performer_chunk_rows`: 64 at d = 64, 32 at d = 80 / 128); paging needs the fused decode attention
        (`fused_attention=True`, d in {64, 80, 128}).  ValueError otherwise, or when the prefixes do not fit the pool.
        `max_step_rows` S in 1 .. 8: `step` takes 1 .. S new rows per slot and `rewind` drops rows of the last step again
        (module docstring); contiguous K / V with the fused decode attention only (ValueError with `page_rows` or
        `fused_attention=False`).  None: one row per step, no rewind.
        An entry of `sequences` may be None: that slot starts EMPTY (as after `release`) and sits out until `admit`, `fork`
        or `reorder` fills it; at least one entry is a real sequence.
        `attention_probs`: every step also leaves the sparse attention's per-entry probabilities in `session.attention_probs`
        (module docstring)."""
        self = cls.__new__(cls)
        at = self.attention = attention
        self._want_attention_probs = bool(attention_probs)
        pc = at.pconfig
        seqs = list(sequences)
        if not (pc.causal and not at.training):
            raise ValueError("decoding is the causal inference path")
        real = [sq for sq in seqs if sq is not None]
        if not real:
            raise ValueError("from_sequences needs at least one (state, key_prefix, value_prefix): H, D, dtype and device "
                             "are those of the first real sequence")
        kp0 = real[0][1]
        if kp0.dim() != 4:
            raise ValueError("key / value prefixes are (1, H, L, D)")
        self.N, self.H, self.D, self.capacity = len(seqs), int(kp0.shape[1]), int(kp0.shape[3]), int(capacity)
        self.dtype = kp0.dtype
        if self.dtype not in (torch.float16, torch.bfloat16):
            raise ValueError(f"a ragged session runs on 16-bit data (got {self.dtype})")
        self.T_M, self.k = int(pc.attention_predictor_length), int(pc.k)
        why = _predictor_length_error(self.T_M)
        if why is not None:
            raise ValueError(why)
        self.LB = cnn_lookback(at.attention_predictor_cnn)
        convs = _cnn_convs(at)
        C = 2 * self.H                                                       # (the predictor's channel count: two per head)
        self.fused_cnn = _fused_cnn_ok(convs, C, self.H, self.T_M, self.dtype, self.LB)
        if not self.fused_cnn:
            raise ValueError("a ragged session needs the fused CNN launch: a two-convolution predictor body, T_M in "
                             f"{' / '.join(str(t) for t in ops.DECODE_PREDICTOR_LENGTHS)}, H <= 40 with H % 4 == 0, 16-bit data "
                             f"(got {len(convs)} convolutions, T_M = {self.T_M}, H = {self.H})")
        if not self.capacity <= at.v_eye_learned_causal.shape[2]:
            raise ValueError(f"capacity {self.capacity} beyond the value embedding ({at.v_eye_learned_causal.shape[2]} rows)")
        if max_step_rows is not None:
            if isinstance(max_step_rows, bool) or int(max_step_rows) != max_step_rows or not 1 <= max_step_rows <= 8:
                raise ValueError(f"max_step_rows {max_step_rows}: an integer in 1 .. 8")
            if page_rows is not None or not fused_attention:
                raise ValueError("multi-row steps run on contiguous K / V with the fused decode attention (no page_rows, "
                                 "fused_attention=True)")
            self.max_step_rows = int(max_step_rows)
        lengths = [0 if sq is None else self._check_sequence(*sq) for sq in seqs]       # (None: the slot starts empty)
        N, H, D, dt, dev = self.N, self.H, self.D, self.dtype, kp0.device
        if page_rows is not None:
            page_rows = int(page_rows)
            nb = at.performer.projection_matrix.shape[0]
            chunk = ops.performer_chunk_rows(D, nb, dt)
            if not fused_attention:
                raise ValueError("paged K / V runs on the fused decode attention (fused_attention=True): the unfused launches "
                                 "read contiguous caches only")
            if D not in (64, 80, 128) or chunk <= 0 or not ops.fused_interp_supported(dt, D, self.T_M):
                raise ValueError(f"paged K / V needs the one-row decode attention form (16-bit d = 64 / 80 / 128; got d = {D})")
            if page_rows < 1 or page_rows & (page_rows - 1) or page_rows % chunk:
                raise ValueError(f"page_rows {page_rows}: a power of two and a multiple of the Performer chunk ({chunk} rows)")
            sp = SlotPages(N, self.capacity, page_rows, pool_pages)
            need = sum(sp.count(L + 1) for L, sq in zip(lengths, seqs) if sq is not None)
            pool_pages = sp.free_pages                                       # (nothing is out yet)
            if pool_pages < need:
                raise ValueError(f"a pool of {pool_pages} pages of {page_rows} rows cannot hold the prefixes ({need} pages)")
        elif pool_pages is not None:
            raise ValueError("pool_pages goes with page_rows")
        self.ragged = True
        dil = convs[0].dilation
        row_shape = (C // 8, self.T_M // 4, 8)
        per = real[0][0].states[PerlinAttentionState.PERFORMER].image.numel()
        self.image = torch.zeros((N * per,), dtype=torch.float32, device=dev)          # sequence n's H images: the n-th slice
        S = self.max_step_rows
        if S is None:
            self.x_ring = torch.zeros((N, self.LB) + row_shape, dtype=dt, device=dev)
            self.y1_ring = torch.zeros((N, 2 * 2 * dil + 1) + row_shape, dtype=dt, device=dev)
            self.x_new = torch.zeros((N, 1) + row_shape, dtype=dt, device=dev)
            self.y2 = torch.zeros((N,) + row_shape, dtype=dt, device=dev)
        else:
            # rings that survive a rewind: the LB x rows an export reads and the 2 dil conv1 rows a step reads lie below the
            # kept length, the step wrote up to S positions above it.  Step buffers for S rows; an s-row step uses views
            self.x_ring = torch.zeros((N, self.LB + S) + row_shape, dtype=dt, device=dev)
            self.y1_ring = torch.zeros((N, 2 * dil + S) + row_shape, dtype=dt, device=dev)
            self.x_new = torch.zeros((N * S,) + row_shape, dtype=dt, device=dev)
            self.y2 = torch.zeros((N * S,) + row_shape, dtype=dt, device=dev)
            self.y1_scratch = torch.zeros((N * S * 2,) + row_shape, dtype=dt, device=dev)
            self.image_backup = torch.empty((N, per), dtype=torch.float32, device=dev)
            self.chunk = ops.performer_chunk_rows(D, at.performer.projection_matrix.shape[0], dt)
            self._graphs = {}                                                # s -> (graph, csr, pending emit, probs, ctx)
        self.ticket = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.xs = None
        if page_rows is not None:
            # the pool (2, P, H, page_rows, D): K pages and V pages share one page index; kv_cache names the pool (what the
            # stage writes and the capture saves), k_cache / v_cache its two halves (P, H, page_rows, D)
            self.paged, self.page_rows, self.slot_pages = True, page_rows, sp
            self.allocator, self.pages = sp.allocator, sp.pages            # (host mirror of the table: slot n's pages in order)
            self.block_table = torch.full((N, sp.n_tab), -1, dtype=torch.int32, device=dev)
            self.kv_cache = torch.zeros((2, pool_pages, H, page_rows, D), dtype=dt, device=dev)
        else:
            self.kv_cache = torch.zeros((2, N, H, self.capacity, D), dtype=dt, device=dev)
        self.k_cache, self.v_cache = self.kv_cache[0], self.kv_cache[1]
        # per-sequence counters: row n = [seen, tsrc, tsrc of the step just closed] of sequence n (the uniform session's
        # three, once per sequence); the launches take (N, k) views of it -- a counter per sequence
        self.ctr32 = torch.zeros((N, 3), dtype=torch.int32, device=dev)
        self.seen32, self.tsrc32, self.tsrc_done32 = self.ctr32[:, 0:1], self.ctr32[:, 1:2], self.ctr32[:, 2:3]
        self.crow = torch.zeros((N, 2), dtype=torch.int32, device=dev)
        self.lengths = list(lengths)                                         # host mirror (bounds checks; a sitting-out slot's position)
        self._paused = [sq is None for sq in seqs]                           # (an empty slot sits out like a paused one)
        self._empty = [sq is None for sq in seqs]
        for n, sq in enumerate(seqs):
            if sq is not None:
                self._seed_slot(n, *sq)
        if any(self._empty):
            self._write_counters()
        self._static_buffers(dev, dt, fused_attention)
        if S is not None:
            self.q_in = torch.zeros((N * H * S * D,), dtype=dt, device=dev)
            self.ctx = torch.zeros((N * S * H * D,), dtype=self.ctx.dtype, device=dev)
            self.use_graph = bool(use_graph)                                 # (graphs are captured per s, on first use)
        elif use_graph:
            self._capture()
        return self

    def _check_sequence(self, state, key_prefix, value_prefix) -> int:
        """One sequence of a ragged session, validated against the session's shape; returns its length."""
        if key_prefix.dim() != 4 or key_prefix.shape[0] != 1 or value_prefix.shape != key_prefix.shape:
            raise ValueError("each sequence is the output of an N = 1 cached forward: key / value prefixes (1, H, L, D)")
        if not key_prefix.is_cuda:
            raise ValueError("the prefixes live on the GPU")
        _, H, L, D = key_prefix.shape
        if (H, D, key_prefix.dtype, value_prefix.dtype) != (self.H, self.D, self.dtype, self.dtype):
            raise ValueError(f"every sequence has H = {self.H}, D = {self.D}, {self.dtype} "
                             f"(got H = {H}, D = {D}, {key_prefix.dtype} / {value_prefix.dtype})")
        if state is None or state.seq_len != L:
            raise ValueError("the state must have seen exactly its prefix")
        ps = state.states.get(PerlinAttentionState.PERFORMER)
        cs = state.states.get(PerlinAttentionState.CNN)
        if ps is None or ps.image is None or cs is None or not torch.is_tensor(cs.rows_c8):
            raise ValueError("the session continues a state written by the HIP estimator (16-bit inference, supported head size)")
        if cs.rows_c8.shape[0] != 1 or cs.rows_c8.shape[1] != self.LB or cs.rows_c8.shape[2] * 8 != 2 * H:
            raise ValueError(f"the prefix must be at least the predictor CNN's reach ({self.LB} rows)")
        nb = self.attention.performer.projection_matrix.shape[0]
        if ps.image.numel() * 4 != _lib.load().sea_performer_state_bytes(1, H, D, nb, _lib.dtype_code(self.dtype)):
            raise ValueError("the Performer state image is not one sequence's")
        if not L < self.capacity:
            raise ValueError(f"a prefix of {L} rows leaves no room in a capacity of {self.capacity}")
        return int(L)

    def _seed_slot(self, n, state, key_prefix, value_prefix):
        """Slot n of a ragged session := the sequence (state, prefixes): its Performer image, rings (slot = position % ring,
        seeded as a uniform session seeds them), cache rows and counters."""
        L, LB, RY = int(key_prefix.shape[2]), self.LB, self.y1_ring.shape[1]
        ps = state.states[PerlinAttentionState.PERFORMER]
        rows = state.states[PerlinAttentionState.CNN].rows_c8
        if self.paged:                                # first: a pool that cannot hold the prefix refuses with nothing changed
            self._seed_pages(n, key_prefix, value_prefix)
        self._flush_columns()
        self.image.view(self.N, -1)[n].copy_(ps.image.view(-1))
        pos = torch.arange(L - LB, L, device=rows.device)
        self.x_ring[n, pos % self.x_ring.shape[1]] = rows[0]
        y1, keep_rows = self._conv1_seed(rows)
        p1 = torch.arange(L - keep_rows, L, device=rows.device)
        self.y1_ring[n].zero_()
        self.y1_ring[n, p1 % RY] = y1[0, LB - keep_rows:]
        if not self.paged:
            self.kv_cache[:, n].zero_()
            self.k_cache[n, :, :L] = key_prefix[0]
            self.v_cache[n, :, :L] = value_prefix[0]
        self.ctr32[n] = torch.tensor([L, L + 1, L + 1], dtype=torch.int32)
        self.lengths[n] = L

    def _seed_pages(self, n, key_prefix, value_prefix):
        """Slot n of a paged session := the prefix: its old pages go back first, then ceil((L + 1) / page_rows) pages (the
        prefix and the row of the next step) take the prefix rows, zero behind them, and the device table row names them."""
        L, H, D, pr = int(key_prefix.shape[2]), self.H, self.D, self.page_rows
        pages = self.slot_pages.reseat(n, L)
        count, dev = len(pages), self.kv_cache.device
        rows = torch.zeros((2, H, count * pr, D), dtype=self.dtype, device=dev)
        rows[0, :, :L] = key_prefix[0]
        rows[1, :, :L] = value_prefix[0]
        idx = torch.tensor(pages, dtype=torch.long, device=dev)
        self.kv_cache[:, idx] = rows.view(2, H, count, pr, D).transpose(1, 2)
        self.block_table[n].fill_(-1)
        self.block_table[n, :count] = idx.to(torch.int32)

    @property
    def free_pages(self) -> Optional[int]:
        """Pages of the pool no slot holds (a paged session; None otherwise): what a scheduler may still admit or grow into.
        free_pages + the distinct pages the slots hold = the pool (a shared page counts once)."""
        return self.slot_pages.free_pages if self.paged else None

    @property
    def shared_pages(self) -> Optional[List[int]]:
        """The pages more than one slot holds (after `fork` / `reorder`: closed pages, never written again while they are
        shared), ascending; None when the session is not paged."""
        return self.slot_pages.shared() if self.paged else None

    def sequence_kv(self, slot: int):
        """Sequence `slot`'s logical K and V rows, (1, H, L, D) each (copies; a paged session gathers them from its pages):
        what a cached forward continues from, with `export_state(slot)`."""
        if not self.ragged:
            raise ValueError("sequence_kv: a ragged session (DecodeSession.from_sequences)")
        self._check_slot(slot)
        if self._empty[slot]:
            raise ValueError(f"sequence_kv: slot {slot} is empty (released, or never admitted)")
        L = self.lengths[slot]
        if self.paged:
            idx = torch.tensor(self.pages[slot], dtype=torch.long, device=self.kv_cache.device)
            kv = self.kv_cache[:, idx].transpose(1, 2).reshape(2, self.H, -1, self.D)[:, :, :L]
        else:
            kv = self.kv_cache[:, slot, :, :L]
        return kv[0:1].clone(), kv[1:2].clone()

    @torch.no_grad()
    def admit(self, slot: int, state: PerlinAttentionState, key_prefix: torch.Tensor, value_prefix: torch.Tensor):
        """Continuous batching: slot `slot` of a ragged session starts over on a new sequence (an N = 1 cached forward's
        state and prefixes), between two steps.  The other slots go on where they were; the captured graph stays (it holds
        pointers to the session's buffers, whose contents change here), so `captures` does not move.  A paged session
        gives the slot's pages back first; when the pool still cannot hold the new prefix it raises RuntimeError and leaves
        the slot as it was."""
        if not self.ragged:
            raise ValueError("admit: only a ragged session (DecodeSession.from_sequences) takes new sequences")
        self._check_slot(slot)
        self._check_sequence(state, key_prefix, value_prefix)
        self._seed_slot(slot, state, key_prefix, value_prefix)    # (a paged session: the refusal comes first, see there)
        self._paused[slot] = self._empty[slot] = False                       # (a paused or empty slot: active on the new sequence)
        self._last_step = None                        # (an admit ends the chance to rewind)

    @torch.no_grad()
    def extend(self, slot: int, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """Slot `slot` of a ragged session takes s >= 1 new rows at once, between two steps: q, k, v (1, H, s, D) -> the s context
        rows (1, s, H*D), a fresh tensor.  The rows are the module's cached forward (`PerlinAttention.forward(...,
        last_state=...)`) over the s rows against the slot's K / V, continued from the slot's own image and window, so they --
        and every later step -- are bitwise what one-row steps over the same rows give.  Eager: no capture, `captures` does not
        move.  Afterwards the slot stands at L + s with its Performer image, rings, K / V rows and counter row as `admit`
        leaves a prefix of L + s rows; an active slot stays active, a paused one paused (the parked prompt: `fork` the paused
        prompt, `extend` each copy by its request's own rows, `resume` them).  Every other slot keeps every bit.
        A paged session writes rows >= L only: the slot's table entries below its open page (the one row L lies in) -- the closed pages
        it may share with other slots -- are not touched; it takes the pages it lacks up to ceil((L + s + 1) / page_rows) (the
        prefix and the next step's row, as seeding does; no page beyond the table for a slot filled to capacity) before
        anything is launched, and its rows travel through a contiguous scratch of the session ((2, H, capacity, D), allocated at
        the first call): `sea_decode_gather_rows` in, `sea_decode_append_rows` out (include/sea_hip.h).
        It ends the chance to `rewind`.  Refused with nothing changed: a uniform session, an empty slot (that is `admit`'s),
        wrong shapes / dtype / device, L + s > capacity (ValueError); a slot out of range (IndexError); a pool that cannot
        supply the pages, or an open page another slot holds too (RuntimeError)."""
        if not self.ragged:
            raise ValueError("extend: only a ragged session (DecodeSession.from_sequences) extends one slot")
        slot = int(slot)
        self._check_slot(slot)
        if self._empty[slot]:
            raise ValueError(f"extend: slot {slot} is empty (released, or never admitted): admit or fork into it")
        H, D, L = self.H, self.D, self.lengths[slot]
        if not all(torch.is_tensor(t) and t.dim() == 4 for t in (q, k, v)) or k.shape != q.shape or v.shape != q.shape \
                or (q.shape[0], q.shape[1], q.shape[3]) != (1, H, D) or q.shape[2] < 1:
            raise ValueError(f"extend: q, k, v are (1, H, s, D) = (1, {H}, s, {D}) each with s >= 1 "
                             f"(got {[tuple(t.shape) if torch.is_tensor(t) else type(t).__name__ for t in (q, k, v)]})")
        if not all(t.dtype == self.dtype and t.device == self.kv_cache.device for t in (q, k, v)):
            raise ValueError(f"extend: {self.dtype} rows on {self.kv_cache.device}")
        s = int(q.shape[2])
        T = L + s
        if T > self.capacity:
            raise ValueError(f"extend: slot {slot} stands at {L} rows, {s} more pass the capacity of {self.capacity}")
        fresh = self.slot_pages.extend_take(slot, L, s) if self.paged else []
        at, dev = self.attention, self.kv_cache.device
        try:
            self._flush_columns()
            # contiguous K / V rows 0 .. T-1 for the forward: a paged slot's rows are gathered into the scratch, a contiguous
            # session's are its cache (the new rows are staged where they belong; rows >= L are read by nobody before)
            if self.paged:
                if self._extend_kv is None:
                    self._extend_kv = torch.empty((2, H, self.capacity, D), dtype=self.dtype, device=dev)
                kv = self._extend_kv
                ops.decode_gather_rows(self.kv_cache, self.block_table, self.capacity, slot, 0, L, kv)
            else:
                kv = self.kv_cache[:, slot]
            kv[0, :, L:T].copy_(k[0])
            kv[1, :, L:T].copy_(v[0])
            k_all, v_all = kv[0:1, :, :T], kv[1:2, :, :T]
            # the session's own image and window, as `export_state(slot)` hands them out (the image as a view: the Performer
            # step reads it and returns a new one)
            pos = torch.arange(L - self.LB, L, device=dev)
            st = self._state(self.image.view(self.N, -1)[slot], self.x_ring[slot:slot + 1, pos % self.x_ring.shape[1]], L)
            fp_min = torch.finfo(torch.float16).min / 2
            mask = torch.triu(torch.full((s, T), fp_min, dtype=self.dtype, device=dev), diagonal=L + 1).view(1, 1, s, T)
            out = at(q, k_all, v_all, q, k_all, v_all, q, k_all, mask, None, None, st)
            new_ps = out.state.states.get(PerlinAttentionState.PERFORMER)
            new_cs = out.state.states.get(PerlinAttentionState.CNN)
            if new_ps is None or new_ps.image is None or new_cs is None or not torch.is_tensor(new_cs.rows_c8) \
                    or new_cs.rows_c8.shape[1] != self.LB:
                raise ValueError("extend: the cached forward did not continue the session's state on the HIP estimator")
            window = new_cs.rows_c8.contiguous()
            y1, keep_rows = self._conv1_seed(window)                 # (the rows `_seed_slot` keeps: conv1's true values)
            if fresh:                                 # the new table entries: one small stream-ordered copy, no synchronise
                n0 = len(self.pages[slot])
                self.block_table[slot, n0:n0 + len(fresh)].copy_(torch.tensor(fresh, dtype=torch.int32).pin_memory(), non_blocking=True)
            row = [~T, ~(T + 1), ~T] if self._paused[slot] else [T, T + 1, T]
            nb = at.performer.projection_matrix.shape[0]
            paged = dict(kv_pool=self.kv_cache, block_table=self.block_table) if self.paged else {}
            ops.decode_append_rows(slot, L, s, kv[0, :, L:T] if self.paged else None, kv[1, :, L:T] if self.paged else None, window, y1,
                                   keep_rows, new_ps.image.view(-1), self.image, self.x_ring, self.y1_ring, self.ctr32, row,
                                   self.capacity, H, D, nb, **paged)
        except Exception:
            if fresh:                                 # (the host mirror `pages` has not moved: the slot is what it was)
                n0 = len(self.pages[slot])
                self.block_table[slot, n0:n0 + len(fresh)].fill_(-1)
                self.slot_pages.cancel(fresh)
            raise
        if fresh:
            self.pages[slot].extend(fresh)
        self.lengths[slot] = T
        self._last_step = None                        # (as an admit: the chance to rewind ends)
        return out.context_layer

    @torch.no_grad()
    def fork(self, src: int, dsts) -> None:
        """Parallel sampling: every slot in `dsts` drops what it held (as in `admit`) and continues as a copy of slot `src`:
        the same length, Performer image, CNN rings and counters.  Its block table names `src`'s closed pages -- shared,
        never copied -- and a private copy of `src`'s open page (the page the next row goes to; none when `src`'s last step
        filled a page: the next step gives every slot a page of its own).  Paged ragged sessions only, between steps, one
        `sea_decode_fork` call; the captured graph stays.  A copy of a paused slot is paused (`resume` it); an empty
        destination is filled.  Refused, with nothing changed: a slot out of range (IndexError), `src` in `dsts`, a
        repeated slot or an empty `src` (ValueError), too few free pages (RuntimeError naming the slots)."""
        self._require_paged("fork")
        dsts = [int(d) for d in dsts]
        for n in [src] + dsts:
            if not 0 <= n < self.N:
                raise IndexError(f"slot {n} outside 0..{self.N - 1}")
        if src in dsts or len(set(dsts)) != len(dsts):
            raise ValueError(f"fork({src}, {dsts}): the destinations are distinct slots other than the source")
        if self._empty[src]:
            raise ValueError(f"fork: slot {src} is empty (released, or never admitted): nothing to copy")
        parents = list(range(self.N))
        for d in dsts:
            parents[d] = src
        self._move(parents)

    @torch.no_grad()
    def reorder(self, parents) -> None:
        """Beam search (HF `_reorder_cache`): slot i continues as what slot `parents[i]` held before the call, for every i at
        once (swaps, cycles and many-to-one included).  Slots with parents[i] == i cost nothing.  Moved slots share their
        parent's closed pages and get a private copy of its open page, as in `fork`; the pages only the old contents of a
        moved slot held go back to the pool after the call has taken its new pages.  Refused, with nothing changed: a
        parent map of the wrong length or an empty parent of another slot (ValueError), a parent out of range (IndexError),
        too few free pages (RuntimeError).  Whether a slot is paused travels with its contents."""
        self._require_paged("reorder")
        parents = [int(p) for p in parents]
        if len(parents) != self.N:
            raise ValueError(f"reorder: {len(parents)} parents for {self.N} slots")
        for p in parents:
            if not 0 <= p < self.N:
                raise IndexError(f"parent slot {p} outside 0..{self.N - 1}")
        gone = sorted({p for i, p in enumerate(parents) if p != i and self._empty[p]})
        if gone:
            raise ValueError(f"reorder: parent slot(s) {gone} are empty (released, or never admitted): nothing to copy")
        self._move(parents)

    @property
    def paused(self) -> List[bool]:
        """Which slots sit out the steps (host mirror): paused ones, and empty ones -- `release` is a pause that also drops
        the sequence.  All False for a uniform session."""
        return list(self._paused) if self.ragged else [False] * self.N

    @property
    def empty(self) -> List[bool]:
        """Which slots hold no sequence (released, or built from a None entry) until `admit`, `fork` or `reorder` fills them."""
        return list(self._empty) if self.ragged else [False] * self.N

    def _check_slot(self, slot):
        if not 0 <= slot < self.N:
            raise IndexError(f"slot {slot} outside 0..{self.N - 1}")

    def _flush_columns(self):
        """The last step's pending columns follow the counters: emit them before the counters move."""
        if self.csr is not None and self.csr.col_is_pending:
            self.csr.col

    @staticmethod
    def _rearm(csr, col_emit):
        """After a replay: the handle of the capture is every replay's.  Its cached wire format is the first step's, and
        columns that no replayed launch writes are pending again (the emit launcher reads this step's bits / crow / counter)."""
        csr._wire = None
        if col_emit is not None:
            csr._pending = col_emit

    def _publish_attention_probs(self, s=1):
        """After a step of s rows: the step's structure with the buffer's values, a new handle (no wire format of an earlier
        step; pending columns follow `self.csr`, which the step has just re-armed)."""
        if self._probs_buf is not None:
            self.attention_probs = self.csr.with_values(self._probs_buf[:, :s * self.z_cap])

    def _conv1_seed(self, window):
        """What seeds the y1 ring behind a window of LB rows: conv1 over the window, and how many of its last rows are conv1's
        true values (all their taps lie inside the window)."""
        conv1 = _cnn_convs(self.attention)[0]
        dil = conv1.dilation
        y1 = ops.causal_conv_c8(window.contiguous(), conv1.weight, conv1.bias, 3, dil, dil, relu=True)
        return y1, min(self.y1_ring.shape[1] - 1, self.LB - 2 * dil)

    def _state(self, image, window, length) -> PerlinAttentionState:
        """The `PerlinAttentionState` a cached forward continues from: a Performer image and a CNN window at `length` rows."""
        st = PerlinAttentionState(self.attention)
        ps, cs, cav = PerformerState(), CnnWindowState(self.LB), CumAvgState()
        ps.image, ps.seq_index, cs.rows_c8 = image, length, window
        cav.prev_len, cav.in_image = length, True
        st.states = {PerlinAttentionState.PERFORMER: ps, PerlinAttentionState.CNN: cs, PerlinAttentionState.CUMAVG: cav}
        return st

    def _write_counters(self):
        """The device counter rows from the host mirrors, one small stream-ordered copy: [L, L + 1, L] for a slot that takes
        part (what a step leaves behind), the bitwise complement of each for one that sits out (the module docstring)."""
        rows = [[~L, ~(L + 1), ~L] if out else [L, L + 1, L] for L, out in zip(self.lengths, self._paused)]
        self.ctr32.copy_(torch.tensor(rows, dtype=torch.int32).pin_memory(), non_blocking=True)

    def _zero_sitting_rows(self, ctx):
        """The fused decode attention stores the zeros of a sitting-out slot itself.  The emit + unfused launch pair
        (`fused_attention=False`, head sizes without the fused form) knows an empty CSR row only, whose context is the
        average mix: there the zeros are small fills behind the step, for the sitting-out slots alone."""
        if any(self._paused) and not (self.fused_attention and ops.fused_interp_supported(self.dtype, self.D, self.T_M)):
            for n, out in enumerate(self._paused):
                if out:
                    ctx[n].zero_()

    def _between_steps(self, what, slots):
        """Common front of pause / resume / release: a ragged session, slots in range; returns them as a list."""
        if not self.ragged:
            raise ValueError(f"{what}: only a ragged session (DecodeSession.from_sequences) has slots that sit out steps; "
                             "a uniform session's sequences share one position")
        slots = [slots] if isinstance(slots, int) else list(slots)
        slots = [int(n) for n in slots]
        bad = [n for n in slots if not 0 <= n < self.N]
        if bad:
            raise IndexError(f"{what}: slot(s) {bad} outside 0..{self.N - 1}")
        return slots

    def _flags_changed(self):
        self._write_counters()
        self._last_step = None                        # (as an admit: the chance to rewind ends)

    @torch.no_grad()
    def pause(self, slots) -> None:
        """From the next step on the listed slots (one index or several) sit out: `step` ignores their input rows, returns
        zeros for them with an empty CSR row, and leaves their length, Performer image, CNN rings, K / V rows and pages as
        they are.  Between steps; no new capture.  Pausing a paused or empty slot changes nothing.  ValueError on a uniform
        session, IndexError for a slot out of range (nothing changed)."""
        slots = self._between_steps("pause", slots)
        self._flush_columns()
        for n in slots:
            self._paused[n] = True
        self._flags_changed()

    @torch.no_grad()
    def resume(self, slots) -> None:
        """The listed slots take part again from exactly where they stood.  A slot that is full gives `step`'s RuntimeError
        at the next step.  ValueError for an empty slot (there is nothing to resume: `admit` or `fork` into it), naming the
        slots, with nothing changed; otherwise as `pause`."""
        slots = self._between_steps("resume", slots)
        gone = [n for n in slots if self._empty[n]]
        if gone:
            raise ValueError(f"resume: slot(s) {gone} are empty (released, or never admitted): admit or fork into them")
        self._flush_columns()
        for n in slots:
            self._paused[n] = False
        self._flags_changed()

    @torch.no_grad()
    def release(self, slots) -> None:
        """A pause that also drops the sequence: the listed slots are EMPTY afterwards.  A paged session gives their pages
        back (a page another slot still shares stays out until its last holder lets go).  `admit`, or `fork` / `reorder`
        into the slot, fills it again; `resume`, `export_state`, `sequence_kv` and `fork` / `reorder` from it raise
        ValueError.  Releasing an empty slot changes nothing.  Errors as `pause`."""
        slots = self._between_steps("release", slots)
        self._flush_columns()
        for n in slots:
            if self.paged and self.pages[n]:
                self.slot_pages.release(n)
                self.block_table[n].fill_(-1)
            self._paused[n] = self._empty[n] = True
            self.lengths[n] = 0
        self._flags_changed()

    def _require_paged(self, what):
        if not (self.ragged and self.paged):
            raise ValueError(f"{what}: paging is required (DecodeSession.from_sequences(..., page_rows=...)): slots share "
                             "closed pages and copy only their small state and the open page")

    def _move(self, parents):
        """Slot i := slot parents[i] as it was before the call (fork / reorder); one `sea_decode_fork` call."""
        moves = [(p, i) for i, p in enumerate(parents) if p != i]
        if not moves:
            return
        sp = self.slot_pages
        new_open = sp.move_plan(moves, self.lengths)          # (refused here, or every copy's fresh open page is taken)
        dsts = {dst for _, dst in moves}
        rows, n_staged = [], 0
        for src, dst in moves:
            stage = -1
            if src in dsts:                           # (its state is overwritten by this call: read from a staged copy)
                stage, n_staged = n_staged, n_staged + 1
            rows.append((src, dst, *new_open.get(dst, (-1, -1)), stage))      # (the source's open page, its copy's page)
        dev = self.kv_cache.device
        nb = self.attention.performer.projection_matrix.shape[0]
        staging = None
        if n_staged:
            per = ops.decode_fork_staging_bytes(self.image.numel() // self.N * 4, self.x_ring[0].numel() * self.x_ring.element_size(),
                                                self.y1_ring[0].numel() * self.y1_ring.element_size(), sp.n_tab)
            staging = torch.empty((n_staged * per,), dtype=torch.uint8, device=dev)
        try:
            self._flush_columns()
            moves_dev = torch.tensor(rows, dtype=torch.int32).pin_memory().to(dev, non_blocking=True)   # (no host synchronise)
            ops.decode_fork(moves_dev, n_staged, self.image, self.x_ring, self.y1_ring,
                            self.ctr32, self.block_table, self.capacity, self.kv_cache, nb, staging)
        except Exception:
            sp.cancel(pg for _, pg in new_open.values())
            raise
        # host mirrors: from the snapshot
        # (whether a slot sits out belongs to its contents: the kernel copied the parent's counter row as it is, paused or not)
        sp.move_commit(moves, self.lengths, new_open)
        old_lengths, old_paused = list(self.lengths), list(self._paused)
        for src, dst in moves:
            self.lengths[dst] = old_lengths[src]
            self._paused[dst], self._empty[dst] = old_paused[src], False

    @property
    def win(self) -> torch.Tensor:
        """The predictor CNN's input rows of the last LB positions, oldest first, (N, LB, C/8, W, 8): a view of the shifted
        window (round-4 launches) or the ring read out by age (fused CNN launch; a copy)."""
        if self.ragged:                                            # (each sequence's ring by its own age)
            dev = self.x_ring.device
            pos = torch.tensor(self.lengths, device=dev).view(-1, 1) + torch.arange(-self.LB, 0, device=dev).view(1, -1)
            return self.x_ring[torch.arange(self.N, device=dev).view(-1, 1), pos % self.x_ring.shape[1]]
        if self.fused_cnn:
            pos = torch.arange(self.length - self.LB, self.length, device=self.x_ring.device)
            return self.x_ring[:, pos % self.x_ring.shape[1]]
        return self.xs[:, :self.LB]

    # the one launch of a position whose arguments change: q -> q_in, k / v -> the caches' new rows (a max_step_rows session:
    # the s rows of the step, into the view of q_in that an s-row step reads)
    def _stage(self, q, k, v):
        q_in = self.q_in if self.max_step_rows is None else self._rows_views(q.shape[2])[0]
        ops.decode_stage(q, k, v, q_in, self.kv_cache, self.ctr32[:, :2] if self.ragged else self.ctr32[:2],
                         block_table=self.block_table, capacity=self.capacity)

    # the (captured) launches of one position; everything position-dependent is read from device memory
    def _launch(self):
        at, H, D, T_M = self.attention, self.H, self.D, self.T_M
        paged = dict(block_table=self.block_table, capacity=self.capacity) if self.paged else {}
        # chunk-aligned step: the kernel walks the open Performer chunk again from the caches (which hold the new row already)
        performer_value, avg_rows, _ = ops.performer_step(
            self.q_in, self.k_cache, self.v_cache, at.v_eye_learned_causal[0, 0], at.performer.projection_matrix,
            state_in=self.image, t_base_dev=self.seen32, **paged)
        _x, _t, row_scale, avg_scale = ops.predictor_mlp(
            performer_value, at.attention_predictor_enc[0], at.attention_predictor_enc[1],
            at.attention_predictor_dec_row[0], at.attention_predictor_cnn[0].module,
            at.attention_predictor_dec_scaler[0], want_tpred=False,
            x_c8_out=self.x_new if self.fused_cnn else self.xs[:, -1:])       # the new row (fused CNN: its own buffer; else behind the window)
        keepres, ln2 = at.attention_predictor_cnn[1].module, at.attention_predictor_cnn[2].module
        body = list(keepres.net.children())
        conv4 = body[-1].module
        if self.fused_cnn:
            # conv1 + conv2 (one new row each) + tail + selection + the counters' advance: one launch
            # The attention launch expands the kept pixels itself (decode form of sea_sparse_attention: the emit phase / launch and the
            # crow -> col -> K / V chain leave the position's critical path); where that form does not exist the CSR row's
            # column ids come out of this launch (LDS allowing) or an emit launch behind it, as in the first round-5 version.
            fused_attn = self.fused_attention and ops.fused_interp_supported(self.q_in.dtype, D, T_M)
            emits = not fused_attn and ops.decode_cnn_emits(self.x_new.shape[-3] * 8)
            col = torch.empty((self.N, self.z_cap), dtype=torch.int32, device=self.q_in.device) if emits else None
            self.probs, sel = ops.decode_cnn_tail_select(
                self.x_new, self.x_ring, self.y1_ring, self.y2, body[0].module, body[2].module, conv4.weight[:, :, 0, 0], conv4.bias,
                ln2.weight, ln2.bias, T_M, self.keep_table, self.k, self.ctr32, self.ticket, self.crow, eps=ln2.eps,
                col_out=col, T_cap=self.capacity)
            if emits:
                csr = ops.FlatCSR(self.crow, col, sel[2], H, self.capacity, bits=sel[0], row_nnz=sel[1])
            else:
                csr = ops.csr_from_selection(*sel, H, T_M, self.capacity, self.k, True, self.z_cap, t_src_dev=self.tsrc_done32,
                                             crow=self.crow, defer_emit=fused_attn)
            ops.sparse_attention(self.q_in, self.k_cache, self.v_cache, csr,
                                 row_scale=row_scale if at.pconfig.partial_attention_scaler else None,
                                 avg=avg_rows, mix=avg_scale, out=self.ctx.view(self.N, 1, H, D).permute(0, 2, 1, 3),
                                 path="gather", keep_columns_pending=True, block_table=self.block_table,
                                 probs_out=self._probs_buf)
            self.csr = csr                                                    # (the step's selection: columns on first read of .col)
            self._col_emit = csr._pending                                     # (None: a launch of the step writes the columns)
            return
        y = self.xs                                                           # (N, LB + 1, C/8, W, 8)
        for i in range(0, len(body) - 2, 2):
            conv = body[i].module
            y = ops.causal_conv_c8(y, conv.weight, conv.bias, conv.kernel_size, conv.dilation, conv.padding[1], relu=True)
        y_new = y[:, -1:]                                                     # (the tail reads the row where it lies)
        self.probs, _, sel = ops.predictor_tail_select(
            y_new, conv4.weight[:, :, 0, 0], conv4.bias, ln2.weight, ln2.bias, up=4, T_m=T_M, keep=self.keep_table,
            k=self.k, T_src=0, is_causal=True, eps=ln2.eps, want_scores=False, t_src_dev=self.tsrc32, crow_out=self.crow)
        csr = ops.csr_from_selection(*sel, H, T_M, self.capacity, self.k, True, self.z_cap, t_src_dev=self.tsrc32, crow=self.crow)
        ops.sparse_attention(self.q_in, self.k_cache, self.v_cache, csr,
                             row_scale=row_scale if at.pconfig.partial_attention_scaler else None,
                             avg=avg_rows, mix=avg_scale, out=self.ctx.view(self.N, 1, H, D).permute(0, 2, 1, 3),
                             path="gather", probs_out=self._probs_buf)
        self.csr, self._col_emit = csr, None                                  # (the emit launch above wrote the columns)
        ops.c8_window_shift(self.xs, counters=self.ctr32[:2])                 # the window of the next position; counters += 1

    # a step of s rows (max_step_rows sessions): the same launches over s rows per sequence, on views of the S-row buffers
    def _rows_views(self, s):
        N, H, D, rs = self.N, self.H, self.D, tuple(self.x_new.shape[1:])
        return (self.q_in[:N * H * s * D].view(N, H, s, D), self.x_new[:N * s].view((N, s) + rs), self.y2[:N * s].view((N, s) + rs),
                self.y1_scratch[:N * s * 2].view((N, s, 2) + rs), self.ctx[:N * s * H * D].view(N, s, H * D))

    def _launch_rows(self, s):
        at, N, H, D, T_M = self.attention, self.N, self.H, self.D, self.T_M
        q_in, x_new, y2, y1_scratch, ctx = self._rows_views(s)
        performer_value, avg_rows, _ = ops.performer_step(
            q_in, self.k_cache, self.v_cache, at.v_eye_learned_causal[0, 0], at.performer.projection_matrix,
            state_in=self.image, t_base_dev=self.seen32)
        _x, _t, row_scale, avg_scale = ops.predictor_mlp(
            performer_value, at.attention_predictor_enc[0], at.attention_predictor_enc[1],
            at.attention_predictor_dec_row[0], at.attention_predictor_cnn[0].module,
            at.attention_predictor_dec_scaler[0], want_tpred=False, x_c8_out=x_new)
        keepres, ln2 = at.attention_predictor_cnn[1].module, at.attention_predictor_cnn[2].module
        body = list(keepres.net.children())
        conv4 = body[-1].module
        self.probs, sel = ops.decode_cnn_tail_select(
            x_new, self.x_ring, self.y1_ring, y2, body[0].module, body[2].module, conv4.weight[:, :, 0, 0], conv4.bias,
            ln2.weight, ln2.bias, T_M, self.keep_table, self.k, self.ctr32, self.ticket, eps=ln2.eps, y1_scratch=y1_scratch)
        fused_attn = ops.fused_interp_supported(self.dtype, D, T_M)
        csr = ops.csr_from_selection(*sel, H, T_M, self.capacity, self.k, True, s * self.z_cap, t_src_dev=self.tsrc_done32,
                                     defer_emit=fused_attn)
        ops.sparse_attention(q_in, self.k_cache, self.v_cache, csr,
                             row_scale=row_scale if at.pconfig.partial_attention_scaler else None,
                             avg=avg_rows, mix=avg_scale, out=ctx.view(N, s, H, D).permute(0, 2, 1, 3),
                             path="gather", keep_columns_pending=True,
                             probs_out=None if self._probs_buf is None else self._probs_buf[:, :s * self.z_cap])
        self.csr, self._col_emit = csr, csr._pending

    def _capture(self, s=None):
        """One eager step on a side stream would advance the state, so the capture runs against SAVED copies of the
        mutable buffers, restored afterwards (a capture records launches, it does not execute them).

        The captured launches hold RAW POINTERS to the re-laid-out predictor weights of `ops.predictor._prep_cache` (MLP,
        convolution, tail, LayerNorm and projection packs built lazily inside `_launch`).  The session pins the very
        tensors its launches took from the cache (`ops.pinned_prep`), so a cache eviction -- `clear_prep_cache()` from
        another layer's `.to()` / `load_state_dict`, or the cache's own size bound -- cannot free memory a replay still
        reads; and it remembers the cache generation: `step()` re-captures when that has moved, because a cleared cache
        means the weights may have been edited and the pinned packs may be stale.
        `s` (max_step_rows sessions): the graph of an s-row step, one per distinct s (kept in `_graphs`)."""
        mutable = [self.image, self.kv_cache, self.ctr32]
        mutable += [self.x_ring, self.y1_ring, self.ticket] if self.fused_cnn else [self.xs]
        saved = [t.clone() for t in mutable]
        with ops.pinned_prep() as pins:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side), torch.no_grad():                    # warm-up: lazy library work happens outside the capture
                zero = torch.zeros((self.N, self.H, s or 1, self.D), dtype=self.q_in.dtype, device=self.q_in.device)
                self._stage(zero, zero, zero)
                self._launch() if s is None else self._launch_rows(s)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g), torch.no_grad():
                self._launch() if s is None else self._launch_rows(s)
        for dst, src in zip(mutable, saved):
            dst.copy_(src)
        if s is None:
            self.graph = g
            self._pinned = pins
        else:
            self._graphs[s] = (g, self.csr, self._col_emit, self.probs, pins)
        self.captures = getattr(self, "captures", 0) + 1
        self._prep_generation = ops.prep_generation()

    def export_state(self, slot: Optional[int] = None) -> PerlinAttentionState:
        """The session's state as the `PerlinAttentionState` a cached forward continues from (copies: the session keeps
        running on its own buffers).  `slot`: that sequence alone, as an N = 1 state (a ragged session exports one
        sequence at a time)."""
        if slot is None and self.ragged and self.N > 1:
            raise ValueError("a ragged session exports one sequence at a time: export_state(slot)")
        if slot is not None:
            self._check_slot(slot)
        if self.ragged and self._empty[slot or 0]:
            raise ValueError(f"export_state: slot {slot or 0} is empty (released, or never admitted)")
        length = self.lengths[slot or 0] if self.ragged else self.length
        image, win = self.image, self.win
        if slot is not None:
            image, win = image.view(self.N, -1)[slot], win[slot:slot + 1]
        return self._state(image.clone(), win.clone(), length)

    @torch.no_grad()
    def step(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> torch.Tensor:
        """The new rows of every slot, (N, H, 1, D) each -> the context rows (N, 1, H*D), a static buffer.  A session built
        with `max_step_rows` S takes (N, H, s, D) with 1 <= s <= S and returns (N, s, H*D); `rewind` may then undo it.
        Slots that sit out (`paused`, `empty`): their input rows are ignored (anything, NaN included), their context rows are
        zeros and their CSR rows empty; capacity and the page pool are checked for the slots that take part only."""
        if self.max_step_rows is not None:
            return self._step_rows(q, k, v)
        if self.ragged and q.dim() == 4 and q.shape[2] != 1:
            raise ValueError(f"a step of {q.shape[2]} rows: this session takes one row per step "
                             "(DecodeSession.from_sequences(..., max_step_rows=...) takes several)")
        if self.ragged:
            full = [n for n, L in enumerate(self.lengths) if L >= self.capacity and not self._paused[n]]
            if full:
                raise RuntimeError(f"cache capacity {self.capacity} reached by slot(s) {full}")
            if self.paged:                             # new pages (or RuntimeError, nothing changed): their table entries are
                for n, i, pg in self.slot_pages.grow(self.lengths, self._paused):    # small fills in stream order, no synchronise
                    self.block_table[n, i].fill_(pg)
        else:
            assert self.length < self.capacity, "cache capacity reached"
        if self.graph is not None and ops.prep_generation() != self._prep_generation:
            self.graph = None                                      # (re-captured below, BEFORE this step's stage launch: the capture
            self._capture()                                        #  runs a warm-up step on saved copies of the state)
        self._stage(q, k, v)
        if self.graph is not None:
            self.graph.replay()
            self._rearm(self.csr, self._col_emit)
        else:
            self._launch()
        self._publish_attention_probs()
        if self.ragged:
            self._zero_sitting_rows(self.ctx)
            self.lengths = [L if out else L + 1 for L, out in zip(self.lengths, self._paused)]
        else:
            self.length += 1
        return self.ctx

    def _step_rows(self, q, k, v):
        N, H, D = self.N, self.H, self.D
        if not all(torch.is_tensor(t) and t.dim() == 4 for t in (q, k, v)) or k.shape != q.shape or v.shape != q.shape \
                or (q.shape[0], q.shape[1], q.shape[3]) != (N, H, D):
            raise ValueError(f"step: q, k, v are (N, H, s, D) = ({N}, {H}, s, {D}) each (got {[tuple(t.shape) for t in (q, k, v)]})")
        if not all(t.dtype == self.dtype and t.is_cuda for t in (q, k, v)):
            raise ValueError(f"step: {self.dtype} rows on the GPU")
        s = int(q.shape[2])
        if not 1 <= s <= self.max_step_rows:
            raise ValueError(f"a step of {s} rows: this session takes 1 .. {self.max_step_rows}")
        full = [n for n, L in enumerate(self.lengths) if L + s > self.capacity and not self._paused[n]]
        if full:
            raise RuntimeError(f"cache capacity {self.capacity} reached by slot(s) {full} (a step of {s} rows)")
        if self._graphs and ops.prep_generation() != self._prep_generation:
            self._graphs = {}                                      # (re-captured lazily, before this step's stage launch)
        if self.use_graph and s not in self._graphs:
            self._capture(s)
        # the Performer image changes only when a chunk completes (at most once: s <= 8 <= chunk): a copy of the slices that
        # this step moves to the next boundary, for `rewind`
        C = self.chunk
        crossed = [n for n, L in enumerate(self.lengths) if (L + s) // C > L // C and not self._paused[n]]
        img = self.image.view(N, -1)
        for n in crossed:
            self.image_backup[n].copy_(img[n])
        self._stage(q, k, v)
        if self.use_graph:
            g, self.csr, self._col_emit, self.probs, _pins = self._graphs[s]
            g.replay()
            self._rearm(self.csr, self._col_emit)                  # (as in `step`: the handle is every replay's)
        else:
            self._launch_rows(s)
        self._publish_attention_probs(s)
        self._last_step = (s, list(self.lengths), crossed)
        self.lengths = [L if out else L + s for L, out in zip(self.lengths, self._paused)]
        ctx = self._rows_views(s)[4]
        self._zero_sitting_rows(ctx)
        return ctx

    @torch.no_grad()
    def rewind(self, drop) -> None:
        """Undo the last drop[n] rows of the last step in slot n (0 <= drop[n] <= s of that step; speculative decoding drops
        the rejected draft tokens).  Slot n is then bitwise what a plain session is after stepping only the kept rows: its
        Performer image, CNN rings, K / V rows below its length and every later step.  Only the last step, once, and only
        while nothing else has changed the session (another `step`, an `admit`, `pause`, `resume` or `release` ends the
        chance).  A slot that sat out the step has nothing to drop (drop[n] = 0, else ValueError).  Sessions built with
        `max_step_rows`; ValueError otherwise, and for a rewind without a step to undo or a bad `drop`, with nothing changed."""
        if self.max_step_rows is None:
            raise ValueError("rewind: a session built with DecodeSession.from_sequences(..., max_step_rows=...)")
        if self._last_step is None:
            raise ValueError("rewind: no step to undo (only the last step, once, and not after an admit)")
        s, before, crossed = self._last_step
        drop = [int(d) for d in drop]
        if len(drop) != self.N:
            raise ValueError(f"rewind: {len(drop)} counts for {self.N} slots")
        if not all(0 <= d <= s for d in drop):
            raise ValueError(f"rewind: counts {drop} outside 0 .. {s} (the rows of the last step)")
        sat_out = [n for n, d in enumerate(drop) if d and self._paused[n]]
        if sat_out:
            raise ValueError(f"rewind: slot(s) {sat_out} sat out the last step (paused or empty): nothing of it to drop")
        self._flush_columns()
        kept = [L if out else L + s - d for L, d, out in zip(before, drop, self._paused)]
        img, C = self.image.view(self.N, -1), self.chunk
        for n in crossed:
            if kept[n] // C == before[n] // C:        # back below the boundary the step completed: the image from before it
                img[n].copy_(self.image_backup[n])
        self.lengths = kept
        self._write_counters()
        self._last_step = None


class SessionState:
    """What a graph-replayed step hands back in the place of a `PerlinAttentionState` (e.g. as the third element of the
    OPT block's cache tuple): a ticket for the NEXT step of the same session.  It is valid while the session has not moved
    on; `materialize()` turns it into a real state for a call the session cannot serve (several tokens at once: the OPT
    block's uniform session takes one; a ragged session built with `max_step_rows` takes several itself)."""

    def __init__(self, session: DecodeSession):
        self.session = session
        self.seq_len = session.length

    @property
    def current(self) -> bool:
        return self.session.length == self.seq_len

    def materialize(self) -> PerlinAttentionState:
        assert self.current, "this decode state is stale: its session has produced later positions (sessions cannot branch)"
        return self.session.export_state()
