"""`perlin_attention.decode.SlotPages`: the host-side owner of a paged decode session's pages -- which pages a slot takes when
it is seeded, grows or is extended, which a fork shares and which it copies, what a refusal leaves behind, and
free + distinct held = pool.  Plain lists, no GPU: `DecodeSession` applies these decisions to the device.

The expected page numbers of the worked scenario are derived by hand from the allocator's rule (lowest index first; pages
given back go out again before any never-used one, most recently returned first), not read off the code under test."""
import random

import pytest

from sea_attention_amd.perlin_attention.decode import SlotPages


def _holders(sp, pool):
    return [sp.allocator.holders(pg) for pg in range(pool)]


def _free_list(sp):
    return list(sp.allocator._free)


def _move(sp, parents, lengths, paused, empty):
    """fork / reorder as `DecodeSession._move` drives them: plan (refusal or fresh pages), the launch, commit, host mirrors."""
    moves = [(p, i) for i, p in enumerate(parents) if p != i]
    new_open = sp.move_plan(moves, lengths)
    sp.move_commit(moves, lengths, new_open)
    old_lengths, old_paused = list(lengths), list(paused)
    for src, dst in moves:
        lengths[dst], paused[dst], empty[dst] = old_lengths[src], old_paused[src], False
    return new_open


def test_worked_scenario():
    sp = SlotPages(3, 64, 16, 8)
    assert (sp.n_tab, sp.page_rows, sp.capacity, sp.free_pages) == (4, 16, 64, 8)
    assert [sp.count(r) for r in (0, 1, 16, 17, 64)] == [0, 1, 1, 2, 4]
    assert sp.reseat(0, 20) == [0, 1]                            # 21 rows: two pages
    assert sp.reseat(1, 40) == [2, 3, 4]
    lengths, paused, empty = [20, 40, 0], [False, False, True], [False, False, True]
    assert 20 // sp.page_rows == 1 and sp.open_page(0, 20) == 1  # slot 0's next row lies at table index 1: page 1
    assert _move(sp, [0, 1, 0], lengths, paused, empty) == {2: (1, 5)}       # fork 0 -> 2: page 1 is copied to the next unused page
    assert sp.pages == [[0, 1], [2, 3, 4], [0, 5]] and sp.allocator.holders(0) == 2 and sp.free_pages == 2
    assert sp.shared() == [0] and [sp.reclaimable(n) for n in range(3)] == [1, 3, 1]
    assert lengths == [20, 40, 20] and empty == [False] * 3
    fresh = sp.extend_take(2, 20, 30)                            # rows 20 .. 49 and the next step's: ceil(51 / 16) = 4 pages, it has 2
    assert fresh == [6, 7] and sp.pages[2] == [0, 5]             # (taken, not yet the slot's)
    sp.pages[2].extend(fresh)                                    # (the session files them once the rows are written)
    assert sp.pages[2] == [0, 5, 6, 7] and sp.free_pages == 0
    assert sp.grow([20, 40, 50], [False] * 3) == []              # nobody's next row starts a page
    before = ([list(p) for p in sp.pages], _holders(sp, 8), _free_list(sp))
    with pytest.raises(RuntimeError, match=r"page pool exhausted: slot\(s\) \[0\]"):
        sp.grow([32, 40, 50], [False] * 3)                       # slot 0 stands at the end of its second page, nothing is free
    assert ([list(p) for p in sp.pages], _holders(sp, 8), _free_list(sp)) == before
    assert sp.grow([32, 40, 50], [True, False, False]) == []     # it sits out: no page wanted
    sp.release(1)
    assert _free_list(sp) == [2, 3, 4] and sp.pages[1] == []
    assert sp.grow([32, 0, 50], [False, True, False]) == [(0, 2, 2)] and sp.pages[0] == [0, 1, 2]
    sp.release(0)                                                # page 0 stays out: slot 2 still names it
    assert _free_list(sp) == [1, 2, 3, 4] and sp.allocator.holders(0) == 1 and sp.shared() == []
    assert sp.extend_take(2, 50, 1) == []                        # open page 7 is private; row 51 and the next lie in it
    sp.allocator.share(sp.pages[2])                              # slot 1 names slot 2's whole row, the open page included
    sp.pages[1] = list(sp.pages[2])
    before = ([list(p) for p in sp.pages], _holders(sp, 8), _free_list(sp))
    with pytest.raises(RuntimeError, match="open page 7 has other holders"):
        sp.extend_take(1, 50, 1)
    assert ([list(p) for p in sp.pages], _holders(sp, 8), _free_list(sp)) == before


def test_reseat_refuses_before_anything_changes():
    sp = SlotPages(2, 64, 16, 4)
    assert sp.reseat(0, 20) == [0, 1] and sp.reseat(1, 10) == [2]
    before = ([list(p) for p in sp.pages], _holders(sp, 4), _free_list(sp))
    with pytest.raises(RuntimeError, match="page pool exhausted: slot 1 needs 3 pages for a prefix of 40 rows, 1 free "):
        sp.reseat(1, 40)                                         # 1 free + 1 of its own < 3
    assert ([list(p) for p in sp.pages], _holders(sp, 4), _free_list(sp)) == before
    assert sp.reseat(1, 20) == [2, 3]                            # its own page comes back first and goes out first


# (a pool of 20 pages left four of the twenty seeds with fewer than five refusals; 16 gives 243 - 290 completed operations
#  and 9 - 59 refusals per seed)
SLOTS, CAPACITY, PAGE_ROWS, POOL, OPS = 6, 96, 16, 16, 400
KINDS = ["admit", "step", "step", "step", "extend", "fork", "reorder", "release", "pause", "resume"]


def _check(sp, lengths, empty):
    rows = sp.pages
    for pg in range(POOL):
        assert sp.allocator.holders(pg) == sum(row.count(pg) for row in rows), pg
    assert sp.free_pages + len({pg for row in rows for pg in row}) == POOL
    for n, row in enumerate(rows):
        assert len(set(row)) == len(row), (n, row)
        if empty[n]:
            assert row == []
        else:
            assert sp.count(lengths[n]) <= len(row) <= sp.n_tab, (n, lengths[n], row)


def _apply(sp, rng, kind, lengths, paused, empty):
    """One operation, driven the way the session drives it.  Returns False when the session would refuse it by argument
    (nothing is called then); RuntimeError is a refusal by `SlotPages`."""
    n = rng.randrange(SLOTS)
    if kind == "admit":
        L = rng.randrange(1, CAPACITY)
        sp.reseat(n, L)
        lengths[n], paused[n], empty[n] = L, False, False
    elif kind == "step":
        if any(L >= CAPACITY and not out for L, out in zip(lengths, paused)):       # (the session's own capacity refusal)
            return False
        sp.grow(lengths, paused)
        lengths[:] = [L if out else L + 1 for L, out in zip(lengths, paused)]
    elif kind == "extend":
        s = rng.randrange(1, 40)
        if empty[n] or lengths[n] + s > CAPACITY:
            return False
        sp.pages[n].extend(sp.extend_take(n, lengths[n], s))
        lengths[n] += s
    elif kind == "fork":
        dsts = rng.sample([d for d in range(SLOTS) if d != n], rng.randrange(1, 3))
        if empty[n]:
            return False
        parents = list(range(SLOTS))
        for d in dsts:
            parents[d] = n
        _move(sp, parents, lengths, paused, empty)
    elif kind == "reorder":
        parents = [rng.randrange(SLOTS) for _ in range(SLOTS)]
        if any(p != i and empty[p] for i, p in enumerate(parents)):
            return False
        _move(sp, parents, lengths, paused, empty)
    elif kind == "release":
        sp.release(n)
        lengths[n], paused[n], empty[n] = 0, True, True
    elif kind == "pause":
        paused[n] = True
    elif kind == "resume":
        if empty[n]:
            return False
        paused[n] = False
    return True


@pytest.mark.parametrize("seed", range(20))
def test_random_walk_keeps_the_books(seed):
    rng = random.Random(seed)
    sp = SlotPages(SLOTS, CAPACITY, PAGE_ROWS, POOL)
    lengths, paused, empty = [0] * SLOTS, [True] * SLOTS, [True] * SLOTS
    done = refused = 0
    for _ in range(OPS):
        kind = rng.choice(KINDS)
        snap = ([list(p) for p in sp.pages], _holders(sp, POOL), _free_list(sp), list(lengths))
        try:
            done += _apply(sp, rng, kind, lengths, paused, empty)
        except RuntimeError:
            refused += 1
            assert ([list(p) for p in sp.pages], _holders(sp, POOL), _free_list(sp), list(lengths)) == snap, kind
        _check(sp, lengths, empty)
    print(f"seed {seed}: {done} completed, {refused} refused")
    assert done >= 200 and refused >= 5, (done, refused)
