"""Shared pages in the page allocator of a paged decode session (`perlin_attention.decode.PageAllocator.share / holders /
give_back`): what `DecodeSession.fork` / `reorder` lean on.  A page stays out until its last holder gives it back, the free
count is exact, and refused calls change nothing.  No GPU."""
import pytest

from sea_attention_amd.perlin_attention.decode import PageAllocator


def test_a_shared_page_stays_out_until_its_last_holder_gives_it_back():
    a = PageAllocator(6)
    pages = a.take(3)
    assert [a.holders(pg) for pg in pages] == [1, 1, 1] and a.holders(5) == 0
    a.share(pages[:2])                            # a fork: a second slot names the two closed pages
    a.share(pages[:1])                            # and a third the first one
    assert [a.holders(pg) for pg in pages] == [3, 2, 1]
    assert a.free_pages == 3
    a.give_back(pages)                            # the first slot lets go: only page 2 comes free
    assert a.free_pages == 4 and [a.holders(pg) for pg in pages] == [2, 1, 0]
    a.give_back(pages[:2])
    assert a.free_pages == 5 and a.holders(0) == 1 and a.holders(1) == 0
    a.give_back(pages[:1])
    assert a.free_pages == 6 and a.holders(0) == 0


def test_pages_come_free_in_give_back_order_only_when_released():
    a = PageAllocator(8)
    slot0 = a.take(3)                             # 0, 1, 2
    a.share(slot0[:2])
    slot1 = slot0[:2] + a.take(1)                 # 0, 1 shared, 3 private
    a.give_back(slot0)                            # 2 comes free (0, 1 still held by slot 1)
    assert a.take(1) == [2]
    a.give_back(slot1)                            # 0, 1, 3 come free, reused in the order given back
    assert a.take(4) == [0, 1, 3, 4]


def test_free_pages_is_exact_with_sharing():
    a = PageAllocator(10)
    rows = [a.take(4)]
    for _ in range(3):                            # three forks of one slot: 3 closed pages shared, an open page each
        a.share(rows[0][:3])
        rows.append(rows[0][:3] + a.take(1))
    distinct = {pg for r in rows for pg in r}
    assert len(distinct) == 7 and a.free_pages + len(distinct) == 10
    assert [a.holders(pg) for pg in rows[0]] == [4, 4, 4, 1]


def test_sharing_a_page_that_is_not_out_is_refused_and_changes_nothing():
    a = PageAllocator(4)
    pages = a.take(2)
    with pytest.raises(ValueError, match="not out"):
        a.share([pages[0], 3])                    # 3 was never taken: page 0 gains no holder either
    assert a.holders(pages[0]) == 1 and a.holders(3) == 0 and a.free_pages == 2
    a.give_back(pages[1:])
    with pytest.raises(ValueError, match="not out"):
        a.share(pages[1:])                        # given back: free, not shareable
    with pytest.raises(ValueError):
        a.share([9])                              # foreign
    assert a.free_pages == 3


def test_double_frees_are_refused_and_change_nothing():
    a = PageAllocator(4)
    pages = a.take(2)
    a.share(pages[:1])                            # page 0: two holders, page 1: one
    with pytest.raises(ValueError, match="double free"):
        a.give_back([pages[1], pages[1]])         # more give-backs than holders in one call
    with pytest.raises(ValueError, match="double free"):
        a.give_back(pages + [3])                  # 3 is not out: nothing of the call goes back
    assert a.holders(pages[0]) == 2 and a.holders(pages[1]) == 1 and a.free_pages == 2
    a.give_back([pages[0], pages[0]])             # as many as it has holders: fine
    assert a.holders(pages[0]) == 0 and a.free_pages == 3
    with pytest.raises(ValueError, match="double free"):
        a.give_back(pages[:1])
    assert a.free_pages == 3


def test_one_holder_per_page_behaves_as_before():
    """Without share(), take / give_back hand pages out and back exactly as the unshared allocator did."""
    a = PageAllocator(10)
    slot0, slot1 = a.take(3), a.take(4)
    a.give_back(slot1)
    assert a.take(2) == [3, 4] and a.take(3) == [5, 6, 7]
    a.give_back(slot0)
    assert a.take(4) == [0, 1, 2, 8]
    assert all(a.holders(pg) == 1 for pg in range(9)) and a.holders(9) == 0
