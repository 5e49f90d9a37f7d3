"""The host-side page allocator of a paged decode session (`perlin_attention.decode.PageAllocator`): hand-out order,
exhaustion, double frees and the give-back-then-take of `admit`.  No GPU."""
import pytest

from sea_attention_amd.perlin_attention.decode import PageAllocator


def test_pages_go_out_in_order():
    a = PageAllocator(6)
    assert a.free_pages == 6
    assert a.take(2) == [0, 1]
    assert a.take(3) == [2, 3, 4]
    assert a.free_pages == 1
    assert a.take(0) == []


def test_exhaustion_takes_nothing():
    a = PageAllocator(4)
    a.take(3)
    with pytest.raises(RuntimeError, match="page pool exhausted"):
        a.take(2)
    assert a.free_pages == 1                      # the refused request took nothing
    assert a.take(1) == [3]
    with pytest.raises(RuntimeError, match="exhausted"):
        a.take(1)


def test_double_free_and_foreign_pages_are_refused():
    a = PageAllocator(4)
    pages = a.take(2)
    a.give_back(pages)
    with pytest.raises(ValueError, match="double free"):
        a.give_back(pages)
    with pytest.raises(ValueError):
        a.give_back([7])                          # never out of this pool
    got = a.take(1)
    with pytest.raises(ValueError):
        a.give_back(got + got)                    # the same page twice in one call
    assert a.free_pages == 3                      # nothing of the refused calls went back


def test_given_back_pages_are_reused_first_in_their_order():
    """admit: the slot's pages go back first, then its new prefix takes pages -- the same ones, in the same order."""
    a = PageAllocator(10)
    slot0, slot1 = a.take(3), a.take(4)
    assert slot1 == [3, 4, 5, 6]
    a.give_back(slot1)
    assert a.free_pages == 7
    assert a.take(2) == [3, 4]                    # the returned pages before never-used 7, 8, 9
    assert a.take(3) == [5, 6, 7]
    a.give_back(slot0)
    assert a.take(4) == [0, 1, 2, 8]


def test_an_empty_pool_is_refused():
    with pytest.raises(ValueError):
        PageAllocator(0)
