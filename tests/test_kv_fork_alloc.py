"""The reference-counted page bookkeeping behind HipModel.reserve / release / fork_row (specdec_hip.pages.PagePool), driven
without a device: what a fork shares against what it copies, the accounting after it, and that a fork-free sequence hands out the
pages the plain free stack handed out before pages could have two owners."""

import pytest

from specdec_hip.pages import PagePool, shared_pages

P = 32
# length -> (pages shared, [positions copied per fresh page]): pages wholly below position length - 2 are shared
EXPECT = {
    1: (0, [1]), 2: (0, [2]), 31: (0, [31]), 32: (0, [32]), 33: (0, [32, 1]), 34: (1, [2]),
    64: (1, [32]), 65: (1, [32, 1]), 66: (2, [2]),
}


def _pool(n_pages=16, rows=4):
    return PagePool(n_pages, rows, P)


@pytest.mark.parametrize("length", sorted(EXPECT))
def test_what_is_shared_and_what_is_copied(length):
    n_share, copied = EXPECT[length]
    assert shared_pages(length, P) == n_share
    pool = _pool()
    pool.reserve(2, 1)                                  # so that the source's pages are not 0, 1, 2
    pool.reserve(1, pool.pages_for(length + 20))        # the source owns more than `length` needs
    src = list(pool.owned[1])
    n_src = pool.pages_for(length)
    before = pool.pages_in_use()
    plan = pool.fork(1, [0, 3], length)
    assert plan.shared == src[:n_share]
    assert len(plan.tables) == 2 and len(plan.copies) == 2 * len(copied)
    fresh = set()
    for t, d in enumerate((0, 3)):
        own = pool.owned[d]
        assert own == plan.tables[t] and len(own) == n_src
        assert own[:n_share] == src[:n_share]                       # shared: the very pages of the source
        mine = plan.copies[t * len(copied):(t + 1) * len(copied)]
        assert [c[0] for c in mine] == src[n_share:n_src]           # copied from the source's pages, in position order
        assert [c[1] for c in mine] == own[n_share:]                # ... into the row's fresh pages
        assert [c[2] for c in mine] == copied
        fresh |= set(own[n_share:])
    assert not fresh & set(src) and len(fresh) == 2 * len(copied)   # fresh pages are nobody else's
    assert pool.owned[1] == src                                     # the source keeps what it had
    assert pool.pages_in_use() == before + 2 * len(copied)          # a shared page counts once
    assert all(pool.refs[p] == 3 for p in src[:n_share]) and all(pool.refs[p] == 1 for p in fresh)


def test_releasing_the_source_first_keeps_shared_pages_alive():
    pool = _pool()
    pool.reserve(0, 3)                                  # 96 positions
    src = list(pool.owned[0])
    pool.fork(0, [1, 2], 90)                            # 88 // 32 = 2 pages shared, the third copied (26 positions)
    assert pool.pages_in_use() == 3 + 2 and pool.shares(0) and pool.shares(1)
    pool.release(0)
    assert pool.pages_in_use() == 4                     # only the source's own third page went back
    assert src[2] in pool.free and src[0] not in pool.free and src[1] not in pool.free
    assert pool.owned[1][:2] == src[:2] and pool.owned[2][:2] == src[:2]
    pool.release(1)
    assert pool.pages_in_use() == 3 and not pool.shares(2)
    pool.release(2)
    assert pool.pages_in_use() == 0 and sorted(pool.free) == list(range(16)) and pool.refs == [0] * 16


def test_destination_releases_what_it_owned_and_can_be_forked_again():
    pool = _pool(n_pages=6, rows=3)
    pool.reserve(0, 2)
    pool.reserve(1, 3)                                  # the destination holds an older sequence
    pool.fork(0, [1], 64)                               # 1 shared + 1 fresh; row 1's three pages went back first
    assert pool.pages_in_use() == 3 and len(pool.owned[1]) == 2
    pool.fork(0, [1], 64)                               # again: nothing leaks
    assert pool.pages_in_use() == 3
    pool.reserve(1, 4)                                  # a forked row grows like any other
    assert pool.pages_in_use() == 5 and len(pool.owned[1]) == 4
    for r in range(3):
        pool.release(r)
    assert pool.pages_in_use() == 0


def test_pool_exhaustion_leaves_the_state_unchanged():
    pool = _pool(n_pages=5, rows=3)
    pool.reserve(0, 3)
    pool.reserve(1, 2)                                  # 5 of 5 pages
    snap = (list(pool.free), [list(o) for o in pool.owned], list(pool.refs))
    with pytest.raises(RuntimeError, match="pool exhausted"):
        pool.fork(0, [2], 70)                           # 2 shared, but the third page needs a fresh one and row 2 gives nothing up
    assert (pool.free, pool.owned, pool.refs) == (snap[0], snap[1], snap[2])
    pool.release(1)
    pool.reserve(1, 1)                                  # 1 page free now
    snap = (list(pool.free), [list(o) for o in pool.owned], list(pool.refs))
    with pytest.raises(RuntimeError, match="pool exhausted"):
        pool.fork(0, [2], 33)                           # nothing shared below 31: two fresh pages
    assert (pool.free, pool.owned, pool.refs) == (snap[0], snap[1], snap[2])


def test_pages_a_destination_gives_up_count_as_free():
    pool = _pool(n_pages=5, rows=3)
    pool.reserve(0, 3)
    pool.reserve(1, 2)                                  # pool full
    pool.fork(0, [1], 96)                               # 2 shared + 1 fresh: served by the pages row 1 releases
    assert pool.pages_in_use() == 4 and len(pool.owned[1]) == 3


def test_bad_rows_are_refused_before_any_change():
    pool = _pool()
    pool.reserve(0, 2)
    snap = (list(pool.free), [list(o) for o in pool.owned])
    for dsts in ([0], [1, 1], [4], [-1]):
        with pytest.raises(ValueError):
            pool.fork(0, dsts, 40)
    with pytest.raises(ValueError):
        pool.fork(0, [1], 65)                           # the source does not hold that many positions
    assert (pool.free, pool.owned) == (snap[0], snap[1])


def test_fork_free_sequences_hand_out_the_same_pages_as_the_plain_free_stack():
    """The literal lists are what HipModel.reserve handed out for this sequence when _free / _owned were a plain stack and plain
    lists (pop() from the end; release: _free.extend(reversed(owned)))."""
    pool = PagePool(8, 3, P)
    got = []
    need = lambda n: pool.pages_for(n)
    got.append(pool.reserve(0, need(65)))
    got.append(pool.reserve(1, need(40)))
    got.append(pool.reserve(0, need(100)))
    got.append(pool.reserve(0, need(100)))             # already there: nothing new
    pool.release(0)
    assert pool.free == [7, 6, 5, 2, 1, 0]
    got.append(pool.reserve(2, need(70)))
    pool.release(1)
    assert pool.free == [7, 6, 5, 4, 3]
    got.append(pool.reserve(0, need(33)))
    got.append(pool.reserve(1, need(96)))
    assert got == [(0, [0, 1, 2]), (0, [3, 4]), (3, [5]), (4, []), (0, [0, 1, 2]), (0, [3, 4]), (0, [5, 6, 7])]
    assert pool.pages_in_use() == 8 and max(pool.refs) == 1
    with pytest.raises(RuntimeError, match="pool exhausted: row 2 needs 1 more pages, 0 free of 8"):
        pool.reserve(2, 4)
    assert pool.owned == [[3, 4], [5, 6, 7], [0, 1, 2]]
