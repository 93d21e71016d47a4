"""Host-side bookkeeping of a paged KV pool: which pages are free, which pages each row owns (in position order), and
how many rows own each page.

No device and no torch in here: HipModel turns what these methods return into block-table writes and page copies. A page
has more than one owner only after `fork` (rows that hold the same prompt prefix share its pages); until then every
count is 0 or 1 and `reserve` / `release` hand pages out and take them back exactly as a plain free stack does.
"""

from __future__ import annotations

from typing import List, NamedTuple, Sequence, Tuple


class ForkPlan(NamedTuple):
    """What `PagePool.fork` did, for the caller to carry out on the device."""

    shared: List[int]                    # the source's pages every destination now also owns (table entries 0 .. len - 1)
    copies: List[Tuple[int, int, int]]   # (source page, destination page, positions to copy), over all destinations
    tables: List[List[int]]              # per destination: its pages in position order (shared ones first)


def shared_pages(length: int, page_len: int) -> int:
    """How many leading pages of a row with `length` cached positions a fork may share instead of copying.

    A shared page must never be written again by any of its owners. A row that holds `length` cached positions is
    handed to the step loop with seq_len = length + 1 (sd_specdec_set_row: the caches hold [0, seq_len - 1) of the
    target and at least [0, seq_len - 2) of the draft). The lowest position a step then writes is seq_len - 2 =
    length - 1: draft forward 0 runs over (prev, last) at positions seq_len - 2 and seq_len - 1, the verify forward of
    the target starts at seq_len - 1, and rows only append from there or roll back to >= their accepted length. This
    function keeps one more position of margin, as the rule is stated for callers: only pages that lie wholly below
    position length - 2 are shared, i.e. page i with (i + 1) * page_len <= length - 2; everything from there on is
    copied. (A row whose cache is rebuilt from position 0 — a resync — gives its shared pages up first:
    HipModel.unshare.)"""
    return max(int(length) - 2, 0) // int(page_len)


class PagePool:
    def __init__(self, n_pages: int, n_rows: int, page_len: int):
        self.n_pages, self.page_len = int(n_pages), int(page_len)
        self.free: List[int] = list(range(self.n_pages - 1, -1, -1))      # stack of free page indices
        self.owned: List[List[int]] = [[] for _ in range(int(n_rows))]     # per row, in position order
        self.refs: List[int] = [0] * self.n_pages                          # owners per page

    def pages_for(self, length: int) -> int:
        return (int(length) + self.page_len - 1) // self.page_len

    def reserve(self, row: int, need: int) -> Tuple[int, List[int]]:
        """Grow `row` to `need` pages. -> (index of the first new table entry, the new pages); raises when the pool cannot
        serve it, with nothing changed."""
        own = self.owned[row]
        first = len(own)
        if need <= first:
            return first, []
        if need - first > len(self.free):
            raise RuntimeError(f"KV page pool exhausted: row {row} needs {need - first} more pages, {len(self.free)} free of {self.n_pages}")
        while len(own) < need:
            p = self.free.pop()
            self.refs[p] = 1
            own.append(p)
        return first, own[first:]

    def release(self, row: int) -> None:
        """Give up the row's pages; a page goes back to the free stack when its last owner has released it."""
        for p in reversed(self.owned[row]):
            self.refs[p] -= 1
            if self.refs[p] <= 0:
                self.refs[p] = 0
                self.free.append(p)
        self.owned[row] = []

    def pages_in_use(self) -> int:
        """Physical pages with at least one owner (a shared page counts once)."""
        return self.n_pages - len(self.free)

    def shares(self, row: int) -> bool:
        """Does the row own a page that another row owns too?"""
        return any(self.refs[p] > 1 for p in self.owned[row])

    def fork(self, src: int, dsts: Sequence[int], length: int) -> ForkPlan:
        """Give every row of `dsts` the first `length` positions of row `src`: each destination releases what it owns,
        then owns the source's leading pages that no later write can touch (shared_pages) and one fresh page for each of
        the source's remaining pages up to `length`. Raises (pool exhausted, bad rows) before anything has changed."""
        length, P = int(length), self.page_len
        dsts = [int(d) for d in dsts]
        n_rows = len(self.owned)
        if not 0 <= src < n_rows or any(not 0 <= d < n_rows for d in dsts):
            raise ValueError(f"fork: rows {src} -> {dsts} outside the batch of {n_rows}")
        if src in dsts or len(set(dsts)) != len(dsts):
            raise ValueError(f"fork: destinations {dsts} must be distinct and differ from the source row {src}")
        n_src = self.pages_for(length)
        if length < 0 or n_src > len(self.owned[src]):
            raise ValueError(f"fork: row {src} owns {len(self.owned[src])} pages, {length} positions need {n_src}")
        n_share = shared_pages(length, P)
        n_copy = n_src - n_share
        # pages the destinations' releases would free: those whose every owner is a destination
        giving = {}
        for d in dsts:
            for p in self.owned[d]:
                giving[p] = giving.get(p, 0) + 1
        freed = sum(1 for p, n in giving.items() if self.refs[p] - n <= 0)
        if n_copy * len(dsts) > len(self.free) + freed:
            raise RuntimeError(f"KV page pool exhausted: forking {length} positions of row {src} into {len(dsts)} rows needs "
                               f"{n_copy * len(dsts)} pages, {len(self.free) + freed} free of {self.n_pages}")
        for d in dsts:
            self.release(d)
        src_pages = self.owned[src][:n_src]
        shared = src_pages[:n_share]
        copies: List[Tuple[int, int, int]] = []
        tables: List[List[int]] = []
        for d in dsts:
            own = list(shared)
            for p in shared:
                self.refs[p] += 1
            for i in range(n_share, n_src):
                p = self.free.pop()
                self.refs[p] = 1
                own.append(p)
                copies.append((src_pages[i], p, min(P, length - i * P)))
            self.owned[d] = own
            tables.append(list(own))
        return ForkPlan(shared, copies, tables)
