"""Cascade attention's groups (csrc/attention_cascade.hip): which cache rows share a prefix with which, as the table of
HipModel.set_shared_prefix wants it. Pure bookkeeping, no device work: a session calls fork() where it forks a row's KV from
another's and rewrite() before it rewrites a slot, then sends flush() to the engine.

The table: leader[b] and shared_len[b] per row. Keys [0, shared_len[b]) of row b are bit-identical to row leader[b]'s. A group is
one level deep: its root names itself with the longest length of its members, every member names the root. A row in no group is
(b, 0). Lengths are multiples of 32 (the kernel's key block); a row that would share fewer than min_shared positions stays out."""

from __future__ import annotations

from typing import List, Tuple


# Shared lengths below this stay out of the table unless the config key cascade_min_shared says otherwise. From
# profiles/cascade_attention.md: the verify pass does not stop losing anywhere up to 32768 shared positions (the longest measured),
# so the default lies at that edge and a run that asks for the mode without lowering the key forms no group below it.
MIN_SHARED_DEFAULT = 32768


def asked(pipe, cascade_attention) -> bool:
    """the call's argument over the config key"""
    return bool(pipe.config.get("cascade_attention", False) if cascade_attention is None else cascade_attention)


def refuse_single(pipe, kwargs) -> None:
    if asked(pipe, kwargs.pop("cascade_attention", None)):
        raise NotImplementedError("cascade_attention belongs to generate_batch and generate_many: generate() decodes one row")


def check_session(pipe, share_prefix: bool, self_draft: bool, windowed: bool, on_step: bool = True) -> None:
    """What a session with cascade attention refuses, before any device work: what share_prefix refuses, and the runs whose
    target engine cannot take the cascade launch."""
    if not share_prefix:
        raise ValueError("cascade_attention reads what forked rows share: it needs share_prefix=True or n > 1")
    if pipe._fake or not on_step:
        raise NotImplementedError("cascade_attention needs the captured device step (implementation='hip'; policy 'longest_prefix', or "
                                  "'rejection' with backend='device')")
    if self_draft or pipe.config.get("draft_mode", "vanilla") != "vanilla" or pipe.medusa_heads is not None:
        raise NotImplementedError("cascade_attention needs the draft-model mode (draft_mode='vanilla'): medusa / eagle steps are not supported with it")
    if bool(getattr(pipe.controller, "per_row", False)):
        raise NotImplementedError("cascade_attention keeps a fixed K (controller='fixed'): adaptive K is not supported")
    if windowed:
        raise NotImplementedError("cascade_attention is not supported with context_window: a shared prefix does not move")
    if getattr(pipe.base_lm, "kv_cache_dtype", "bf16") == "fp8":
        raise NotImplementedError("cascade_attention is not available with kv_cache_dtype fp8 (an e4m3 cache is not forked)")


class CascadeGroups:
    def __init__(self, n_rows: int, min_shared: int = 32):
        self.leader: List[int] = list(range(n_rows))
        self.length: List[int] = [0] * n_rows
        self.min_shared = max(int(min_shared), 32)
        self._dirty: dict = {}       # row -> whether it was a member (named another row) at the last flush

    def _set(self, b: int, leader: int, length: int) -> None:
        if (self.leader[b], self.length[b]) != (leader, length):
            self._dirty.setdefault(b, self.leader[b] != b and self.length[b] > 0)
            self.leader[b], self.length[b] = leader, length

    def members(self, root: int) -> List[int]:
        """the rows that name `root`, the root itself excluded"""
        return [b for b in range(len(self.leader)) if b != root and self.leader[b] == root and self.length[b] > 0]

    def fork(self, b: int, src: int, n_pos: int) -> int:
        """Row b's first n_pos positions were copied from row src. -> the length b now shares with its root (0: in no group).
        leader(b) = root(src); the length is floor32(n_pos) when src is the root, else floor32(min(n_pos, shared_len(src))): b has
        in common with the root only what src has."""
        self.rewrite(b)
        root = self.leader[src] if self.length[src] > 0 else src
        n = int(n_pos) if root == src else min(int(n_pos), self.length[src])
        n = n // 32 * 32
        if b == root or n < self.min_shared:
            return 0
        self._set(b, root, n)
        self._set(root, root, max(self.length[root], n))
        return n

    def rewrite(self, b: int) -> None:
        """Row b's slot is about to be rewritten (an admission, a rebuild of the row): it leaves its group first. A root's
        lowest remaining member becomes the root, and every other member keeps min(its own length, the new root's); a group
        of one dissolves."""
        if self.length[b] == 0:
            return
        root = self.leader[b]
        self._set(b, b, 0)
        rest = self.members(root)
        if b != root:
            self._set(root, root, max((self.length[m] for m in rest), default=0))
            return
        if not rest:
            return
        new, others = rest[0], rest[1:]
        cap = self.length[new]
        for m in others:
            self._set(m, new, min(self.length[m], cap))
        self._set(new, new, max((self.length[m] for m in others), default=0))

    def flush(self) -> List[Tuple[int, int, int]]:
        """(row, leader, shared_len) of every entry that changed since the last flush: roots first, then members, then the rows that
        left every group, former members before former roots (the engine wants a member's leader to be a root when the member is written, and a row to have no members
        left when it stops being one)"""
        out = sorted(((3 - was_member) if self.length[b] == 0 else int(self.leader[b] != b), b) for b, was_member in self._dirty.items())
        self._dirty.clear()
        return [(b, self.leader[b], self.length[b]) for _, b in out]

    def stats(self) -> Tuple[int, int]:
        """(rows in a group, positions they read through their root instead of their own cache)"""
        rows = [b for b in range(len(self.leader)) if self.length[b] > 0]
        return len(rows), sum(self.length[b] for b in rows if self.leader[b] != b)
