"""Restatement of the rolling context window (csrc/kv_evict.hip, DecodeSession's rolls) for the tests: test infrastructure only,
no conftest. Three things are stated here once:

  * the move: positions [keep + drop, n_pos) of a cache row become positions [keep, n_pos - drop); V as it is, K rotated by -drop
    positions with row `drop` of the model's fp32 RoPE tables — rotate-half pairs (i, i + D/2), a' = a c + b s, b' = b c - a s;
  * the bound of a rotated K element against fp64: one bf16 rounding of the result (half an ulp of bf16's 8 significant bits is at
    most 2^-8 |want|) plus two fp32 products and one fp32 addition (3 x 2^-24 (|a c| + |b s|)). Derived from the formats, not
    from what a kernel gives;
  * the replay of a run under a schedule of (tokens generated before the roll, drop) events on an oracle's own cache.
"""

from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

F64 = torch.float64


def rotate_back(k: torch.Tensor, cos_row: torch.Tensor, sin_row: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """k [..., D] (any float dtype; the stored values) rotated by -drop in fp64 with the table rows cos_row / sin_row [D/2] ->
    (want fp64 [..., D], bound fp64 [..., D] on |got - want| for a bf16 result computed in fp32)"""
    D = k.shape[-1]
    a, b = k[..., : D // 2].to(F64), k[..., D // 2:].to(F64)
    c, s = cos_row.to(F64).cpu().to(k.device), sin_row.to(F64).cpu().to(k.device)
    want = torch.cat([a * c + b * s, b * c - a * s], -1)
    mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1)
    return want, 2.0 ** -8 * want.abs() + 3 * 2.0 ** -24 * mag


def evicted_cache(k: torch.Tensor, v: torch.Tensor, row: int, keep: int, drop: int, n_pos: int, cos_row, sin_row):
    """The caches of an engine (kv_view(): k bf16 [layers][B][Hkv][Lmax][D], v bf16 [layers][B][Hkv][D][Lmax]) after
    evict_row(row, keep, drop, n_pos) -> (want_k fp64, bound_k fp64 — zero wherever K must keep its bits —, want_v int16 bits)."""
    want_k = k.to(F64).clone()
    bound = torch.zeros_like(want_k)
    want_v = v.view(torch.int16).clone()
    m = n_pos - keep - drop
    if m > 0:
        rot, bnd = rotate_back(k[:, row, :, keep + drop:n_pos], cos_row, sin_row)
        want_k[:, row, :, keep:keep + m] = rot
        bound[:, row, :, keep:keep + m] = bnd
        want_v[:, row, :, :, keep:keep + m] = v.view(torch.int16)[:, row, :, :, keep + drop:n_pos]
    return want_k, bound, want_v


def roll_past(past, keep: int, drop: int, cos_row: torch.Tensor, sin_row: torch.Tensor, round_bf16: bool = True, rotate: bool = True):
    """An oracle's cache (OracleLM: per layer (k, v), each fp32 [B][Hkv][L][D]) rolled the way the kernel rolls a row that holds L
    positions: [keep + drop, L) -> [keep, L - drop), the moved K rotated in fp64 and rounded to bf16 (round_bf16) as the kernel stores
    it. rotate=False is the planted defect "moved, not rotated"."""
    out = []
    for k, v in past:
        ks = k[:, :, keep + drop:]
        if rotate:
            ks = rotate_back(ks, cos_row, sin_row)[0]
        ks = ks.to(torch.float32)
        if round_bf16:
            ks = ks.to(torch.bfloat16).to(torch.float32)
        out.append((torch.cat([k[:, :, :keep], ks], 2), torch.cat([v[:, :, :keep], v[:, :, keep + drop:]], 2)))
    return out


class RolledOracle:
    """One row's cache in an OracleLM: feed(tokens) appends them at the cache's own positions and gives their logits rows,
    roll(drop) evicts the `drop` positions after the sinks the way the kernel does. The callers below apply a schedule."""

    def __init__(self, lm, sinks: int, cos: torch.Tensor, sin: torch.Tensor, round_bf16: bool = True, rotate: bool = True):
        self.lm, self.sinks, self.cos, self.sin = lm, int(sinks), cos, sin
        self.round_bf16, self.rotate = round_bf16, rotate
        self.past = None

    def cached(self) -> int:
        return 0 if self.past is None else int(self.past[0][0].shape[2])

    def feed(self, tokens: Sequence[int]) -> torch.Tensor:
        """tokens appended at the cache's own positions -> logits fp32 [len(tokens)][V]"""
        lg, self.past = self.lm.forward(torch.tensor([list(tokens)], dtype=torch.long), self.past)
        return lg[0]

    def roll(self, drop: int) -> None:
        self.past = roll_past(self.past, self.sinks, drop, self.cos[drop], self.sin[drop], self.round_bf16, self.rotate)


def replay_logits(lm, prompt: Sequence[int], generated: Sequence[int], evictions: Sequence[Tuple[int, int]], sinks: int, cos, sin,
                  round_bf16: bool = True, rotate: bool = True, rebuilds: Sequence[int] = ()) -> torch.Tensor:
    """The logits row that precedes every generated token ([len(generated)][V]) when prompt + generated is teacher-forced through
    `lm` and the cache — which holds every token but the last one, as a session's does — is rolled at each event (g, drop): after g
    generated tokens, before the forward that consumes generated[g - 1]. rebuilds: the g at which the session rebuilt the row's
    cache from the tokens it still holds (a resync of a rolled row): the oracle's is recomputed from them too."""
    ro = RolledOracle(lm, sinks, cos, sin, round_bf16, rotate)
    events = list(evictions)
    rebuilds = list(rebuilds)
    kept = list(prompt)                       # the tokens whose positions the cache still holds, plus the pending last one
    rows = []
    if len(kept) > 1:
        ro.feed(kept[:-1])
    for g in range(len(generated) + 1):
        while rebuilds and rebuilds[0] == g:
            rebuilds.pop(0)
            ro.past = None
            ro.feed(kept[:-1])
        while events and events[0][0] == g:
            _, drop = events.pop(0)
            assert ro.cached() == len(kept) - 1
            ro.roll(drop)
            del kept[sinks:sinks + drop]
        if g == len(generated):
            break
        rows.append(ro.feed(kept[-1:])[0])    # the pending token goes in; its logits choose generated[g]
        kept.append(int(generated[g]))
    assert not events, events
    return torch.stack(rows)


def greedy_replay(lm, prompt: Sequence[int], n_tokens: int, evictions: Sequence[Tuple[int, int]], sinks: int, cos, sin) -> List[int]:
    """The oracle's own greedy decoding of n_tokens under the schedule (first argmax, as the device's)."""
    ro = RolledOracle(lm, sinks, cos, sin)
    events = list(evictions)
    kept = list(prompt)
    out: List[int] = []
    if len(kept) > 1:
        ro.feed(kept[:-1])
    for g in range(n_tokens):
        while events and events[0][0] == g:
            _, drop = events.pop(0)
            ro.roll(drop)
            del kept[sinks:sinks + drop]
        tok = int(ro.feed(kept[-1:])[0].argmax())
        out.append(tok)
        kept.append(tok)
    return out


def rope_fp64(cfg, positions: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """cos / sin [n][D/2] in fp64 from scratch (default RoPE frequencies, no scaling): theta^(-2i/D) * position"""
    D = cfg.head_dim
    inv = 1.0 / (torch.tensor(float(cfg.rope_theta), dtype=F64) ** (torch.arange(0, D, 2, dtype=F64) / D))
    ang = positions.to(F64).unsqueeze(1) * inv.unsqueeze(0)
    return ang.cos(), ang.sin()
