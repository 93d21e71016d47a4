"""CPU restatement of speculative sampling inside the step (csrc/spec_sample.hip), numpy float64.

TEST INFRASTRUCTURE ONLY. Built on oracle/sampling_ref.py (Philox4x32-10, the CDF uniform, the Gumbel-max draw), which it
imports and does not change. Per row and step (T = temperature > 0 as the device holds it, a float32; c = the row's draw
counter at the start of the step; sid = the row's Philox stream; key = seed), over bf16-valued logits rows:

  d_{i+1}, i = 0..K-1 : gumbel_argmax_ref(q_i, T, seed, c + i, sid)
  u_i,     i = 0..K-1 : draw_uniform(seed, c + i, sid)
  ratio_i             = exp((p_i[d]/T - lse(p_i/T)) - (q_i[d]/T - lse(q_i/T))),  lse(v) = max v + log(sum exp(v - max v))
  a                   = number of leading i with u_i < ratio_i
  next token          : Gumbel-max with counter (c + K, sid, element, Gumbel tag) over
                          a < K : log r_v, r_v = exp(p_a[v]/T - lse p_a) - exp(q_a[v]/T - lse q_a), on the v with r_v > 0
                                  (no such v: over p_a[v]/T)
                          a == K: p_K[v]/T
  the counter advances by K + 1; inactive rows consume nothing.
A position whose p or q row holds a NaN or has a non-finite maximum is rejected (ratio NaN) and its candidate is the plain
Gumbel-max over p_i/T (NaN scores first, lowest index among equals).

Every decision that a last-bit difference of exp / log / the summation order could flip reports its MARGIN: the relative
|u_i - ratio_i| of a flag and the gap between the two largest Gumbel scores of a draw.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

import numpy as np

from oracle import sampling_ref as S


def scaled(x, temperature: float) -> np.ndarray:
    """x / T in float64 with T the float32 temperature; no division when T == 1 (as the kernels)."""
    v = np.asarray(x, dtype=np.float32).astype(np.float64)
    T = float(np.float32(temperature))
    return v / T if T != 1.0 else v


def gumbel_noise(V: int, seed: int, draw: int, stream: int) -> np.ndarray:
    r = S.philox4x32_10((np.full(V, draw & S.MASK32, dtype=np.uint64), np.full(V, stream & S.MASK32, dtype=np.uint64),
                         np.arange(V, dtype=np.uint64), np.full(V, S.TAG_GUMBEL, dtype=np.uint64)),
                        (seed & S.MASK32, (seed >> 32) & S.MASK32))[0]
    u = (r.astype(np.float64) + 0.5) * 2.0 ** -32
    return -np.log(-np.log(u))


def best_of(score: np.ndarray, valid: Optional[np.ndarray] = None):
    """-> (index, gap to the runner-up) under the device's order: NaN first, then value, then lowest index.
    gap = 0 for a tie, inf when there is no runner-up."""
    idx = np.arange(score.shape[0]) if valid is None else np.nonzero(valid)[0]
    sc = score[idx]
    if np.isnan(sc).any():
        return int(idx[np.argmax(np.isnan(sc))]), float("inf")
    k = int(np.argmax(sc))
    if sc.shape[0] < 2:
        return int(idx[k]), float("inf")
    rest = np.delete(sc, k)
    with np.errstate(invalid="ignore"):
        gap = float(sc[k] - rest.max())
    return int(idx[k]), (gap if gap == gap else 0.0)


def lse(v: np.ndarray) -> float:
    m = v.max()
    return float(m + np.log(np.exp(v - m).sum()))


def row_is_finite(v: np.ndarray) -> bool:
    return not np.isnan(v).any() and bool(np.isfinite(v.max()))


def next_weights(p_row, q_row, temperature: float) -> np.ndarray:
    """Unnormalised weights of the redraw at a rejected position: max(0, softmax(p/T) - softmax(q/T)), or softmax(p/T) when
    that is zero everywhere."""
    vp, vq = scaled(p_row, temperature), scaled(q_row, temperature)
    r = np.exp(vp - lse(vp)) - np.exp(vq - lse(vq))
    r = np.where(r > 0, r, 0.0)
    return r if (r > 0).any() else np.exp(vp - lse(vp))


@dataclass
class Position:
    ratio: float = float("nan")
    u: float = 0.0
    flag: bool = False
    margin: float = float("inf")    # relative |u - ratio|
    cand: int = 0
    gap: float = float("inf")       # top-2 Gumbel-score gap of the candidate draw


@dataclass
class StepResult:
    accept_len: int
    next_tok: int
    positions: List[Position] = field(default_factory=list)

    @property
    def ratios(self) -> np.ndarray:
        return np.array([p.ratio for p in self.positions[:-1]], dtype=np.float64)

    def close_calls(self, cap: float = 1e-9) -> int:
        """decisions within `cap` of a tie: flags by their relative margin, candidate draws by their score gap"""
        n = sum(1 for p in self.positions[:-1] if p.margin < cap)
        return n + sum(1 for p in self.positions if p.gap < cap)


def position_ref(p_row, q_row, d: Optional[int], temperature: float, seed: int, c_flag: int, c_next: int, stream: int) -> Position:
    """One verify position: q_row / d None for position K (bonus draw only)."""
    out = Position()
    vp = scaled(p_row, temperature)
    V = vp.shape[0]
    g = gumbel_noise(V, seed, c_next, stream)
    residual = False
    if q_row is not None:
        vq = scaled(q_row, temperature)
        d = min(max(int(d), 0), V - 1)
        out.u = S.draw_uniform(seed, c_flag & S.MASK32, stream)
        if row_is_finite(vp) and row_is_finite(vq):
            lp, lq = lse(vp), lse(vq)
            out.ratio = float(np.exp((vp[d] - lp) - (vq[d] - lq)))
            out.flag = bool(out.u < out.ratio)
            out.margin = abs(out.u - out.ratio) / max(out.ratio, np.finfo(np.float64).tiny)
            with np.errstate(over="ignore"):
                r = np.exp(vp - lp) - np.exp(vq - lq)
            pos = r > 0
            if pos.any():
                with np.errstate(divide="ignore", invalid="ignore"):
                    score = np.where(pos, np.log(np.where(pos, r, 1.0)), -np.inf) + g
                out.cand, out.gap = best_of(score, pos)
                residual = True
    if not residual:
        with np.errstate(invalid="ignore"):
            out.cand, out.gap = best_of(vp + g)
    return out


def spec_accept_ref(q, p, draft_ids, temperature: float, seed: int, counter: int, stream: int) -> StepResult:
    """Steps 3 and 4 for one row: q [K][V], p [K+1][V], draft_ids [K] -> accept length, next token, per-position details."""
    q, p = np.asarray(q, dtype=np.float32), np.asarray(p, dtype=np.float32)
    K = q.shape[0]
    assert p.shape[0] == K + 1 and len(draft_ids) == K
    pos = [position_ref(p[i], q[i], draft_ids[i], temperature, seed, counter + i, counter + K, stream) for i in range(K)]
    pos.append(position_ref(p[K], None, None, temperature, seed, 0, counter + K, stream))
    a = 0
    while a < K and pos[a].flag:
        a += 1
    return StepResult(a, pos[a].cand, pos)


def draft_draw_ref(q_row, temperature: float, seed: int, counter: int, i: int, stream: int) -> int:
    """d_{i+1}: the Gumbel-max draw over q_i / T."""
    return S.gumbel_argmax_ref(np.asarray(q_row, dtype=np.float32), temperature, seed, (counter + i) & S.MASK32, stream)


def spec_step_ref(q, p, temperature: float, seed: int, counter: int, stream: int, active: bool = True):
    """A whole step of one row from its stored logits: -> (draft ids, StepResult or None, emitted tokens, counter after).
    The draft ids are the draws of the stored q rows (which the device made while it produced them)."""
    K = np.asarray(q).shape[0]
    if not active:
        return [], None, [], counter
    d = [draft_draw_ref(q[i], temperature, seed, counter, i, stream) for i in range(K)]
    res = spec_accept_ref(q, p, d, temperature, seed, counter, stream)
    return d, res, d[: res.accept_len] + [res.next_tok], counter + K + 1
