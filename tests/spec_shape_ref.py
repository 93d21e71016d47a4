"""CPU restatement of top-k / top-p SHAPED speculative sampling (csrc/spec_sample.hip: the shaped variant), numpy float64.

TEST INFRASTRUCTURE ONLY. Built on oracle/sampling_ref.py (`filtered_distribution`, `draw_uniform`, `philox4x32_10`,
`sample_token_ref`), which it imports and does not change. For a bf16-valued logits row x, S(x) = filtered_distribution(x, T,
top_k, top_p): the kept ids in sorted order (value descending, index ascending), float64 weights e_j = exp(x_j/T - max), Z =
their sum added sequentially in sorted order; a row whose top value is not finite is the point mass on its first id.
x'(v) = e(v)/Z on the kept set, 0 elsewhere. Per row and step (c = the row's draw counter at the start of the step, sid = its
Philox stream, key = seed; Philox counter words are (draw, stream, element, tag)):

  1. d_{i+1}, i = 0..K-1 : the uniform of counter (c + i, sid, 0, TAG_CDF) inverted through S(q_i) in sorted order
                           (= sample_token_ref(q_i, T, top_k, top_p, seed, c + i, sid))
  2. u_i,     i = 0..K-1 : counter (c + i, sid, 0, TAG_ACCEPT = 0x5EED0003), u = r0 * 2^-32
  3. ratio_i = (e_p(d)/Z_p) / (e_q(d)/Z_q), d = d_{i+1}; e_p(d) = 0 when d is outside the target's kept set; d outside q's
     kept set: NaN (rejected). a = number of leading i with u_i < ratio_i
  4. next token, uniform u_n of counter (c + K, sid, 0, TAG_CDF):
       a < K : r_j = max(0, p'_a(id_j) - q'_a(id_j)) over the target's kept ids in the target's sorted order, Z_r summed
               sequentially, the first j with u_n Z_r < cum_j (the last kept id otherwise); Z_r == 0: the same inversion
               through e_p (= sample_token_ref(p_a, .., draw c + K))
       a == K: sample_token_ref(p_K, .., draw c + K)
  5. the counter advances by K + 1; inactive rows consume nothing.

Every decision that a last-bit difference of exp could flip reports its MARGIN: the relative |u_i - ratio_i| of a flag,
|u Z - cum_j| / Z to the nearest boundary of an inversion draw, |cum - top_p| at the nucleus cut of each row, and a residual
whose whole mass Z_r is positive but below the cap (rounding noise deciding between the residual and the target's own draw).
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional

import numpy as np

from oracle import sampling_ref as S

TAG_ACCEPT = 0x5EED0003
TINY = np.finfo(np.float64).tiny


def accept_uniform(seed: int, draw: int, stream: int) -> float:
    """u_i: the uniform of counter (draw, stream, 0, TAG_ACCEPT)."""
    x0 = S.philox4x32_10((draw & S.MASK32, stream & S.MASK32, 0, TAG_ACCEPT), (seed & S.MASK32, (seed >> 32) & S.MASK32))[0]
    return float(x0) * 2.0 ** -32


def seq_sum(w) -> float:
    z = 0.0
    for v in w:
        z += float(v)
    return z


@dataclass
class Kept:
    ids: np.ndarray            # kept token ids, sorted order
    e: np.ndarray              # float64 weights
    z: float                   # their sum, sequential
    cut: float = float("inf")  # min |cum - top_p| over the comparisons the nucleus cut made
    index: Dict[int, int] = field(default_factory=dict)

    def weight(self, tok: int) -> Optional[float]:
        j = self.index.get(int(tok))
        return None if j is None else float(self.e[j])


def kept_set(row, temperature: float, top_k: int, top_p: Optional[float]) -> Kept:
    x = np.asarray(row, dtype=np.float32)
    ids, e = S.filtered_distribution(x, temperature, top_k, top_p)
    cut = float("inf")
    if top_p is not None and float(np.float32(top_p)) < 1.0:
        ids_k, e_k = S.filtered_distribution(x, temperature, top_k, None)
        if len(e_k) > 1:       # (a point-mass row makes no comparison)
            tp, z, cum = float(np.float32(top_p)), seq_sum(e_k), 0.0
            for i in range(len(e_k)):
                cum += float(e_k[i]) / z
                if i > 0:
                    cut = min(cut, abs(cum - tp))
                    if cum > tp:
                        break
    return Kept(np.asarray(ids, dtype=np.int64), np.asarray(e, dtype=np.float64), seq_sum(e), cut, {int(t): j for j, t in enumerate(ids)})


def invert(w, z: float, u: float):
    """-> (index, margin): the first j with u z < cum_j (sequential), else the last; margin = |u z - nearest cum_j| / z."""
    target, c, margin = u * z, 0.0, float("inf")
    for j in range(len(w)):        # the cumulative sums do not decrease: the first one above the target is the nearest above
        c += float(w[j])
        margin = min(margin, abs(target - c) / z)
        if target < c:
            return j, margin
    return len(w) - 1, margin


def draft_draw_ref(q_row, temperature: float, top_k: int, top_p: Optional[float], seed: int, counter: int, i: int, stream: int,
                   kq: Optional[Kept] = None):
    """d_{i+1} -> (token, inversion margin)."""
    kq = kq or kept_set(q_row, temperature, top_k, top_p)
    j, margin = invert(kq.e, kq.z, S.draw_uniform(seed, (counter + i) & S.MASK32, stream))
    return int(kq.ids[j]), margin


def ratio_of(kp: Kept, kq: Kept, d: int) -> float:
    eq = kq.weight(d)
    if eq is None:
        return float("nan")
    ep = kp.weight(d) or 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        return float((np.float64(ep) / np.float64(kp.z)) / (np.float64(eq) / np.float64(kq.z)))


def residual_weights(kp: Kept, kq: Kept) -> np.ndarray:
    """r_j over the target's kept ids, in the target's sorted order."""
    r = np.zeros(len(kp.ids))
    for j, t in enumerate(kp.ids):
        eq = kq.weight(t) or 0.0
        v = float(kp.e[j]) / kp.z - eq / kq.z
        r[j] = v if v > 0.0 else 0.0
    return r


@dataclass
class Position:
    ratio: float = float("nan")
    u: float = 0.0
    flag: bool = False
    margin: float = float("inf")    # relative |u - ratio|
    cand: int = 0
    gap: float = float("inf")       # inversion margin of the candidate draw
    cut: float = float("inf")       # nucleus-cut margin of the rows of this position
    zr: float = 0.0                 # residual mass (0: the target's own draw)


@dataclass
class StepResult:
    accept_len: int
    next_tok: int
    positions: List[Position] = field(default_factory=list)

    @property
    def ratios(self) -> np.ndarray:
        return np.array([p.ratio for p in self.positions[:-1]], dtype=np.float64)

    def close_calls(self, cap: float = 1e-9) -> int:
        n = sum(1 for p in self.positions[:-1] if p.margin < cap)
        n += sum(1 for p in self.positions if p.gap < cap or p.cut < cap or 0.0 < p.zr < cap)
        return n


def position_ref(kp: Kept, kq: Optional[Kept], d: Optional[int], seed: int, c_flag: int, c_next: int, stream: int) -> Position:
    out = Position(cut=kp.cut if kq is None else min(kp.cut, kq.cut))
    un = S.draw_uniform(seed, c_next & S.MASK32, stream)
    w, z = kp.e, kp.z
    if kq is not None:
        out.u = accept_uniform(seed, c_flag, stream)
        out.ratio = ratio_of(kp, kq, int(d))
        out.flag = bool(out.u < out.ratio)
        if out.ratio == out.ratio:
            out.margin = abs(out.u - out.ratio) / max(out.ratio, TINY)
        r = residual_weights(kp, kq)
        out.zr = seq_sum(r)
        if out.zr > 0.0:
            w, z = r, out.zr
    j, out.gap = invert(w, z, un)
    out.cand = int(kp.ids[j])
    return out


def spec_accept_ref(q, p, draft_ids, temperature: float, top_k: int, top_p: Optional[float], seed: int, counter: int, stream: int,
                    kq: Optional[List[Kept]] = None) -> StepResult:
    """Steps 2-4 for one row: q [K][V], p [K+1][V], draft_ids [K]."""
    q, p = np.asarray(q, dtype=np.float32), np.asarray(p, dtype=np.float32)
    K = q.shape[0]
    assert p.shape[0] == K + 1 and len(draft_ids) == K
    kq = kq or [kept_set(q[i], temperature, top_k, top_p) for i in range(K)]
    kp = [kept_set(p[i], temperature, top_k, top_p) for i in range(K + 1)]
    pos = [position_ref(kp[i], kq[i], draft_ids[i], seed, counter + i, counter + K, stream) for i in range(K)]
    pos.append(position_ref(kp[K], None, None, seed, 0, counter + K, stream))
    a = 0
    while a < K and pos[a].flag:
        a += 1
    return StepResult(a, pos[a].cand, pos)


def spec_step_ref(q, p, temperature: float, top_k: int, top_p: Optional[float], seed: int, counter: int, stream: int, active: bool = True):
    """A whole step of one row from its stored logits: -> (draft ids, StepResult or None, emitted tokens, counter after, smallest
    inversion margin of the draft draws)."""
    q = np.asarray(q, dtype=np.float32)
    K = q.shape[0]
    if not active:
        return [], None, [], counter, float("inf")
    kq = [kept_set(q[i], temperature, top_k, top_p) for i in range(K)]
    draws = [draft_draw_ref(q[i], temperature, top_k, top_p, seed, counter, i, stream, kq[i]) for i in range(K)]
    d = [t for t, _ in draws]
    res = spec_accept_ref(q, p, d, temperature, top_k, top_p, seed, counter, stream, kq)
    return d, res, d[: res.accept_len] + [res.next_tok], counter + K + 1, min(m for _, m in draws)
