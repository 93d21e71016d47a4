"""CPU restatement of the draft-target agreement op (csrc/spec_agree.hip, sd_spec_agreement), numpy float64.

TEST INFRASTRUCTURE ONLY. Per pair of bf16-valued rows P (target) and Q (draft), T the float32 temperature (x / T in float64, no
division when T == 1, as tests/spec_sample_ref.py `scaled`):

  a_v = P[v]/T - lse(P/T),  b_v = Q[v]/T - lse(Q/T),  lse(x) = max x + log(sum exp(x - max x))
  alpha = sum_v min(exp a_v, exp b_v)
  kl    = sum over the v with P[v] > -inf of exp(a_v) (a_v - b_v); a Q[v] = -inf under a finite P[v] contributes +inf
  p_arg, q_arg = argmax ids, NaN first, then larger value, then lower index; agree = (p_arg == q_arg)
A pair in which either row holds a NaN, or has a non-finite maximum (+inf present, or every entry -inf), gives alpha = kl = NaN.

`bounds` is the distance allowed between two float64 evaluations of these formulas that differ in summation order and in the last
bit of exp / log (the device against this file, or two forms of one identity here). Derivation, u = 2^-53, to first order:
  * exp and log are taken to be within one ulp: relative 2u.
  * S = sum_v exp(x_v/T - M): every term carries exp's 2u and its argument's rounding u |x_v/T - M| <= u (Amax + log V), where
    Amax = max |a_v| over the finite entries (|x/T - M| <= |a_v| + |lse - M| and 0 <= lse - M <= log V); adding V terms in any
    order costs at most V u relative; the device folds slice sums s_k exp(m_k - M): one more exp, its argument and a product,
    2u + u (Amax + log V) + u. So S is within eS = u (V + 5 + 2 (Amax + log V)) relative.
  * lse = M + log S: log S moves by eS + 2u log V, the sum rounds by u |lse| <= u (X + log V), X = max |x_v / T| over the finite
    entries of both rows: d_lse = eS + u (X + 3 log V).
  * a_v: the division rounds by u X, the subtraction by u |a_v|: d_a = u (X + Amax) + d_lse; exp(a_v) is then within
    (2u + d_a) relative. The same for b with Bmax.
  * alpha: min is 1-Lipschitz in each argument, so the terms move by at most exp(a_v)(2u + d_a) + exp(b_v)(2u + d_b), which sum
    (sum exp a_v = sum exp b_v = 1) to 4u + d_a + d_b; adding V terms in [0, 1] whose sum is <= 1 costs V u.
      B_alpha = 2 (V u + 4u + d_a + d_b)                                (the 2: either evaluation may be off by this much)
  * kl: the term t_v = exp(a_v)(a_v - b_v) moves by |a_v - b_v| exp(a_v)(2u + d_a)  [exp]  + exp(a_v)(d_a + d_b + u |a_v - b_v|)
    [the difference] + u |t_v| [the product]; with T1 = sum_v |t_v| these sum to T1 (4u + d_a) + d_a + d_b; adding V signed
    terms costs V u T1.       B_kl = 2 (T1 (V u + 4u + d_a) + d_a + d_b)
    T1 <= kl + 2 (for b > a, exp(a)(b - a) <= exp(b) - exp(a) by convexity, so the negative terms sum to at most 1 in size).
Every input of the bounds (V, X, Amax, Bmax, T1) is computed here from the rows; nothing is fitted to a device output.
"""

from __future__ import annotations

import math
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

U = 2.0 ** -53


class Agreement(NamedTuple):
    alpha: float
    kl: float
    agree: bool
    p_arg: int
    q_arg: int


def scaled(x, temperature: float) -> np.ndarray:
    v = np.asarray(x, dtype=np.float32).astype(np.float64)
    T = float(np.float32(temperature))
    return v / T if T != 1.0 else v


def argmax_nan_first(x: np.ndarray) -> int:
    """NaN first, then the larger value, then the lower index (argmax_better / sample_gumbel_kernel)."""
    nan = np.isnan(x)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(x))   # first occurrence of the maximum; -0 == +0


def lse(v: np.ndarray) -> float:
    m = v.max()
    return float(m + np.log(np.exp(v - m).sum()))


def row_ok(v: np.ndarray) -> bool:
    return not np.isnan(v).any() and bool(np.isfinite(v.max()))


def _log_probs(p_row, q_row, temperature):
    vp, vq = scaled(p_row, temperature), scaled(q_row, temperature)
    return vp, vq, vp - lse(vp), vq - lse(vq)


def agreement_row(p_row, q_row, temperature: float = 1.0) -> Agreement:
    p32, q32 = np.asarray(p_row, dtype=np.float32), np.asarray(q_row, dtype=np.float32)
    pa, qa = argmax_nan_first(p32), argmax_nan_first(q32)
    vp, vq = scaled(p32, temperature), scaled(q32, temperature)
    if not (row_ok(vp) and row_ok(vq)):
        return Agreement(float("nan"), float("nan"), pa == qa, pa, qa)
    a, b = vp - lse(vp), vq - lse(vq)
    alpha = float(np.minimum(np.exp(a), np.exp(b)).sum())
    sup = vp > -np.inf
    if (sup & (vq == -np.inf)).any():
        kl = float("inf")
    else:
        kl = float((np.exp(a[sup]) * (a[sup] - b[sup])).sum())
    return Agreement(alpha, kl, pa == qa, pa, qa)


def agreement_ref(p, q, temperature: float = 1.0) -> List[Agreement]:
    """target rows p [n][V], draft rows q [n][V] -> one Agreement per row"""
    p, q = np.asarray(p, dtype=np.float32), np.asarray(q, dtype=np.float32)
    assert p.shape == q.shape and p.ndim == 2
    return [agreement_row(p[t], q[t], temperature) for t in range(p.shape[0])]


def tv_alpha(p_row, q_row, temperature: float = 1.0) -> float:
    """1 - (1/2) sum |p - q|: the other form of alpha (finite rows)."""
    _, _, a, b = _log_probs(p_row, q_row, temperature)
    return float(1.0 - 0.5 * np.abs(np.exp(a) - np.exp(b)).sum())


def bounds(p_row, q_row, temperature: float = 1.0):
    """(B_alpha, B_kl) of the module docstring for one pair of rows without NaN and with finite maxima; B_kl is inf where kl is."""
    vp, vq, a, b = _log_probs(p_row, q_row, temperature)
    V = vp.shape[0]
    fin_p, fin_q = np.isfinite(vp), np.isfinite(vq)
    X = max(float(np.abs(vp[fin_p]).max()), float(np.abs(vq[fin_q]).max()))
    amax, bmax = float(np.abs(a[fin_p]).max()), float(np.abs(b[fin_q]).max())
    logv = math.log(V) if V > 1 else 0.0

    def d_arg(m):
        e_s = U * (V + 5 + 2 * (m + logv))
        d_lse = e_s + U * (X + 3 * logv)
        return U * (X + m) + d_lse

    d_a, d_b = d_arg(amax), d_arg(bmax)
    b_alpha = 2 * (V * U + 4 * U + d_a + d_b)
    both = fin_p & fin_q
    if (fin_p & ~fin_q).any():
        return b_alpha, float("inf")
    t1 = float(np.abs(np.exp(a[both]) * (a[both] - b[both])).sum())
    return b_alpha, 2 * (t1 * (V * U + 4 * U + d_a) + d_a + d_b)


def expected_tokens_loop(alpha: Sequence[float], K: int) -> Optional[float]:
    """mean over the windows t = 0 .. len(alpha) - K of sum_{j=0..K} prod_{i<j} alpha[t+i], written out term by term"""
    n = len(alpha)
    if n - K + 1 < 1:
        return None
    tot = 0.0
    for t in range(n - K + 1):
        for j in range(K + 1):
            prod = 1.0
            for i in range(j):
                prod *= float(alpha[t + i])
            tot += prod
    return tot / (n - K + 1)
