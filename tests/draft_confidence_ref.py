"""float64 restatement of the confidence-gated draft length (csrc/draft_confidence.hip, sd_specdec_set_draft_confidence), the planted
rows the op test runs, and the op's error bound.

conf(row) = 1 / sum_v exp(x_v - max_v x_v) over the STORED values (bf16 / f16 / f32 widened to float64): the temperature-1 softmax
probability of the row's largest value. An entry at -inf adds 0; a row with a NaN, a +inf, or nothing above -inf gives NaN.
k_rule(confs, tau, min_k): the smallest i + 1 >= min_k with not (c_i >= tau), else K = len(confs); a NaN stops the row.
margins(confs, tau, min_k): |c_i - tau| of every decision the rule makes on the way (the judged forwards up to the stop)."""

import math

import numpy as np

import typical_ref

NEG = float("-inf")
NAN = float("nan")


def conf(row) -> float:
    x = np.asarray(row, dtype=np.float64)
    if np.isnan(x).any():
        return NAN
    m = x.max()
    if not np.isfinite(m):                       # +inf on top, or every entry -inf
        return NAN
    fin = x > NEG
    return float(1.0 / np.exp(x[fin] - m).sum())


def judged(K: int, min_k: int):
    """The forwards whose confidence is looked at: i = min_k - 1 .. K - 2 (forward K - 1 needs no judgement)."""
    return range(min_k - 1, K - 1)


def k_rule(confs, tau: float, min_k: int) -> int:
    K = len(confs)
    for i in judged(K, min_k):
        if not (confs[i] >= tau):
            return i + 1
    return K


def margins(confs, tau: float, min_k: int):
    out = []
    for i in judged(len(confs), min_k):
        out.append(abs(confs[i] - tau) if confs[i] == confs[i] else float("inf"))   # (a NaN stop does not hinge on rounding)
        if not (confs[i] >= tau):
            break
    return out


# --------------------------------------------------------------------------------------------------------- planted rows
def planted_rows(V: int):
    """[(name, row float64 [V], expected confidence (NaN: the row must give NaN))]. Every value is exact in bf16 / f16 / f32, so the
    expectation holds for the stored row whatever the dtype."""
    d = (7 * V) // 11 % V
    rows = []
    one = np.full(V, NEG)
    one[d] = 1.5
    rows.append(("one_hot", one, 1.0))                                     # every other entry adds exactly 0
    rows.append(("flat", np.full(V, -2.0), 1.0 / V))
    for n in (2, 3):
        if V >= 2 * n:
            r = np.full(V, -30.0)
            r[[(d + 3 * j) % V for j in range(n)]] = 4.0
            # n equal maxima over a floor 34 below them: 1 / (n + (V - n) e^-34), 1/n to 1e-12 for any V here
            rows.append((f"{n}_maxima", r, 1.0 / (n + (V - n) * math.exp(-34.0))))
    if V >= 4:
        half = np.zeros(V)
        half[1::2] = NEG
        rows.append(("half_masked", half, 1.0 / len(half[0::2])))
    nan = np.zeros(V)
    nan[d] = NAN
    rows.append(("nan", nan, NAN))
    if V >= 2:
        nan_low = np.full(V, 3.0)
        nan_low[(d + 1) % V] = NAN                                        # a NaN that is not where the maximum is
        rows.append(("nan_beside_max", nan_low, NAN))
    inf = np.zeros(V)
    inf[d] = float("inf")
    rows.append(("pos_inf", inf, NAN))
    rows.append(("all_neg_inf", np.full(V, NEG), NAN))
    return rows


def random_rows(B: int, V: int, scale: float, seed: int):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, V)) * scale
    x[rng.random((B, V)) < 0.01] = NEG
    x[:, 0] = np.where(np.isneginf(x[:, 0]), 0.0, x[:, 0])                 # (never a row of -inf alone)
    return x


# --------------------------------------------------------------------------------------------------- the device's error bound
def width(dtype_name: str, V: int, aligned: bool) -> int:
    """Elements per load of the row walker (csrc/sample_device.h): 8 for a 16-byte aligned bf16 row with V % 8 == 0, 4 for an
    aligned f32 row with V % 4 == 0, else 1 (f16 rows are always walked element by element)."""
    if dtype_name == "bf16" and aligned and V % 8 == 0:
        return 8
    if dtype_name == "f32" and aligned and V % 4 == 0:
        return 4
    return 1


def bound(row, dtype_name: str, aligned: bool) -> float:
    """Relative bound of the device's confidence for a stored row. The kernel keeps typical_row_kernel's summation shape (the same
    running-maximum stream per thread, the 6 xor merges, the 15 wave-partial merges; T = 1 only drops an exact division), so S
    carries the relative error typical_ref.bounds derives for it, and c = 1 / S adds one division: the `p` bound at t_d = 0, the
    probability of the maximum, whose e^{t_d} = 1 is exact."""
    x = np.asarray(row, dtype=np.float64)
    V = x.shape[0]
    fin = x > NEG
    t = x[fin] - x[fin].max()
    e = np.exp(t)
    S = e.sum()
    M1 = float((np.abs(t) * e).sum() / S)
    M2 = float((t * t * e).sum() / S)
    _, e_p, _, _ = typical_ref.bounds(V, width(dtype_name, V, aligned), math.log(S), M1, M2, 0.0, 0.0)
    return e_p
