"""float64 restatement of csrc/token_logprobs.hip: one logits row and one token -> (logprob, rank, top-N), and the device's bound.

Over the STORED values x (bf16 / f16 / f32 widened to float64), at temperature 1, with m = max x and S = sum e^{x - m} (a -inf
element adds 0):
    logprob(t) = (x_t - m) - log S                      -inf for a token at -inf
    rank(t)    = #{v : x_v > x_t, or x_v == x_t and v < t}
    top N      the N = min(top_n, V) largest entries, value descending, index ascending: (id, logprob); entries at -inf follow in
               that order with logprob -inf
A row with no finite element: logprob NaN, rank -1, top ids -1 (log-probs NaN) — the "no record" value.
"""

import math

import numpy as np

import typical_ref

NEG = float("-inf")
NAN = float("nan")
FLT_MAX = float(np.finfo(np.float32).max)


def row_logprobs(x, t, top_n=0):
    """(logprob, rank, top_ids [N], top_logprobs [N], moments) of token t in row x; moments = (log S, M1, t_d) with M1 = sum |x - m| p:
    what `bounds` is stated in (None for a row with no finite element)."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    assert 0 <= t < V
    N = min(int(top_n), V)
    fin = x > NEG
    if not fin.any():
        return NAN, -1, np.full(N, -1, dtype=np.int64), np.full(N, NAN), None
    m = x[fin].max()
    d = np.where(fin, x - m, NEG)
    e = np.where(fin, np.exp(np.where(fin, d, 0.0)), 0.0)
    S = e.sum()
    logS = math.log(S)
    lp_all = np.where(fin, d - logS, NEG)
    rank = int(((x > x[t]) | ((x == x[t]) & (np.arange(V) < t))).sum())
    order = np.argsort(-x, kind="stable")[:N]          # value descending, index ascending
    M1 = float((np.abs(np.where(fin, d, 0.0)) * e).sum() / S)
    t_d = float(d[t]) if fin[t] else 0.0
    return float(lp_all[t]), rank, order.astype(np.int64), lp_all[order], (logS, M1, t_d)


def bounds(V, width, logS, M1, t_d):
    """Absolute bound of a log-prob (x_d - m) - log S computed by the device, t_d = x_d - m.

    The stream of S is typical_accept.hip's at T = 1 (typical_ref.bounds: e_S, the relative bound of S; the division by T that its
    2 U (M1 + 1) term carries is the identity here, so the term is generous). On top of it:
        log S        |d log S| <= e_S (1 + e_S) <= 1.01 e_S, then logf: 1 ulp of |log S|
        x_d - m      one fp32 subtraction: U |t_d|
        the result   one fp32 subtraction: U (|t_d| + |log S|) (1 + ...)
    """
    e_S = typical_ref.bounds(V, width, logS, M1, 0.0, t_d, 0.0)[0]
    return 1.01 * e_S + typical_ref.U_FN * abs(logS) + typical_ref.U * abs(t_d) + 1.01 * typical_ref.U * (abs(t_d) + abs(logS))


def check_row(x, t, top_n, width, got, worst=None):
    """Assert one device record against the restatement. got = (logprob, rank, top_ids, top_logprobs) as numbers / arrays; the exact
    parts (rank, ids, the -inf / NaN pattern) must be equal, the finite log-probs within `bounds`. Returns measured / bound (max)."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    lp, rank, ids, lps, mom = row_logprobs(x, t, top_n)
    g_lp, g_rank, g_ids, g_lps = float(got[0]), int(got[1]), np.asarray(got[2]), np.asarray(got[3], dtype=np.float64)
    assert g_rank == rank, (g_rank, rank)
    assert g_ids.tolist() == ids.tolist(), (g_ids.tolist(), ids.tolist())
    ratio = 0.0
    if mom is None:
        assert math.isnan(g_lp) and np.isnan(g_lps).all()
        return ratio
    logS, M1, _ = mom
    m = x[x > NEG].max()
    for want, have, xv in [(lp, g_lp, x[t])] + [(lps[j], g_lps[j], x[ids[j]]) for j in range(len(ids))]:
        if want < -FLT_MAX * (1 + typical_ref.U):     # past what fp32 holds (x_t - m between bf16's two ends): the result format's -inf
            want = NEG
        if want == NEG:
            assert have == NEG, (want, have)
            continue
        bound = bounds(V, width, logS, M1, xv - m)
        err = abs(have - want)
        ratio = max(ratio, err / bound)
        if worst is not None:
            worst["ratio"] = max(worst.get("ratio", 0.0), err / bound)
            worst["abs"] = max(worst.get("abs", 0.0), err)
        assert err <= bound, (want, have, err, bound)
    return ratio


def none_record(got):
    """True iff `got` is the "no record" value (nothing emitted at that position)."""
    return (math.isnan(float(got[0])) and int(got[1]) == -1 and (np.asarray(got[2]) == -1).all()
            and np.isnan(np.asarray(got[3], dtype=np.float64)).all())
