"""float64 restatement of the lossy acceptance rules of csrc/typical_accept.hip, and the cases the device tests run.

Row (b, i), i < K, of a [B][K+1][V] logits block is the target's distribution where d_{i+1} = draft_ids[b][i] was proposed. With
z = x / T over the STORED values (bf16 / f16 / f32 widened to float64):
    S = sum e^{z - m},  W = sum (z - m) e^{z - m}  (a -inf element adds 0 to both),  H = log S - W / S,  p_d = e^{z_d - m} / S
    rank_d = #{v : x_v > x_d, or x_v == x_d and v < d}
    rule "typical":    keep iff p_d >= min(eps, delta * exp(-H))   (delta None / inf: the fixed threshold eps)
    rule "topk_agree": keep iff rank_d < k
accept_len = the leading run of kept positions. `margin` of a position = |p_d - thr| / thr: how far the decision is from flipping.
"""

import math

import numpy as np

NEG = float("-inf")


def row_stats(x, d, T=1.0):
    """(p_d, H, rank_d, moments) of one row x (any float dtype -> float64) for draft id d. moments = (log S, M1, M2) with
    M1 = sum |t| p, M2 = sum t^2 p, t = z - m: what the device's error bound is stated in."""
    x = np.asarray(x, dtype=np.float64)
    V = x.shape[0]
    ok = 0 <= d < V
    fin = x > NEG
    m = x[fin].max() if fin.any() else NEG
    t = (np.where(fin, x, m) - m) / T if fin.any() else np.zeros(V)
    e = np.where(fin, np.exp(t), 0.0)
    S = e.sum()
    W = (t * e).sum()
    H = math.log(S) - W / S if S > 0 else float("nan")
    xd = x[d] if ok else NEG
    pd = float(e[d] / S) if (ok and xd > NEG and S > 0) else 0.0
    rank = int(((x > xd) | ((x == xd) & (np.arange(V) < d))).sum()) if ok else V
    M1 = float((np.abs(t) * e).sum() / S) if S > 0 else 0.0
    M2 = float((t * t * e).sum() / S) if S > 0 else 0.0
    return pd, H, rank, (math.log(S) if S > 0 else NEG, M1, M2)


def threshold(H, eps, delta):
    if delta is None or math.isinf(delta):
        return eps
    return min(eps, delta * math.exp(-H))


def decide(x, d, rule, T=1.0, eps=0.09, delta=0.3, k=1):
    """(keep, p_d, H, thr, rank_d, margin) for one row."""
    pd, H, rank, _ = row_stats(x, d, T)
    if rule == "typical":
        thr = threshold(H, eps, delta)
        keep = bool(pd >= thr) if H == H else False
        margin = abs(pd - thr) / thr if H == H else float("inf")
    else:
        thr = float(k)
        keep = rank < k
        margin = float("inf")           # an integer comparison: nothing to round
    return keep, pd, H, thr, rank, margin


def accept(logits, draft_ids, rule, T=1.0, eps=0.09, delta=0.3, k=1):
    """logits [B][K+1][V], draft_ids [B][K] -> (accept_len [B], stats [B][K][4] float64 (p_d, H, thr, rank), margins [B][K])."""
    logits, draft_ids = np.asarray(logits), np.asarray(draft_ids)
    B, K = draft_ids.shape
    acc = np.zeros(B, dtype=np.int64)
    stats = np.zeros((B, K, 4))
    margins = np.zeros((B, K))
    for b in range(B):
        run = True
        for i in range(K):
            keep, pd, H, thr, rank, mg = decide(logits[b, i], int(draft_ids[b, i]), rule, T, eps, delta, k)
            stats[b, i] = (pd, H, thr, rank)
            margins[b, i] = mg
            run = run and keep
            acc[b] += 1 if run else 0
    return acc, stats, margins


# --------------------------------------------------------------------------------------------------------- planted rows
def two_level(V, d, p_d, rng=None, masked=None):
    """A row whose softmax (T = 1) puts p_d on token d and spreads the rest evenly over the other unmasked tokens; `masked`
    (index array) entries are -inf. Exact in float64; the caller rounds to the dtype under test and re-derives the margin."""
    x = np.zeros(V)
    live = np.ones(V, dtype=bool)
    if masked is not None:
        live[masked] = False
    live[d] = True
    n_other = int(live.sum()) - 1
    x[:] = math.log((1.0 - p_d) / max(n_other, 1))
    x[d] = math.log(p_d)
    x[~live] = NEG
    return x


def planted_cases(V, K):
    """[(name, rule, params, logits [1][K+1][V] float64, draft_ids [1][K], expected accept_len)]: every planted case of the op test,
    one batch row each. Margins are checked by tests/test_typical_ref.py after rounding to bf16."""
    cases = []
    eps, delta = 0.09, 0.3
    par = {"T": 1.0, "eps": eps, "delta": delta}
    d0 = [(7 * i + 3) % V for i in range(K)]

    def block(rows):
        lg = np.zeros((1, K + 1, V))
        for i, r in enumerate(rows):
            lg[0, i] = r
        return lg

    # uniform rows: H = log V, p = 1/V; thr = min(eps, delta / V): p = 1/V >= 0.3/V -> kept (margin 1/0.3 - 1) when delta/V < eps
    cases.append(("uniform", "typical", par, block([np.zeros(V)] * K), [d0], K))
    # ... and rejected by the fixed threshold as soon as 1/V < eps
    if 1.0 / V < eps * 0.9:
        cases.append(("uniform/fixed", "typical", dict(par, delta=None), block([np.zeros(V)] * K), [d0], 0))
    # one dominant logit at T = 0.05 (z up to 400: the overflow guard): the dominant token is kept, any other rejected
    dom = np.zeros(V)
    dom[d0[0]] = 20.0
    cases.append(("dominant/kept", "typical", dict(par, T=0.05), block([dom] * K), [[d0[0]] * K], K))
    if V > 1:
        cases.append(("dominant/other", "typical", dict(par, T=0.05), block([dom] * K), [[(d0[0] + 1) % V] * K], 0))
    # half the vocabulary at -inf: the live half is uniform -> H = log(V/2): kept; d on a -inf entry: p_d = 0, rejected
    if V >= 4:
        half = np.zeros(V)
        half[1::2] = NEG
        even = [2 * ((3 * i + 1) % (V // 2)) for i in range(K)]
        cases.append(("half_masked/kept", "typical", par, block([half] * K), [even], K))
        cases.append(("half_masked/d_masked", "typical", par, block([half] * K), [[e + 1 if e + 1 < V else 1 for e in even]], 0))
        one = np.full(V, NEG)
        one[even[0]] = 1.5                    # all -inf but one: H = 0, p = 1
        cases.append(("one_live", "typical", par, block([one] * K), [[even[0]] * K], K))
    # the first failing position at every i, including none: rows keep d at p = 0.5 (thr <= 0.09); the failing row is all but uniform
    # (thr ~ delta / V) with p_d = 0.03 / V, a tenth of it
    for fail in range(K + 1):
        rows = [two_level(V, d0[i], 0.03 / V if i == fail else 0.5) for i in range(K)]
        if V >= 8:
            cases.append((f"first_fail/{fail}", "typical", par, block(rows), [d0], min(fail, K)))
    # exact ties around d for the rank rule: x_d shared by tokens below and above d; rank = (# strictly larger) + (# equal below d)
    if V >= 16:
        d = V // 2
        tie = np.full(V, -3.0)
        tie[[1, d - 1, d, d + 1, V - 1]] = 2.0            # two equal below d, two above
        tie[0] = 5.0                                     # one strictly larger
        for k, want in ((3, 0), (4, K)):                 # rank_d = 1 + 2 = 3: rejected at k = 3, kept at k = 4
            cases.append((f"ties/k{k}", "topk_agree", {"k": k}, block([tie] * K), [[d] * K], want))
        cases.append(("ties/lowest_index_wins", "topk_agree", {"k": 1}, block([np.zeros(V)] * K), [[0] * K], K))
        cases.append(("ties/second_index_loses", "topk_agree", {"k": 1}, block([np.zeros(V)] * K), [[1] * K], 0))
    return cases


def random_case(B, K, V, seed, scale=3.0, p_draft_top=0.6):
    """Seeded random logits (normal * scale, a few -inf) with draft ids that are the row's argmax with probability p_draft_top, else
    a random token among the 8 largest: accept lengths spread over 0..K."""
    rng = np.random.default_rng(seed)
    lg = rng.standard_normal((B, K + 1, V)) * scale
    lg[rng.random((B, K + 1, V)) < 0.01] = NEG
    ids = np.zeros((B, K), dtype=np.int32)
    for b in range(B):
        for i in range(K):
            order = np.argsort(-lg[b, i], kind="stable")
            ids[b, i] = order[0] if rng.random() < p_draft_top else order[rng.integers(0, min(8, V))]
    return lg, ids


# --------------------------------------------------------------------------------------------------- the device's error bound
U = 2.0 ** -24          # unit roundoff of fp32
U_FN = 2.0 ** -23       # expf / logf: 1 ulp


def chain_length(V, width):
    """Factors a term of S passes through on the device: the rescales of its thread (at most one per element the thread folds in
    after it: n - 1), the 6 wave merges, the 15 sequential wave-partial merges, and its own expf. width: elements per load of the
    row walker (8: aligned bf16 / f16... rows with V % 8 == 0; 4: aligned f32 rows with V % 4 == 0; 1: the scalar path)."""
    per = width * math.ceil(V / width / 1024)
    return per + 6 + 15 + 1, per


def bounds(V, width, logS, M1, M2, t_d, H):
    """(relative bound of S, relative bound of p_d, absolute bound of H, relative bound of thr) as DESIGN section 4 derives them."""
    L, per = chain_length(V, width)
    e_S = 2 * U * (M1 + 1) + L * (U_FN + U) + (per + 21) * U
    e_p = e_S + U_FN + 2 * U * abs(t_d) + 2 * U
    e_H = (e_S + U_FN * abs(logS) + U) + M1 * (2 * e_S + 3 * U) + 2 * U * M2 + U * (abs(H) + abs(logS) + M1)
    e_thr = e_H * 1.01 + U_FN + 2 * U
    return e_S, e_p, e_H, e_thr
