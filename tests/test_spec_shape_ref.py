"""The restatement of top-k / top-p shaped speculative sampling (tests/spec_shape_ref.py): the exact law of the emitted token
by enumeration, a chi-square over its actual draws, the draw schedule, non-finite rows — and the library's two new entry
points (exports, binding table, argument validation), which needs no GPU."""

import ctypes

import numpy as np
import pytest
import torch
from scipy import stats

import spec_shape_ref as R
from oracle import sampling_ref as S


def _bf16(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _law(k: R.Kept, V: int) -> np.ndarray:
    out = np.zeros(V)
    out[k.ids] = k.e / k.z
    return out


def _q_row(kind: str, p_row, kp: R.Kept, rng):
    """q whose kept set is equal to / disjoint from / nested in / overlapping p's (when top_k allows it)."""
    V = p_row.shape[0]
    if kind == "equal":
        return p_row.copy()
    if kind == "disjoint":
        return _bf16(-p_row)
    if kind == "nested":       # the first half of p's kept ids raised by 6: the same sorted order, more mass on top, an earlier cut
        q = p_row.copy()
        q[kp.ids[: max(1, len(kp.ids) // 2)]] += 6.0
        return _bf16(q)
    if kind == "overlap":
        return _bf16(p_row + rng.normal(0, 1.5, V))
    return _bf16(rng.normal(0, 2.0, V))     # unrelated


SHAPES = [(5, 1.0, 0.7), (8, 0.9, 1.0), (1, 1.0, 1.0), (40, 0.5, 1.3), (12, 0.2, 0.7), (3, 0.9, 2.0)]


@pytest.mark.parametrize("kind", ["equal", "disjoint", "nested", "overlap", "unrelated"])
def test_emitted_law_is_the_shaped_target_by_enumeration(kind):
    """K = 1, no statistics: sum_d q'(d) [ min(1, p'(d)/q'(d)) 1{x = d} + (1 - min(..)) r(x)/Z_r ] from the restatement's own
    weights equals p'(x) to 1e-12 for every x (Z_r == 0: the fallback is p' itself)."""
    rng = np.random.default_rng(["equal", "disjoint", "nested", "overlap", "unrelated"].index(kind) + 40)
    worst = 0.0
    for V in (12, 17, 29, 40):
        for top_k, top_p, T in SHAPES:
            p_row = _bf16(rng.normal(0, 2.0, V))
            kp = R.kept_set(p_row, T, top_k, top_p)
            kq = R.kept_set(_q_row(kind, p_row, kp, rng), T, top_k, top_p)
            if kind == "disjoint" and min(top_k, V) * 2 <= V:
                assert not set(kp.ids.tolist()) & set(kq.ids.tolist())
            if kind == "nested":
                assert set(kq.ids.tolist()) <= set(kp.ids.tolist())
            r = R.residual_weights(kp, kq)
            zr = R.seq_sum(r)
            nxt = np.zeros(V)
            nxt[kp.ids] = r / zr if zr > 0 else kp.e / kp.z
            law = np.zeros(V)
            for j, d in enumerate(kq.ids.tolist()):
                qd = float(kq.e[j]) / kq.z
                acc = min(1.0, R.ratio_of(kp, kq, d))
                law[d] += qd * acc
                law += qd * (1.0 - acc) * nxt
            want = _law(kp, V)
            worst = max(worst, float(np.abs(law - want).max()))
            np.testing.assert_allclose(law, want, rtol=0, atol=1e-12, err_msg=str((kind, V, top_k, top_p, T)))
    print(f"{kind}: max |law - p'| = {worst:.2e}")


def _first_token_counts(p, q, T, top_k, top_p, seed, n_steps):
    K, V = q.shape
    counts = np.zeros(V, dtype=np.int64)
    c = 0
    for _ in range(n_steps):
        d, res, emitted, c2, _ = R.spec_step_ref(q, p, T, top_k, top_p, seed, c, 3)
        assert c2 == c + K + 1 and len(emitted) == res.accept_len + 1
        counts[emitted[0]] += 1
        c = c2
    return counts


CASES = ["q_equals_p", "q_disjoint", "q_far", "q_near"]


@pytest.mark.parametrize("case", CASES)
def test_first_emitted_token_is_distributed_as_the_shaped_target(case):
    """Over N = 6000 seeded steps (K = 3, V = 16, T = 0.75, top_k 8, top_p 0.9, counters running as on the device) the law of
    the FIRST emitted token is S(p_0), whatever q is. Pearson chi-square over the kept tokens (tokens outside the kept set must
    never appear); the level, fixed before the first run: p-value > 1e-4."""
    V, K, T, N, top_k, top_p = 16, 3, 0.75, 6000, 8, 0.9
    rng = np.random.default_rng(CASES.index(case) + 21)
    p = _bf16(rng.normal(0, 1.5, (K + 1, V)))
    if case == "q_equals_p":
        q = p[:K].copy()
    elif case == "q_disjoint":
        q = _bf16(-p[:K])
    elif case == "q_far":
        q = _bf16(rng.normal(0, 3.0, (K, V)))
    else:
        q = _bf16(p[:K] + rng.normal(0, 0.3, (K, V)))
    counts = _first_token_counts(p, q, T, top_k, top_p, 20261016 + CASES.index(case), N)
    want = _law(R.kept_set(p[0], T, top_k, top_p), V)
    support = want > 0
    assert counts[~support].sum() == 0
    chi2, pval = stats.chisquare(counts[support], want[support] * N)
    print(f"{case}: chi2 = {chi2:.2f}, df = {int(support.sum()) - 1}, p = {pval:.3f}")
    assert pval > 1e-4, (case, chi2, pval)


def test_draw_schedule():
    V, K, T, top_k, top_p = 64, 3, 0.75, 10, 0.9
    rng = np.random.default_rng(5)
    p, q = _bf16(rng.normal(0, 2, (K + 1, V))), _bf16(rng.normal(0, 2, (K, V)))
    seed, c, sid = 1234, 10, 2
    # no two uniforms of a step share a counter block: (counter, tag) pairs never coincide, and the values differ
    kinds = [(c + i, S.TAG_CDF) for i in range(K)] + [(c + i, R.TAG_ACCEPT) for i in range(K)] + [(c + K, S.TAG_CDF)]
    assert len(set(kinds)) == 2 * K + 1 and R.TAG_ACCEPT not in (S.TAG_CDF, S.TAG_GUMBEL)
    us = [S.draw_uniform(seed, c + i, sid) for i in range(K + 1)] + [R.accept_uniform(seed, c + i, sid) for i in range(K)]
    assert len(set(us)) == 2 * K + 1
    for other in ((1235, 10, 2), (1234, 11, 2), (1234, 10, 3), (1234 + (1 << 32), 10, 2)):
        assert R.accept_uniform(seed, c, sid) != R.accept_uniform(*other)
    # d_{i+1} is the token sd_sample_token draws from q_i with draw index c + i
    d, res, emitted, c2, _ = R.spec_step_ref(q, p, T, top_k, top_p, seed, c, sid)
    assert d == [S.sample_token_ref(q[i], T, top_k, top_p, seed, c + i, sid) for i in range(K)]
    assert c2 == c + K + 1 and emitted == d[: res.accept_len] + [res.next_tok]
    # q bitwise equal to p: every ratio exactly 1.0, everything accepted, the bonus is the target's own draw with index c + K
    d, res, emitted, _, _ = R.spec_step_ref(p[:K], p, T, top_k, top_p, seed, c, sid)
    assert (res.ratios == 1.0).all() and res.accept_len == K
    assert res.next_tok == S.sample_token_ref(p[K], T, top_k, top_p, seed, c + K, sid)
    assert all(pos.zr == 0.0 for pos in res.positions)
    # ... and the candidate of every position is then the target's own draw at that position
    assert [pos.cand for pos in res.positions] == [S.sample_token_ref(p[i], T, top_k, top_p, seed, c + K, sid) for i in range(K + 1)]
    # a token outside the target's kept set: ratio 0, rejected; outside the draft's: NaN, rejected
    kp, kq = R.kept_set(p[0], T, top_k, top_p), R.kept_set(q[0], T, top_k, top_p)
    only_q = [t for t in kq.ids.tolist() if t not in kp.index]
    if only_q:
        assert R.ratio_of(kp, kq, only_q[0]) == 0.0
    outside = [t for t in range(V) if t not in kq.index][0]
    res = R.spec_accept_ref(q, p, [outside] + d[1:], T, top_k, top_p, seed, c, sid)
    assert np.isnan(res.ratios[0]) and res.accept_len == 0
    # inactive rows consume nothing
    assert R.spec_step_ref(q, p, T, top_k, top_p, seed, c, sid, active=False) == ([], None, [], c, float("inf"))
    # top_k = 1: the greedy step (draft argmax proposals, accepted iff equal to the target's argmax, next = target argmax)
    d, res, emitted, _, _ = R.spec_step_ref(q, p, T, 1, None, seed, c, sid)
    assert d == [int(np.argmax(q[i])) for i in range(K)]
    a = 0
    while a < K and d[a] == int(np.argmax(p[a])):
        a += 1
    assert res.accept_len == a and res.next_tok == int(np.argmax(p[a]))


def test_non_finite_rows_follow_the_point_mass_rule():
    V, K, T, top_k, top_p = 32, 2, 0.9, 6, 0.8
    rng = np.random.default_rng(9)
    p, q = _bf16(rng.normal(0, 2, (K + 1, V))), _bf16(rng.normal(0, 2, (K, V)))
    for bad in (np.nan, np.inf):
        p2 = p.copy()
        p2[0, 7] = bad                  # on top of the target row: the point mass on id 7
        k = R.kept_set(p2[0], T, top_k, top_p)
        assert k.ids.tolist() == [7] and k.e.tolist() == [1.0] and k.z == 1.0
        res = R.spec_accept_ref(q, p2, [7, 3], T, top_k, top_p, 1, 0, 0)
        assert res.positions[0].cand == 7
        if 7 in R.kept_set(q[0], T, top_k, top_p).index:
            assert res.ratios[0] >= 1.0
        res = R.spec_accept_ref(q, p2, [int(np.argmax(q[0])), 3], T, top_k, top_p, 1, 0, 0)
        if int(np.argmax(q[0])) != 7:
            assert res.ratios[0] == 0.0 and res.accept_len == 0 and res.next_tok == 7
    q2 = q.copy()
    q2[1, :] = -np.inf                  # all -inf: the point mass on id 0
    k = R.kept_set(q2[1], T, top_k, top_p)
    assert k.ids.tolist() == [0] and k.z == 1.0
    d, res, _, _, _ = R.spec_step_ref(q2, p, T, top_k, top_p, 3, 0, 0)
    assert d[1] == 0 and not np.isnan(res.ratios).any()
    p3 = p.copy()
    p3[1, 4] = -np.inf                  # a -inf entry of a finite row: weight 0, no special case
    assert 4 not in R.kept_set(p3[1], T, top_k, top_p).index or R.kept_set(p3[1], T, top_k, top_p).weight(4) == 0.0


def test_new_entry_points_are_exported_bound_and_validate_without_gpu():
    """sd_specdec_set_spec_shaping and sd_spec_sample_accept_shaped: exported, in the binding table, and their argument
    validation answers through the return code + sd_last_error before any device work."""
    from specdec_hip import _abi

    lib = _abi.load()
    for name in ("sd_specdec_set_spec_shaping", "sd_spec_sample_accept_shaped"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    rc = lib.sd_specdec_set_spec_shaping(None, 2000, 1.0)
    assert rc != 0 and "top_k=2000" in _abi.last_error()
    rc = lib.sd_specdec_set_spec_shaping(None, 0, 0.9)
    assert rc != 0 and "without top_k" in _abi.last_error()
    for bad in (0.0, -0.5, float("nan")):
        rc = lib.sd_specdec_set_spec_shaping(None, 50, bad)
        assert rc != 0 and "top_p" in _abi.last_error()
    rc = lib.sd_specdec_set_spec_shaping(None, 50, 0.9)
    assert rc != 0 and "NULL" in _abi.last_error()
    one = ctypes.c_void_p(8)
    args = lambda top_k, top_p, buf: (buf, buf, buf, 1, 1, 10, 1.0, top_k, top_p, 0, None, 0, None, None, buf, buf, None, buf, 64, None)  # noqa: E731
    rc = lib.sd_spec_sample_accept_shaped(*args(2000, 1.0, one))
    assert rc != 0 and "top_k=2000" in _abi.last_error()
    rc = lib.sd_spec_sample_accept_shaped(*args(0, 0.9, one))
    assert rc != 0 and "without top_k" in _abi.last_error()
    rc = lib.sd_spec_sample_accept_shaped(*args(50, 0.9, None))
    assert rc != 0 and "NULL" in _abi.last_error()
