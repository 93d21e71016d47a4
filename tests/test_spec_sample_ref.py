"""The CPU restatement of speculative sampling (tests/spec_sample_ref.py): it is the acceptance rule of
oracle.hostlogic_ref.rejection_accept, it preserves the target's distribution, and its draw schedule has the stated
properties. The GPU tests (tests/test_hip_spec_sample_gpu.py) compare the device against this restatement."""

import numpy as np
import pytest
import torch
from scipy import stats

import spec_sample_ref as R
from oracle import sampling_ref as S
from oracle.hostlogic_ref import rejection_accept


def _bf16(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).float().numpy()


def _softmax(v):
    e = np.exp(v - v.max())
    return e / e.sum()


@pytest.mark.parametrize("T", [0.5, 0.75, 1.0, 1.5])
def test_accept_length_and_next_distribution_equal_rejection_accept(T):
    V, K = 12, 3
    rng = np.random.default_rng(int(T * 100))
    seen = set()
    for seed in range(150):
        p = _bf16(rng.normal(0, 2.0, (K + 1, V)))
        kind = seed % 3
        q = p[:K].copy() if kind == 0 else _bf16(p[:K] + rng.normal(0, [0.0, 0.5, 3.0][kind], (K, V)))
        c, sid = 7 * seed, seed % 5
        d = [R.draft_draw_ref(q[i], T, seed, c, i, sid) for i in range(K)]
        u = [S.draw_uniform(seed, c + i, sid) for i in range(K)]
        a, nxt = rejection_accept(d, q, p, u, T)
        res = R.spec_accept_ref(q, p, d, T, seed, c, sid)
        assert res.accept_len == a, (seed, res.ratios, u)
        seen.add(a)
        w = R.next_weights(p[a], q[a], T) if a < K else np.exp(R.scaled(p[K], T) - R.lse(R.scaled(p[K], T)))
        np.testing.assert_allclose(w / w.sum(), nxt, rtol=1e-12, atol=1e-300)
        # the token actually drawn lies in the support of that distribution
        assert nxt[res.next_tok] > 0
        if kind == 0:   # q bitwise equal to p: ratio exactly 1, everything accepted, the bonus is a draw from p_K
            assert (res.ratios == 1.0).all() and a == K
            assert res.next_tok == S.gumbel_argmax_ref(p[K], T, seed, c + K, sid)
    assert seen == set(range(K + 1))


def _first_token_counts(p, q, T, seed, n_steps):
    K, V = q.shape
    counts = np.zeros(V, dtype=np.int64)
    c = 0
    for _ in range(n_steps):
        d, res, emitted, c2 = R.spec_step_ref(q, p, T, seed, c, 3)
        assert c2 == c + K + 1 and len(emitted) == res.accept_len + 1
        counts[emitted[0]] += 1
        c = c2
    return counts


CASES = ["q_equals_p", "q_one_hot", "p_with_zeros", "q_far", "q_near"]


@pytest.mark.parametrize("case", CASES)
def test_first_emitted_token_is_distributed_as_the_target(case):
    """Distribution preservation: over N = 6000 seeded steps (K = 3, V = 12, T = 0.75, counters running as on the device) the
    law of the FIRST emitted token is softmax(p_0 / T), whatever q is. Pearson chi-square over the tokens of non-zero target
    probability (tokens of probability zero must never appear); the level, fixed before the first run: p-value > 1e-4.
    Observed (statistic / degrees of freedom / p-value) with the committed seeds:
      q_equals_p 6.73 / 11 / 0.821, q_one_hot 5.18 / 11 / 0.922, p_with_zeros 14.65 / 7 / 0.041, q_far 14.25 / 11 / 0.220,
      q_near 8.59 / 11 / 0.660."""
    V, K, T, N = 12, 3, 0.75, 6000
    rng = np.random.default_rng(CASES.index(case) + 11)
    p = _bf16(rng.normal(0, 1.5, (K + 1, V)))
    if case == "q_equals_p":
        q = p[:K].copy()
    elif case == "q_one_hot":
        q = _bf16(rng.normal(0, 1.0, (K, V)))
        q[:, 4] += 20.0
        q = _bf16(q)
    elif case == "p_with_zeros":
        p[:, [1, 5]] = -np.inf            # probability exactly 0
        p[:, [8, 9]] = -1000.0            # bf16-representable; exp underflows to 0 in float64
        q = _bf16(rng.normal(0, 1.5, (K, V)))
    elif case == "q_far":
        q = _bf16(rng.normal(0, 3.0, (K, V)))
    else:
        q = _bf16(p[:K] + rng.normal(0, 0.3, (K, V)))
    counts = _first_token_counts(p, q, T, 20261016 + CASES.index(case), N)
    want = _softmax(R.scaled(p[0], T))
    support = want > 0
    assert counts[~support].sum() == 0
    chi2, pval = stats.chisquare(counts[support], want[support] / want[support].sum() * N)
    print(f"{case}: chi2 = {chi2:.2f}, df = {int(support.sum()) - 1}, p = {pval:.3f}")
    assert pval > 1e-4, (case, chi2, pval)


def test_draw_schedule_properties():
    V, K, T = 64, 3, 0.75
    rng = np.random.default_rng(5)
    p, q = _bf16(rng.normal(0, 2, (K + 1, V))), _bf16(rng.normal(0, 2, (K, V)))
    base = (1234, 10, 2)   # seed, counter, stream
    g0 = R.gumbel_noise(V, *base)
    for other in ((1235, 10, 2), (1234, 11, 2), (1234, 10, 3), (1234 + (1 << 32), 10, 2)):
        assert not np.array_equal(g0, R.gumbel_noise(V, *other))
        assert S.draw_uniform(*base) != S.draw_uniform(*other)
    # the three kinds of draws of a step use distinct Philox inputs: (counter, tag) pairs never coincide
    c = 10
    kinds = [(c + i, S.TAG_GUMBEL) for i in range(K)] + [(c + i, S.TAG_CDF) for i in range(K)] + [(c + K, S.TAG_GUMBEL)]
    assert len(set(kinds)) == 2 * K + 1
    # ... and the next step starts past them
    d, res, emitted, c2 = R.spec_step_ref(q, p, T, 1234, c, 2)
    assert c2 == c + K + 1 and min(c2 + i for i in range(K + 1)) > max(k[0] for k in kinds)
    # the draft tokens are sample_token's whole-row draw of the stored q rows
    assert d == [S.sample_token_ref(q[i], T, None, None, 1234, c + i, 2) for i in range(K)]
    assert emitted == d[: res.accept_len] + [res.next_tok]
    # other seed / stream / counter: other outcome somewhere over a few steps
    def run(seed, c, sid):
        out = []
        for _ in range(6):
            _, _, e, c = R.spec_step_ref(q, p, T, seed, c, sid)
            out.append(e)
        return out
    assert run(1234, 0, 2) == run(1234, 0, 2)
    assert len({str(run(*x)) for x in ((1234, 0, 2), (1, 0, 2), (1234, 0, 4), (1234, 1, 2))}) == 4
    # inactive rows consume nothing
    assert R.spec_step_ref(q, p, T, 1234, 17, 2, active=False) == ([], None, [], 17)


def test_non_finite_rows_reject_and_redraw_from_p():
    V, K, T = 32, 2, 1.5
    rng = np.random.default_rng(9)
    p, q = _bf16(rng.normal(0, 2, (K + 1, V))), _bf16(rng.normal(0, 2, (K, V)))
    d = [3, 4]
    for what in ("nan_p", "nan_q", "inf_q", "all_ninf_p"):
        pp, qq = p.copy(), q.copy()
        if what == "nan_p":
            pp[0, 7] = np.nan
        elif what == "nan_q":
            qq[0, 9] = np.nan
        elif what == "inf_q":
            qq[0, 2] = np.inf
        else:
            pp[0, :] = -np.inf
        res = R.spec_accept_ref(qq, pp, d, T, 5, 0, 0)
        assert res.accept_len == 0 and np.isnan(res.ratios[0]) and not np.isnan(res.ratios[1])
        want = 7 if what == "nan_p" else S.gumbel_argmax_ref(pp[0], T, 5, K, 0)
        assert res.next_tok == want, what
    # -inf entries of finite rows: probability zero on that side, no special case
    pp = p.copy()
    pp[0, 3] = -np.inf
    res = R.spec_accept_ref(q, pp, d, T, 5, 0, 0)
    assert res.ratios[0] == 0.0 and res.accept_len == 0 and res.next_tok != 3
