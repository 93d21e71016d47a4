"""The float64 restatement of the lossy acceptance rules (tests/typical_ref.py) on hand-worked rows, and the decision margins of the
cases the device tests run: every planted case sits >= 1e-2 from its threshold after rounding to bf16, and the seeded random set
leaves at most 2 % of its positions under 1e-4. Runs without a device."""

import math

import numpy as np
import pytest
import torch

import typical_ref as R

NEG = float("-inf")


def bf16(x):
    """float64 array -> the values bf16 stores, as float64"""
    return torch.from_numpy(np.asarray(x, dtype=np.float32)).to(torch.bfloat16).to(torch.float64).numpy()


def test_uniform_row():
    V = 64
    keep, pd, H, thr, rank, _ = R.decide(np.zeros(V), 5, "typical", eps=0.09, delta=0.3)
    assert pd == pytest.approx(1 / V, rel=1e-15) and H == pytest.approx(math.log(V), rel=1e-15)
    assert thr == pytest.approx(0.3 / V, rel=1e-14) and keep and rank == 5          # ties: the 5 lower indices rank first
    assert not R.decide(np.zeros(V), 5, "typical", eps=0.09, delta=None)[0]          # fixed threshold: 1/64 < 0.09


def test_one_hot_row():
    x = np.full(10, NEG)
    x[3] = 2.0
    keep, pd, H, thr, rank, _ = R.decide(x, 3, "typical", T=0.7)
    assert (keep, pd, H, rank) == (True, 1.0, 0.0, 0) and thr == 0.09
    keep, pd, H, thr, rank, _ = R.decide(x, 4, "typical", T=0.7)                     # d on a -inf entry
    assert (keep, pd, H) == (False, 0.0, 0.0) and rank == 4                           # the live token, and the three -inf below index 4


def test_two_point_row():
    # p = (0.8, 0.2) at T = 2 from logits (2 ln 4, 0): H = -(0.8 ln 0.8 + 0.2 ln 0.2)
    x = np.array([2 * math.log(4.0), 0.0])
    H_want = -(0.8 * math.log(0.8) + 0.2 * math.log(0.2))
    keep, pd, H, thr, _, margin = R.decide(x, 1, "typical", T=2.0, eps=0.25, delta=0.3)
    assert pd == pytest.approx(0.2, rel=1e-14) and H == pytest.approx(H_want, rel=1e-14)
    assert thr == pytest.approx(min(0.25, 0.3 * math.exp(-H_want)), rel=1e-14) and thr < 0.2 and keep
    assert margin == pytest.approx((0.2 - thr) / thr, rel=1e-12)
    assert not R.decide(x, 1, "typical", T=2.0, eps=0.25, delta=None)[0]             # 0.2 < 0.25


def test_minus_inf_elements_add_nothing():
    x = np.array([1.0, NEG, 0.0, NEG, -1.0])
    y = np.array([1.0, 0.0, -1.0])
    a, b = R.row_stats(x, 2, 0.5), R.row_stats(y, 1, 0.5)
    assert a[0] == b[0] and a[1] == b[1] and a[3] == b[3]
    assert math.isnan(R.row_stats(np.full(4, NEG), 0)[1]) and not R.decide(np.full(4, NEG), 0, "typical")[0]


def test_rank_ties_go_to_the_lower_index():
    x = np.array([0.0, 3.0, 1.0, 3.0, 1.0, 3.0])
    assert [R.row_stats(x, d)[2] for d in range(6)] == [5, 0, 3, 1, 4, 2]
    assert R.decide(x, 3, "topk_agree", k=1)[0] is False and R.decide(x, 3, "topk_agree", k=2)[0] is True
    assert R.row_stats(x, 6)[2] == 6 and R.row_stats(x, -1)[2] == 6                    # an id outside the vocabulary ranks last


def test_accept_len_is_the_leading_run():
    V, K = 32, 4
    rows = [R.two_level(V, 3, 0.5), R.two_level(V, 3, 0.03 / V), R.two_level(V, 3, 0.5), R.two_level(V, 3, 0.5), np.zeros(V)]
    acc, stats, _ = R.accept(np.stack(rows)[None], [[3] * K], "typical")
    assert acc.tolist() == [1] and stats.shape == (1, K, 4)


SHAPES = [(50, 4), (1000, 4), (8200, 8), (8195, 1), (128256, 4)]


@pytest.mark.parametrize("V,K", SHAPES)
def test_every_planted_case_has_margin(V, K):
    cases = R.planted_cases(V, K)
    names = {c[0].split("/")[0] for c in cases}
    assert {"uniform", "dominant", "half_masked", "one_live", "first_fail", "ties"} <= names
    assert sum(c[0].startswith("first_fail/") for c in cases) == K + 1
    for name, rule, par, lg, ids, want in cases:
        q = bf16(lg)
        acc, _, margins = R.accept(q, ids, rule, **par)
        assert acc.tolist() == [want], name
        acc32, _, m32 = R.accept(np.asarray(lg, dtype=np.float32).astype(np.float64), ids, rule, **par)
        assert acc32.tolist() == [want], name
        assert margins.min() >= 1e-2 and m32.min() >= 1e-2, (name, margins.min())


def test_the_random_set_leaves_few_positions_near_the_threshold():
    under = total = 0
    lens = []
    for seed, (B, K, V) in enumerate([(3, 8, 1000), (3, 4, 8200), (1, 8, 8195), (3, 4, 50)]):
        lg, ids = R.random_case(B, K, V, seed)
        acc, _, margins = R.accept(bf16(lg), ids, "typical", T=0.7, eps=0.09, delta=0.3)
        under += int((margins < 1e-4).sum())
        total += margins.size
        lens += acc.tolist()
    assert under <= 0.02 * total
    assert len(set(lens)) >= 3          # the set is not all-or-nothing


def test_bounds_grow_with_the_chain():
    L8, per8 = R.chain_length(128256, 8)
    L1, per1 = R.chain_length(8195, 1)
    assert (per8, L8) == (128, 150) and (per1, L1) == (9, 31)
    e_S, e_p, e_H, e_thr = R.bounds(128256, 8, math.log(128256), 1.0, 2.0, -5.0, math.log(128256))
    assert 0 < e_S < e_p < 1e-4 and 0 < e_H < 1e-3 and e_thr > e_H
