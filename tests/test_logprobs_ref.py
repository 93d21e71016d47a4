"""tests/logprobs_ref.py pinned on rows whose answers are computed by hand, and the C entry's refusals that need no device."""

import ctypes
import math

import numpy as np

import logprobs_ref as R

NEG = float("-inf")


def test_uniform_row():
    V, N = 37, 5
    lp, rank, ids, lps, _ = R.row_logprobs(np.full(V, 1.25), 6, N)
    assert lp == -math.log(V)
    assert rank == 6                                  # the six lower indices win the tie
    assert ids.tolist() == list(range(N))
    assert lps.tolist() == [-math.log(V)] * N


def test_one_finite_element_is_exactly_zero():
    x = np.full(9, NEG)
    x[4] = -3.5
    lp, rank, ids, lps, _ = R.row_logprobs(x, 4, 3)
    assert lp == 0.0 and rank == 0
    assert ids.tolist() == [4, 0, 1]                  # then the -inf entries in index order
    assert lps.tolist() == [0.0, NEG, NEG]


def test_tie_at_place_n_goes_to_the_lower_index():
    x = np.array([0.0, 2.0, 1.0, 3.0, 1.0, 1.0, -1.0])
    _, _, ids, lps, _ = R.row_logprobs(x, 0, 3)
    assert ids.tolist() == [3, 1, 2]                  # 1.0 is shared by 2, 4, 5: place 3 goes to index 2
    assert lps[0] > lps[1] > lps[2]
    _, rank, _, _, _ = R.row_logprobs(x, 4, 0)
    assert rank == 3                                  # 3.0, 2.0 and the equal entry at the lower index 2
    _, rank, _, _, _ = R.row_logprobs(x, 5, 0)
    assert rank == 4


def test_two_element_row_by_hand():
    lp, rank, ids, lps, _ = R.row_logprobs(np.array([0.0, math.log(3.0)]), 0, 2)
    assert abs(lp - math.log(0.25)) < 1e-15 and rank == 1
    assert ids.tolist() == [1, 0]
    assert abs(lps[0] - math.log(0.75)) < 1e-15 and abs(lps[1] - math.log(0.25)) < 1e-15


def test_token_at_minus_inf():
    x = np.array([1.0, NEG, 2.0, NEG])
    lp, rank, ids, lps, _ = R.row_logprobs(x, 3, 4)
    assert lp == NEG
    assert rank == 3                                  # two finite entries and the -inf at the lower index 1
    assert ids.tolist() == [2, 0, 1, 3]
    assert lps[2] == NEG and lps[3] == NEG and math.isfinite(lps[1])


def test_all_minus_inf():
    lp, rank, ids, lps, mom = R.row_logprobs(np.full(5, NEG), 2, 3)
    assert math.isnan(lp) and rank == -1 and mom is None
    assert ids.tolist() == [-1, -1, -1] and np.isnan(lps).all()
    assert R.none_record((lp, rank, ids, lps))


def test_top_n_clamps_to_v():
    _, _, ids, lps, _ = R.row_logprobs(np.array([0.5, 1.5, -0.5]), 0, 20)
    assert ids.tolist() == [1, 0, 2] and len(lps) == 3
    assert abs(np.exp(lps).sum() - 1.0) < 1e-14


def test_bound_is_small_and_grows_with_the_chain():
    a = R.bounds(1000, 8, 3.0, 2.0, -5.0)
    b = R.bounds(128256, 8, 3.0, 2.0, -5.0)
    c = R.bounds(128256, 1, 3.0, 2.0, -5.0)
    assert 0 < a < min(b, c) and max(b, c) < 1e-4     # (8-wide loads round a thread's share up: 128 elements against 126)


def test_check_row_rejects_a_wrong_rank_and_a_far_value():
    x = np.array([0.0, 1.0, 2.0, 3.0])
    lp, rank, ids, lps, _ = R.row_logprobs(x, 1, 2)
    assert R.check_row(x, 1, 2, 1, (np.float32(lp), rank, ids, lps.astype(np.float32))) <= 1.0
    for bad in ((lp, rank + 1, ids, lps), (lp + 1e-3, rank, ids, lps), (lp, rank, ids[::-1], lps)):
        try:
            R.check_row(x, 1, 2, 1, bad)
        except AssertionError:
            continue
        raise AssertionError("check_row accepted a wrong record")


def test_entry_refusals_without_a_device():
    """sd_token_logprobs refuses before any device work: the symbols load, the ABI version stays 1."""
    from specdec_hip import _abi

    lib = _abi.load()
    assert lib.sd_abi_version() == 1
    for name in ("sd_token_logprobs", "sd_specdec_set_logprobs", "sd_specdec_logprobs", "sd_specdec_logprob_words"):
        assert hasattr(lib, name)
    p = ctypes.c_void_p(256)   # never dereferenced: every call below is refused first

    def call(logits=p, dtype=_abi.SD_BF16, stride=64, R_=1, V=64, ids=p, top_n=5, lp=p, rank=p, tid=p, tlp=p):
        return lib.sd_token_logprobs(logits, dtype, stride, R_, V, ids, top_n, lp, rank, tid, tlp, None)

    for kw, word in (({"logits": None}, "NULL"), ({"ids": None}, "NULL"), ({"lp": None}, "NULL"), ({"rank": None}, "NULL"),
                     ({"tid": None}, "NULL"), ({"tlp": None}, "NULL"), ({"V": 0}, "V="), ({"R_": 0}, "R="), ({"top_n": -1}, "top_n"),
                     ({"top_n": 21}, "top_n"), ({"dtype": _abi.SD_I32}, "dtype"), ({"stride": 63}, "row_stride"),
                     ({"lp": ctypes.c_void_p(258)}, "misaligned")):
        assert call(**kw) != 0, kw
        assert word in _abi.last_error(), (kw, _abi.last_error())
    assert lib.sd_specdec_set_logprobs(None, 1, 5, None, 0) != 0 and "NULL" in _abi.last_error()
    assert lib.sd_specdec_logprob_words(None) == 0
    assert not lib.sd_specdec_logprobs(None)
