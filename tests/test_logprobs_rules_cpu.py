"""The host rules of a generate_batch step with the log-prob payload (SpeculativePipeline._rules_batch, info=): through every branch
that cuts, appends, strips or deletes tokens, the payload stays parallel to the generated tokens — each entry carries its own token
id, so `[e.token for e in row.token_info] == row.generated` says it — and without a payload the function does what it did before
the payload existed (`_rules_before`, the function as it stood, restated here)."""

import random
from collections import namedtuple

import pytest

import call_route_cases as C

E = namedtuple("E", "token pos")        # a payload entry that knows its token and the step position it came from
EOS, V, K = C.EOS, C.V_SMALL, 4


@pytest.fixture(scope="module")
def pipe():
    return C._stand_in()


def _row(seq, gen=()):
    from src.specdec.core.pipeline import _Row

    r = _Row(list(seq) + list(gen))
    r.n_prompt = len(seq)
    r.generated = list(gen)
    r.token_info = [E(g, -1) for g in gen]
    return r


def _rules_before(row, k, a, t, max_tokens, eos, resample=None, dedup=True):
    """_rules_batch as it stood before the payload (same statements, no payload)"""
    clamp = lambda x: min(max(int(x), 0), V - 1)      # noqa: E731
    gen = row.generated
    if a > 0:
        acc = [clamp(x) for x in t[:a]]
        if eos is not None and eos in acc:
            acc = acc[: acc.index(eos)]
            row.active = False
        pos = a if a < k else len(acc)
        bonus = clamp(t[pos] if (resample is None or pos == a) else resample(pos))
        if eos is not None and bonus == eos:
            row.active = False
        acc.append(bonus)
        if gen and dedup:
            for c in range(min(5, len(gen), len(acc)), 0, -1):
                if gen[-c:] == acc[:c]:
                    acc = acc[c:]
                    break
        gen.extend(acc)
        emitted = acc
    else:
        emitted = [clamp(t[0])]
        if eos is not None and emitted[0] == eos:
            row.active = False
            emitted = []
        if dedup and emitted and gen and gen[-1] == emitted[0]:
            emitted = []
        gen.extend(emitted)
    row.proposed += k
    row.accepted += len(emitted)
    if emitted:
        acc, cur = list(emitted), row.seq
        c = min(5, len(cur), len(acc)) if dedup else 0
        if c > 0 and cur[-c:] == acc[:c]:
            if len(acc) > c:
                acc = acc[c:]
                if len(gen) >= c:
                    del gen[-c:]
            else:
                acc = []
        row.seq = cur + acc
    if len(gen) >= max_tokens:
        row.active = False


def _state(r):
    return (list(r.generated), list(r.seq), r.active, r.proposed, r.accepted)


def _both(pipe, seq, gen, k, a, t, eos=EOS, max_tokens=64, resample=None, dedup=True):
    """the step with a payload, without one, and by the function as it stood: the three rows"""
    info = [E(x, i) for i, x in enumerate(t)]
    with_info, without, before = _row(seq, gen), _row(seq, gen), _row(seq, gen)
    pipe._rules_batch(with_info, k, a, t, max_tokens, eos, resample, dedup=dedup, info=info,
                      resample_info=(lambda pos, tok: E(tok, 100 + pos)) if resample else None)
    pipe._rules_batch(without, k, a, t, max_tokens, eos, resample, dedup=dedup)
    _rules_before(before, k, a, t, max_tokens, eos, resample, dedup)
    assert _state(with_info) == _state(without) == _state(before)
    assert [e.token for e in with_info.token_info] == with_info.generated
    assert len(without.token_info) == len(gen)                       # no payload: nothing is appended
    return with_info


def test_plain_step(pipe):
    r = _both(pipe, [50, 51], [60], K, 2, [5, 6, 7, 8, 9])
    assert r.generated == [60, 5, 6, 7] and [e.pos for e in r.token_info] == [-1, 0, 1, 2]


def test_accepted_eos_cut(pipe):
    r = _both(pipe, [50, 51], [60], K, 3, [5, EOS, 7, 8, 9])         # a < k: cut before the EOS, then t[a]
    assert r.generated == [60, 5, 8] and not r.active
    assert [e.pos for e in r.token_info] == [-1, 0, 3]


def test_accepted_eos_cut_at_full_acceptance(pipe):
    r = _both(pipe, [50, 51], [60], K, K, [5, 6, EOS, 8, 9])         # a == k: the token after the cut is the EOS itself, at its own row
    assert r.generated == [60, 5, 6, EOS] and not r.active
    assert [e.pos for e in r.token_info] == [-1, 0, 1, 2]


def test_accepted_eos_cut_with_a_host_redraw(pipe):
    r = _both(pipe, [50, 51], [60], K, K, [5, 6, EOS, 8, 9], resample=lambda pos: 70 + pos)   # sampled bonus: redrawn at row 2
    assert r.generated == [60, 5, 6, 72] and not r.active
    assert [e.pos for e in r.token_info] == [-1, 0, 1, 102]          # the redraw's own payload, for the redrawn token


def test_bonus_eos(pipe):
    r = _both(pipe, [50, 51], [60], K, 1, [5, EOS, 7, 8, 9])
    assert r.generated == [60, 5, EOS] and not r.active
    assert [e.pos for e in r.token_info] == [-1, 0, 1]


def test_front_overlap_strip(pipe):
    r = _both(pipe, [50, 51], [21, 22, 23], K, 2, [22, 23, 24, 8, 9])      # the step starts with the generated tail (22, 23)
    assert r.generated == [21, 22, 23, 24] and r.active
    assert [e.pos for e in r.token_info] == [-1, -1, -1, 2]


def test_delete_from_the_generated_tail(pipe):
    # a one-token sequence whose token the step repeats: the sequence rule strips it and deletes the LAST generated token
    r = _both(pipe, [7], [], K, 1, [7, 8, 9, 9, 9])
    assert r.generated == [7] and r.seq == [7, 8]
    assert [e.pos for e in r.token_info] == [0]
    # and with five tokens of overlap at K = 8
    t = [11, 12, 13, 14, 15, 16, 17, 18, 19]
    r = _both(pipe, [11, 12, 13, 14, 15], [], 8, 6, t)
    assert r.generated == [11, 12] and r.seq == [11, 12, 13, 14, 15, 16, 17]
    assert [e.pos for e in r.token_info] == [0, 1]


def test_zero_accept_branches(pipe):
    r = _both(pipe, [50, 51], [60], K, 0, [5, 6, 7, 8, 9])
    assert r.generated == [60, 5] and [e.pos for e in r.token_info] == [-1, 0]
    r = _both(pipe, [50, 51], [60], K, 0, [60, 6, 7, 8, 9])          # the duplicate drop
    assert r.generated == [60] and [e.pos for e in r.token_info] == [-1]
    r = _both(pipe, [50, 51], [60], K, 0, [EOS, 6, 7, 8, 9])         # EOS: dropped, row stops
    assert r.generated == [60] and not r.active


def test_dedup_off_keeps_everything(pipe):
    r = _both(pipe, [50, 51], [21, 22, 23], K, 2, [22, 23, 24, 8, 9], dedup=False)
    assert r.generated == [21, 22, 23, 22, 23, 24]
    assert [e.pos for e in r.token_info] == [-1, -1, -1, 0, 1, 2]
    r = _both(pipe, [50, 51], [60], K, 0, [60, 6, 7, 8, 9], dedup=False)
    assert r.generated == [60, 60]


def test_budget_stops_the_row(pipe):
    r = _both(pipe, [50, 51], [60], K, 2, [5, 6, 7, 8, 9], max_tokens=3)
    assert not r.active and len(r.token_info) == len(r.generated) == 4


def test_random_steps_keep_the_payload_parallel(pipe):
    """many steps per row over a tiny alphabet (overlaps, duplicates and EOS all happen), every branch combination"""
    rng = random.Random(5)
    seen = set()
    for trial in range(300):
        dedup, eos = rng.random() < 0.7, (EOS if rng.random() < 0.8 else None)
        k = rng.choice([1, 2, 4, 8])
        resample = (lambda pos: rng.randrange(2, 6)) if rng.random() < 0.3 else None
        seq = [rng.randrange(2, 6) for _ in range(rng.randrange(1, 4))]
        a_row, b_row = _row(seq), _row(seq)
        for _ in range(6):
            if not a_row.active:
                break
            a = rng.randrange(0, k + 1)
            t = [rng.randrange(2, 6) for _ in range(k + 1)]
            info = [E(x, i) for i, x in enumerate(t)]
            state = rng.getstate()
            pipe._rules_batch(a_row, k, a, t, 40, eos, resample, dedup=dedup, info=info, resample_info=lambda pos, tok: E(tok, 100 + pos))
            rng.setstate(state)                                       # the same redraws for the reference run
            _rules_before(b_row, k, a, t, 40, eos, resample, dedup)
            assert _state(a_row) == _state(b_row)
            assert [e.token for e in a_row.token_info] == a_row.generated
            seen.add((a == 0, a == k, dedup, eos is None, resample is None))
    assert len(seen) >= 20
