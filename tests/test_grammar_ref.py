"""The token-automaton compiler (specdec_hip/grammar.py) on the CPU: from_regex against Python's re.fullmatch over a small
multi-byte vocabulary, the check() invariant, union, from_choices, and the refused inputs. The restatement the GPU tests compare
against (tests/grammar_ref.py) is checked against the compiler's own walk on the way. Last, the host rules of a row under a
grammar (no overlap / de-duplication)."""

import itertools
import re

import numpy as np
import pytest

import grammar_ref as G
from specdec_hip.grammar import DEAD, NONE, TokenFSM, from_tokenizer

ALPHABET = 'ab01-"'
PATTERNS = ["(ab|a)*b", "-?[01]{1,3}", '"[ab]*"', "a{2,}", r"(\d\d|-)+", '[^"]a.?']


def _vocab():
    """the six single bytes, 54 random tokens of 2..4 bytes over the alphabet, eos last"""
    rng = np.random.default_rng(5)
    toks = [c.encode() for c in ALPHABET]
    seen = set(toks)
    while len(toks) < 60:
        t = "".join(rng.choice(list(ALPHABET), size=int(rng.integers(2, 5)))).encode()
        if t not in seen:
            seen.add(t)
            toks.append(t)
    return toks + [None], len(toks)


VOCAB, EOS = _vocab()
BYTE_ID = {bytes([c.encode()[0]]): i for i, c in enumerate(ALPHABET)}
BY_LEN = sorted(range(EOS), key=lambda i: -len(VOCAB[i]))


def _per_byte(s: bytes):
    return [BYTE_ID[bytes([c])] for c in s]


def _greedy_longest(s: bytes):
    out, i = [], 0
    while i < len(s):
        t = next(v for v in BY_LEN if s.startswith(VOCAB[v], i))
        out.append(t)
        i += len(VOCAB[t])
    return out


@pytest.fixture(scope="module")
def compiled():
    return {p: TokenFSM.from_regex(p, VOCAB, EOS) for p in PATTERNS}


@pytest.mark.parametrize("pattern", PATTERNS)
def test_random_walks_that_reach_eos_full_match(compiled, pattern):
    fsm = compiled[pattern]
    rx = re.compile(pattern.encode())
    rng = np.random.default_rng(11)
    finished = 0
    for _ in range(500):
        s, out = fsm.start, []
        for _ in range(12):
            ids = fsm.allowed(s)
            assert len(ids), (pattern, s)
            t = int(rng.choice(ids))
            s = fsm.step(s, t)
            assert s != DEAD
            if t == EOS:
                break
            out.append(t)
        else:
            continue                                                # 12 tokens without eos: discarded
        finished += 1
        text = b"".join(VOCAB[t] for t in out)
        assert rx.fullmatch(text), (pattern, out, text)
        assert fsm.allowed(s).tolist() == [EOS]                    # the terminal state
    assert finished >= 50, (pattern, finished)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_every_short_string_agrees_with_re(compiled, pattern):
    fsm = compiled[pattern]
    rx = re.compile(pattern.encode())
    n_acc = 0
    for n in range(7):
        for chars in itertools.product(ALPHABET, repeat=n):
            s = "".join(chars).encode()
            if rx.fullmatch(s):
                n_acc += 1
                for toks in (_per_byte(s), _greedy_longest(s)):
                    assert fsm.accepts(toks), (pattern, s, toks)
                    assert EOS in fsm.allowed(fsm.walk(fsm.start, toks)), (pattern, s, toks)
            else:
                assert not fsm.accepts(_per_byte(s)), (pattern, s)
    assert n_acc >= 3, (pattern, n_acc)


def test_check_invariant_and_restatement_walk(compiled):
    rng = np.random.default_rng(3)
    for p, fsm in compiled.items():
        fsm.check()
        assert fsm.next.dtype == np.uint16 and fsm.next.shape == (fsm.S, len(VOCAB)) and 1 <= fsm.S <= 65534
        masks = G.build_masks(fsm.next)
        for s in range(fsm.S):
            ids = fsm.allowed(s)
            assert np.array_equal(ids, np.flatnonzero(G.allowed_row(fsm.next, s, EOS)))
            bits = [(int(masks[s, v // 32]) >> (v % 32)) & 1 for v in range(fsm.V)]
            assert np.array_equal(np.flatnonzero(bits), ids)
        for _ in range(50):
            toks = rng.integers(-1, fsm.V + 1, size=int(rng.integers(0, 6))).tolist()
            assert fsm.walk(fsm.start, toks) == G.walk(fsm.next, fsm.start, toks), (p, toks)
        assert fsm.walk(-1, [1, 2]) == -1 and fsm.walk(DEAD, [EOS]) == DEAD and fsm.allowed(DEAD).tolist() == [EOS]
        assert fsm.walk(fsm.start, [fsm.V]) == DEAD                # an id outside the vocabulary
    # a table that breaks the invariant is caught
    fsm = compiled["a{2,}"]
    broken = fsm.next.copy()
    broken[fsm.start] = NONE
    with pytest.raises(ValueError, match="allows no token"):
        TokenFSM(broken, fsm.start, EOS).check()
    trap = np.full((3, fsm.V), NONE, dtype=np.uint16)
    trap[0, 0], trap[0, 1], trap[1, EOS], trap[2, EOS], trap[0, 2] = 1, 0, 2, 2, 0
    TokenFSM(trap, 0, EOS).check()
    trap2 = np.vstack([trap, np.full((1, fsm.V), NONE, dtype=np.uint16)])
    trap2[0, 3], trap2[3, 3] = 3, 3                                # state 3 loops for ever: not live
    with pytest.raises(ValueError, match="no accepting state"):
        TokenFSM(trap2, 0, EOS).check()
    trap3 = trap.copy()
    trap3[2, 0] = 0                                                # the state behind eos allows more than eos
    with pytest.raises(ValueError, match="terminal"):
        TokenFSM(trap3, 0, EOS).check()


def test_union_offsets_and_members_behave_as_alone(compiled):
    members = [compiled[p] for p in PATTERNS[:4]]
    merged, starts = TokenFSM.union(members)
    assert merged.S == sum(f.S for f in members)
    off = 0
    for f, st in zip(members, starts):
        assert st == off + f.start
        off += f.S
    merged.check(starts)
    rng = np.random.default_rng(9)
    for f, st in zip(members, starts):
        base = st - f.start
        for _ in range(200):
            s, m = f.start, st
            for _ in range(8):
                assert np.array_equal(f.allowed(s), merged.allowed(m))
                t = int(rng.choice(f.allowed(s))) if rng.random() < 0.9 else int(rng.integers(0, f.V))
                s, m = f.step(s, t), merged.step(m, t)
                assert (s == DEAD and m == DEAD) or m == s + base
                if s == DEAD:
                    break
    with pytest.raises(ValueError, match="differ"):
        TokenFSM.union([members[0], TokenFSM.from_choices([[1]], 10, 0)])


def test_from_choices_accepts_exactly_its_sequences():
    V, eos = 12, 11
    choices = [[1, 2, 3], [1, 2], [4], [1, 5, 5]]
    fsm = TokenFSM.from_choices(choices, V, eos)
    fsm.check()
    want = {tuple(c) for c in choices}
    for n in range(4):
        for seq in itertools.product(range(V - 1), repeat=n):
            assert fsm.accepts(seq) == (seq in want), seq
    assert fsm.allowed(fsm.start).tolist() == [1, 4]
    assert fsm.walk(fsm.start, [1, 2, eos, eos]) == fsm.S - 1 and fsm.allowed(fsm.S - 1).tolist() == [eos]
    for bad in ([], [[1, eos]], [[V]]):
        with pytest.raises(ValueError):
            TokenFSM.from_choices(bad, V, eos)


@pytest.mark.parametrize("pattern,word", [("^a", "anchor"), ("a$", "anchor"), (r"(a)\1", "backreference"), ("(?=a)b", "group extension"),
                                          ("(?P<x>a)", "group extension"), ("a*?", "lazy"), (r"\bab", "escape"), ("a{2", "repeat count"),
                                          ("(a", "unbalanced"), ("a)", "unbalanced"), ("[ab", "unterminated"), ("*a", "nothing to repeat"),
                                          ("[[:alpha:]]", "POSIX"), ("a{3,2}", "repeat count")])
def test_unsupported_constructs_are_named(pattern, word):
    with pytest.raises(ValueError, match=word):
        TokenFSM.from_regex(pattern, VOCAB, EOS)


def test_oversize_tables_and_unspellable_grammars_are_refused():
    with pytest.raises(ValueError, match=r"\d+ bytes"):
        TokenFSM.from_regex("a{2,}", VOCAB, EOS, max_table_bytes=100)
    with pytest.raises(ValueError, match=r"\d+ bytes"):
        TokenFSM.from_choices([[1, 2, 3]], 12, 11, max_table_bytes=50)
    a, b = TokenFSM.from_choices([[1]], 12, 11), TokenFSM.from_choices([[2]], 12, 11)
    with pytest.raises(ValueError, match=r"\d+ bytes"):
        TokenFSM.union([a, b], max_table_bytes=a.S * 12 * 2)
    with pytest.raises(ValueError, match="vocabulary can spell"):
        TokenFSM.from_regex("c+", VOCAB, EOS)
    with pytest.raises(ValueError, match="eos_id"):
        TokenFSM.from_regex("a", VOCAB, len(VOCAB))


def test_from_tokenizer_drops_special_and_undecodable_ids():
    class Tok:
        eos_token_id = 5
        all_special_ids = [4, 5]

        def decode(self, ids):
            return ["a", "b", "ab", "\ufffd", "a", "", "b"][ids[0]]

    fsm = from_tokenizer("(ab)+", Tok(), 7)
    assert fsm.eos_id == 5 and fsm.V == 7
    assert fsm.allowed(fsm.start).tolist() == [0, 2]              # id 4 spells "a" too, but is special
    assert fsm.accepts([0, 1, 2]) and fsm.accepts([0, 6]) and not fsm.accepts([0]) and not fsm.accepts([3])


def test_host_rules_keep_repeats_for_a_row_under_a_grammar():
    """_rules_batch(dedup=False): neither the overlap with the generated tail, nor the zero-accept de-duplication, nor the
    sequence update's overlap rule drops a token; with dedup (the default) each of them still does"""
    from types import SimpleNamespace

    from src.specdec.core.pipeline import SpeculativePipeline, _Row

    pipe = SimpleNamespace(base_lm=SimpleNamespace(vocab_size=100))

    def run(dedup, a, t, seq=(9, 8, 7), gen=(7,)):
        row = _Row(list(seq))
        row.generated = list(gen)
        SpeculativePipeline._rules_batch(pipe, row, 4, a, list(t), 50, 99, None, dedup=dedup)
        return row

    r = run(False, 2, [7, 7, 5, 0, 0])                  # accepted 7, 7 + bonus 5 after a generated 7
    assert r.generated == [7, 7, 7, 5] and r.seq == [9, 8, 7, 7, 7, 5] and r.active
    r = run(True, 2, [7, 7, 5, 0, 0])
    assert r.generated != [7, 7, 7, 5] and len(r.seq) < 6
    r = run(False, 0, [7, 1, 2, 3, 4])                  # zero accept, the base token repeats the last generated one
    assert r.generated == [7, 7] and r.seq == [9, 8, 7, 7]
    r = run(True, 0, [7, 1, 2, 3, 4])
    assert r.generated == [7] and r.seq == [9, 8, 7]
    r = run(False, 2, [5, 99, 99, 99, 99])              # the EOS cut and the bonus EOS stay: accepted 5, eos -> 5, eos, row stops
    assert r.generated == [7, 5, 99] and not r.active
