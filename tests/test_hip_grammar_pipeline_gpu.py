"""Grammars through the pipeline surface: generate_batch / generate / generate_many / start_session with grammar=, against a
CPU greedy decode of OracleLM under the automaton's mask (the restatement of tests/grammar_ref.py on every next-token row) —
the target's own greedy decoding under the grammar, which speculation must reproduce token for token — and the refusals of the
pipeline level.

The synthetic pairs put about 120 on the successor token and about 40 on the next best one. Where the mask removes the
successor, the choice falls among the ~40s, where two candidates can lie within a bf16 step or two of each other and the
device's and the oracle's differently ordered sums may pick differently. Prompts and grammars were therefore chosen on the CPU,
with the oracle alone, so that the smallest top-2 margin among allowed tokens over every run compared here is >= 1.0 (four bf16
steps at that magnitude); each test asserts that margin, which then shows a bad setup and not a device error."""

import numpy as np
import pytest
import torch

import grammar_ref as G
import logit_proc_ref as L
from helpers import synthetic_prompts, tiny_pair
from oracle.model_ref import OracleLM
from specdec_hip.grammar import TokenFSM
from test_hip_logit_proc_pipeline_gpu import _row_bits, _tokens
from test_hip_spec_sample_gpu import _pipe

pytestmark = pytest.mark.gpu

K = 4
V = 1000
EOS = V - 1
MARGIN = 1.0
VOCAB = [b"%03d" % i for i in range(V - 1)] + [None]          # a token's bytes: its id as three digits; eos spells nothing


def oracle_greedy(lm, prompt, n, fsm=None, start=-1):
    """oracle_greedy of test_hip_logit_proc_pipeline_gpu.py under a grammar: up to n tokens of the target's own greedy decoding
    with the mask of the row's state on each next-token row, ending with eos -> (tokens, smallest top-2 margin among allowed
    tokens)"""
    counts = np.zeros(lm.cfg.vocab, np.uint16)
    logits, past = lm.forward(torch.tensor([list(prompt)], dtype=torch.int64))
    out, margin, s = [], float("inf"), start
    for _ in range(n):
        bits = _row_bits(logits[0, -1])
        if fsm is not None and s >= 0:
            row = G.process_row_fsm(bits, counts, fsm.next, s, fsm.eos_id)
            ok = G.allowed_row(fsm.next, s, fsm.eos_id)
        else:
            row, ok = L.process_row(bits, counts), np.ones(len(bits), dtype=bool)
        t = L.argmax_bits(row)
        top = np.sort(L.bf16_to_f32(row)[ok])[::-1]
        if len(top) > 1:
            margin = min(margin, float(top[0] - top[1]))
        out.append(t)
        if fsm is not None and s >= 0:
            if t == fsm.eos_id:
                break
            s = G.step(fsm.next, s, t)
        logits, past = lm.forward(torch.tensor([[t]], dtype=torch.int64), past)
    return out, margin


@pytest.fixture(scope="module")
def pair():
    drf, tgt = tiny_pair(flip_fraction=0.25)
    assert tgt.config.vocab == V
    prompts = synthetic_prompts(4, 12, V, seed=202).tolist()      # (the oracle's smallest margin over the runs below is 2.0 with these)
    return drf, tgt, prompts, OracleLM(tgt, "bf16")


def _first_digit_class(plain_firsts):
    """the last digits that none of the plain runs' first tokens end in"""
    return "".join(str(d) for d in range(10) if all(t % 10 != d for t in plain_firsts))


def test_generate_batch_under_a_regex_is_the_targets_own_greedy_decoding_under_the_mask(pair):
    drf, tgt, prompts, lm = pair
    pipe = _pipe(drf, tgt, k=K)
    plain = _tokens(pipe.generate_batch(prompts[:2], max_tokens=16, do_sample=False))
    # the first token may not end in the digit either plain run starts with; then any tokens; then eos
    fsm = TokenFSM.from_regex(r"\d\d[%s](\d\d\d)*" % _first_digit_class([g[0] for g in plain]), VOCAB, EOS)
    got = pipe.generate_batch(prompts[:2], max_tokens=16, do_sample=False, grammar=fsm)
    assert all(loop.grammar is fsm for rt in pipe._runtimes.values() for loop in rt["loops"].values())
    for p, r, pl in zip(prompts, got, plain):
        g = r["generated_tokens"]
        want, margin = oracle_greedy(lm, p, len(g), fsm, fsm.start)
        assert margin >= MARGIN, margin
        assert not fsm.allowed(fsm.start).tolist().count(pl[0]) and g[0] != pl[0]
        assert len(g) >= 16 and g == want, (g, want)
        assert r["accepted"] > 0 and fsm.walk(fsm.start, g) != G.DEAD
    # no grammar: the stage goes off again and the run is the plain one
    assert _tokens(pipe.generate_batch(prompts[:2], max_tokens=16, do_sample=False)) == plain
    assert not any(loop.logit_processors or loop.grammar is not None for rt in pipe._runtimes.values() for loop in rt["loops"].values())


def _answers(lm, prompts):
    """three answers per the oracle's own walk: the plain continuation's tokens 1..3 (so the first plain token is not an answer's
    first), and two detours off it"""
    w = oracle_greedy(lm, prompts[0], 6)[0]
    return [w[1:4], [w[2], w[0], w[5]], [w[4], w[4], w[3], w[1]]]


def test_from_choices_gives_exactly_one_answer_then_eos_and_stops(pair):
    drf, tgt, prompts, lm = pair
    pipe = _pipe(drf, tgt, k=K)
    answers = _answers(lm, prompts)
    fsm = TokenFSM.from_choices(answers, V, EOS)
    got = pipe.generate_batch(prompts[:3], max_tokens=16, do_sample=False, grammar=fsm)
    for p, r in zip(prompts, got):
        g = r["generated_tokens"]
        want, margin = oracle_greedy(lm, p, 16, fsm, fsm.start)
        assert margin >= MARGIN, margin
        assert g == want and g[-1] == EOS and g[:-1] in answers, (g, want)


def test_mixed_rows_each_follow_their_own_automaton(pair):
    drf, tgt, prompts, lm = pair
    pipe = _pipe(drf, tgt, k=K)
    plain = _tokens(pipe.generate_batch(prompts[:3], max_tokens=12, do_sample=False))
    fsm = TokenFSM.from_regex(r"\d\d[%s](\d\d\d)*" % _first_digit_class([plain[0][0]]), VOCAB, EOS)
    fsm2 = TokenFSM.from_choices(_answers(lm, prompts), V, EOS)
    got = _tokens(pipe.generate_batch(prompts[:3], max_tokens=12, do_sample=False, grammar=[fsm, None, fsm2]))
    assert got[1] == plain[1]
    for b, f in ((0, fsm), (2, fsm2)):
        want, margin = oracle_greedy(lm, prompts[b], len(got[b]), f, f.start)
        assert margin >= MARGIN, margin
        assert got[b] == want and got[b] != plain[b], (b, got[b], want)
    assert len(got[0]) >= 12 and got[2][-1] == EOS


def test_a_token_allowed_twice_in_a_row_is_kept_twice(pair):
    """the overlap / de-duplication rules are off for a row under a grammar, and on for the row next to it"""
    drf, tgt, prompts, lm = pair
    pipe = _pipe(drf, tgt, k=K)
    t = 321
    fsm = TokenFSM.from_choices([[t, t, t, 77, 77]], V, EOS)
    got = _tokens(pipe.generate_batch(prompts[:2], max_tokens=12, do_sample=False, grammar=[fsm, None], allowed_token_ids=[t, 77, EOS]))
    assert got[0] == [t, t, t, 77, 77, EOS]
    # the unconstrained row meets the same repeats under the allowed set alone, and the host rules drop them as they always did
    alone = _tokens(pipe.generate_batch(prompts[:2], max_tokens=12, do_sample=False, allowed_token_ids=[t, 77, EOS]))
    assert got[1] == alone[1] and got[1] and set(got[1]) <= {t, 77, EOS}


def test_generate_many_admits_rows_in_their_own_start_state_and_generate_runs(pair):
    drf, tgt, prompts, lm = pair
    pipe = _pipe(drf, tgt, k=K)
    plain = _tokens(pipe.generate_batch(prompts[:3], max_tokens=12, do_sample=False))
    fsm = TokenFSM.from_regex(r"\d\d[%s](\d\d\d)*" % _first_digit_class([g[0] for g in plain]), VOCAB, EOS)
    fsm2 = TokenFSM.from_choices(_answers(lm, prompts), V, EOS)
    grammars = [fsm, fsm2, fsm]
    many = pipe.generate_many(prompts[:3], max_tokens=12, batch_size=2, do_sample=False, grammar=grammars)   # the third is admitted late
    assert many[0]["batch_size"] == 2
    for p, f, g in zip(prompts, grammars, _tokens(many)):
        want, margin = oracle_greedy(lm, p, len(g), f, f.start)
        assert margin >= MARGIN, margin
        assert g == want and (len(g) >= 12 or g[-1] == EOS), (g, want)
    # generate(): the draft-emit mode of the step, one row
    r = pipe.generate(prompts[0], max_tokens=10, do_sample=False, grammar=fsm)
    assert r["generated_tokens"] == oracle_greedy(lm, prompts[0], 10, fsm, fsm.start)[0]


def test_a_resynced_row_continues_on_the_oracles_tokens(pair):
    """a row whose device state is rebuilt mid-run (the steps launched ahead are void for it) gets its automaton state back
    from the host's in-order view: start state walked over what the row has kept"""
    from specdec_hip.engine import HipSpecDec

    drf, tgt, prompts, lm = pair
    pipe = _pipe(drf, tgt, k=K)
    plain = _tokens(pipe.generate_batch(prompts[:2], max_tokens=12, do_sample=False))
    fsm = TokenFSM.from_regex(r"(\d\d[%s])*" % _first_digit_class([g[0] for g in plain]), VOCAB, EOS)
    sess = pipe.start_session(prompts[:2], 20, HipSpecDec.EMIT_BONUS, None, step_limit=20, grammar=fsm)
    n = 0
    while sess.any_active():
        assert sess.advance()
        n += 1
        if n == 2:
            sess._flagged[0] = "resync"
            for _, void in sess._queue:
                void.add(0)
            sess.stats["resyncs"] += 1
    sess.finish()
    assert sess.stats["resyncs"] > 0 and sess.stats["void_row_steps"] > 0
    for p, r in zip(prompts, sess.rows):
        want, margin = oracle_greedy(lm, p, len(r.generated), fsm, fsm.start)
        assert margin >= MARGIN, margin
        assert len(r.generated) >= 20 and r.generated == want, (r.generated, want)


def test_refusals_at_the_pipeline_level(pair):
    from src.specdec import HipLM, SpeculativePipeline

    drf, tgt, prompts, _ = pair
    pipe = _pipe(drf, tgt, k=K)
    fsm = TokenFSM.from_choices([[5, 6]], V, EOS)
    with pytest.raises(NotImplementedError, match="do_sample"):
        pipe.generate(prompts[0], max_tokens=4, do_sample=True, grammar=fsm)
    with pytest.raises(ValueError, match="entries"):
        pipe.generate_batch(prompts[:2], max_tokens=4, do_sample=False, grammar=[fsm])
    with pytest.raises(ValueError, match="eos_id"):
        pipe.generate_batch(prompts[:1], max_tokens=4, do_sample=False, grammar=TokenFSM.from_choices([[5]], V, 7))
    with pytest.raises(ValueError, match="vocabulary"):
        pipe.generate_batch(prompts[:1], max_tokens=4, do_sample=False, grammar=TokenFSM.from_choices([[5]], 10, 9))
    with pytest.raises(TypeError, match="TokenFSM"):
        pipe.generate_batch(prompts[:1], max_tokens=4, do_sample=False, grammar="a+")
    for policy, pp in (("typical", {"p": 0.9}), ("topk_agree", {"k": 5}), ("conf_threshold", {"tau": 0.5}), ("rejection", {"backend": "host"})):
        hp = _pipe(drf, tgt, k=K, policy=policy, policy_params=pp)
        with pytest.raises(NotImplementedError, match="grammar"):
            hp.generate_batch(prompts[:1], max_tokens=4, do_sample=False, grammar=fsm)
        if policy != "rejection":
            with pytest.raises(NotImplementedError, match="grammar"):
                hp.generate(prompts[0], max_tokens=4, do_sample=False, grammar=fsm)
    for mode in ("medusa", "eagle"):
        mp = SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=HipLM(drf.to("cuda")), controller="fixed", controller_params={"k": K},
                                 draft_mode=mode, seed=1234)
        with pytest.raises(NotImplementedError, match="draft-model mode"):
            mp.generate(prompts[0], max_tokens=4, do_sample=False, grammar=fsm)
    for cp in ({}, {"per_row": True, "initial_k": 2, "min_k": 1, "max_k": 4}):
        ap = SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=HipLM(drf.to("cuda")), controller="adaptive", controller_params=cp, seed=1234)
        with pytest.raises(NotImplementedError, match="fixed K"):
            ap.generate_batch(prompts[:1], max_tokens=4, do_sample=False, grammar=fsm)
    # the device's speculative sampling is a legal route: every row spells one of the answers
    sp = _pipe(drf, tgt, k=K, policy="rejection", policy_params={"backend": "device", "temperature": 20.0, "seed": 3})
    answers = [[5, 6, 7], [5, 8], [900, 901, 902, 903]]
    out = sp.generate_batch(prompts[:2], max_tokens=8, grammar=TokenFSM.from_choices(answers, V, EOS))
    assert all(r["generated_tokens"][-1] == EOS and r["generated_tokens"][:-1] in answers for r in out), _tokens(out)
    # the regex helper of the CLIs goes through the pipeline's own tokenizer: ids spelled in decimal
    rx = pipe.grammar_from_regex("(12|34)5?")
    assert rx is pipe.grammar_from_regex("(12|34)5?") and rx.eos_id == EOS
    assert rx.accepts([12]) and rx.accepts([1, 2, 5]) and rx.accepts([345]) and not rx.accepts([13])
