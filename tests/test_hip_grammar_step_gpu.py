"""The grammar inside the captured step (sd_specdec_set_grammar) against the CPU restatement (tests/grammar_ref.py): per step,
the restatement applied to the target's own raw rows with the row's state from BEFORE the step must give the stored rows, the
ids, the accept length, the emitted tokens and the advanced state — all integers and bf16 words, compared for equality. The
draft's side shows in its proposals (greedy) or in its stored rows (speculative sampling): every position masked by the state
after the step's own earlier draft tokens.

The automata here are random tables, not compiled grammars: every state allows about half the vocabulary, so the synthetic
pairs' ~120 on the successor token is masked away about every second position and the runs both accept and reject."""

import numpy as np
import pytest
import torch

import grammar_ref as G
import logit_proc_ref as L
import spec_sample_ref as RS
import spec_shape_ref as RH
from helpers import synthetic_prompts, tiny_pair
from specdec_hip.grammar import TokenFSM
from test_hip_logit_proc_gpu import CAP, PEN, _bits_of, _greedy_accept, _records
from test_hip_spec_sample_gpu import SEL_TGT, _persist_pair, _pipe

pytestmark = pytest.mark.gpu

IDENTITY = (1.0, 0.0, 0.0)


def _fsm(V, seed=5, S=5):
    rng = np.random.default_rng(seed)
    nxt = rng.integers(0, S, (S, V)).astype(np.uint16)
    nxt[rng.random((S, V)) >= 0.5] = G.NONE
    return TokenFSM(nxt, 0, V - 1)


def _check_steps_fsm(pipe, prompts, K, states, params, n_steps, use_graph, mode="greedy", T=20.0, seed=4321, top_k=None, top_p=None):
    """_check_steps of test_hip_logit_proc_gpu.py with the grammar line: `states` are the rows' states before the first step"""
    from specdec_hip.engine import HipSpecDec

    B = len(prompts)
    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    loop = sess.loop
    loop.sync()
    V = loop.target.cfg.vocab
    fsm = _fsm(V)
    nxt, eos = fsm.next, fsm.eos_id
    counters = [5 * b for b in range(B)]
    if mode != "greedy":
        loop.set_spec_sampling(True, T, seed, stream_ids=list(range(B)), draw_counts=counters, top_k=top_k, top_p=top_p)
    loop.set_logit_processors(True, *params)
    loop.set_grammar(fsm)
    assert loop.grammar is fsm and loop.grammar_state.cpu().tolist() == [-1] * B
    counts = np.stack([L.counts_set(V, p) for p in prompts])
    for b, p in enumerate(prompts):
        loop.set_logit_counts_row(b, p)
        loop.set_grammar_state(b, states[b])
    torch.cuda.synchronize()
    state = np.array(states, dtype=np.int64)
    last = [p[-1] for p in prompts]
    cur = [len(p) - 1 for p in prompts]
    lens, close, masked = [], 0, 0
    for step in range(n_steps):
        loop.step(use_graph=use_graph)
        rec = loop.sync()
        stored = _bits_of(loop.step_logits)
        d = rec.draft_tokens.astype(np.int32)
        toks = torch.from_numpy(np.concatenate([np.array(last, np.int32)[:, None], d], 1)).cuda()
        _, raw = loop.target.forward(toks, torch.tensor(cur, dtype=torch.int32, device="cuda"), want_logits=True, logits_dtype=torch.bfloat16)
        torch.cuda.synchronize()
        raw = _bits_of(raw)
        want, want_ids = G.process_rows_fsm(raw, counts, nxt, state, eos, d, None, *params)
        plain, _ = L.process_rows(raw, counts, d, None, *params)
        assert np.array_equal(stored, want), (step, np.argwhere(stored != want)[:4])
        masked += int((want != plain).sum())
        assert rec.target_ids.tolist() == want_ids.tolist(), step
        p = L.bf16_to_f32(stored)
        for b in range(B):
            # the draft's side: position i was masked by the state after d_1..d_i of this very step
            for i in range(K):
                ok = G.allowed_row(nxt, G.walk(nxt, state[b], d[b][:i]), eos)
                if mode == "greedy":
                    assert ok[d[b][i]], (step, b, i)
                else:
                    q_bits = _bits_of(loop.spec_draft_logits[b, i])
                    assert (q_bits[~ok] == G.NEG_INF_BF16).all() and (q_bits[ok] != G.NEG_INF_BF16).any(), (step, b, i)
            if mode == "greedy":
                a = _greedy_accept(want_ids[b], d[b], K)
                emitted = [int(t) for t in want_ids[b][:a + 1]]
            else:
                q = loop.spec_draft_logits[b].float().cpu().numpy()
                if mode == "spec":
                    dd, res, emitted, c2 = RS.spec_step_ref(q, p[b], T, seed, counters[b], b)
                    close += res.close_calls(CAP)
                else:
                    dd, res, emitted, c2, m = RH.spec_step_ref(q, p[b], T, top_k, top_p, seed, counters[b], b)
                    close += res.close_calls(CAP) + int(m < CAP)
                assert d[b].tolist() == dd, (step, b)
                a, counters[b] = res.accept_len, c2
            assert int(rec.accept_len[b]) == a, (step, b)
            assert [int(t) for t in rec.new_tokens[b]] == emitted + [-1] * (K + 1 - len(emitted)), (step, b)
            if state[b] >= 0:
                assert G.walk(nxt, state[b], emitted) != G.DEAD or state[b] >= fsm.S, (step, b, emitted)
            lens.append(a)
            last[b] = emitted[-1]
            cur[b] += len(emitted)
        assert rec.cur_len.tolist() == cur, step
        counts = L.counts_add(counts, rec.new_tokens, rec.n_new)
        state = G.advance(nxt, state, rec.new_tokens, rec.n_new)
        assert np.array_equal(_bits_of(loop.logit_counts), counts), step
        assert loop.grammar_state.cpu().tolist() == state.tolist(), step
    assert close == 0 and masked > 0
    if mode != "greedy":
        loop.set_spec_sampling(False)
    loop.set_logit_processors(False)
    assert loop.grammar is None
    sess.finish()
    return lens


@pytest.mark.parametrize("B,use_graph", [(1, True), (1, False), (3, True), (3, False)])
def test_greedy_step_reproduces_restatement_on_its_own_raw_logits(B, use_graph):
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(B, 12, tgt.config.vocab).tolist()
    lens = _check_steps_fsm(_pipe(drf, tgt), prompts, 4, [0, -1, 3][:B], IDENTITY, 6, use_graph)
    assert len(set(lens)) >= 2, lens


def test_greedy_step_persistent_draft():
    """B = 1 on the persistent draft: the device-selected two forms of draft forward 0 leave one state chain"""
    drf, tgt = _persist_pair()
    prompts = synthetic_prompts(1, 9, SEL_TGT.vocab, seed=3).tolist()
    lens = _check_steps_fsm(_pipe(drf, tgt), prompts, 4, [2], IDENTITY, 6, True)
    assert len(set(lens)) >= 2, lens


def test_greedy_step_with_penalties_a_dead_row_and_an_unconstrained_one():
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(3, 12, tgt.config.vocab).tolist()
    _check_steps_fsm(_pipe(drf, tgt), prompts, 4, [2, G.DEAD, -1], PEN, 6, True)


@pytest.mark.parametrize("mode,top_k,top_p", [("spec", None, None), ("shaped", 50, 0.9)])
def test_spec_sampling_step_reproduces_restatement_on_processed_rows(mode, top_k, top_p):
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(3, 12, tgt.config.vocab).tolist()
    _check_steps_fsm(_pipe(drf, tgt), prompts, 4, [0, -1, 3], IDENTITY, 6, True, mode=mode, top_k=top_k, top_p=top_p)


@pytest.mark.parametrize("B", [1, 3])
def test_grammar_off_is_the_plain_stage(B):
    """unbound, the step is the stage's own: the same records and the same number of graph nodes; bound, one node more (the
    advance) and nothing else — the mask rides in the process launches"""
    from specdec_hip.engine import HipSpecDec

    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(B, 12, tgt.config.vocab).tolist()
    pipe = _pipe(drf, tgt)
    plain = _records(pipe, prompts, 6, True, lp=PEN)

    def run(bind):
        sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
        loop = sess.loop
        loop.sync()
        loop.set_logit_processors(True, *PEN)
        for b, p in enumerate(prompts):
            loop.set_logit_counts_row(b, p)
        fsm = _fsm(loop.target.cfg.vocab)
        if bind != "never":
            loop.set_grammar(fsm)                  # every row at -1: bound, but no row is constrained
        if bind == "unbound":
            loop.set_grammar(None)
        recs = []
        for _ in range(6):
            loop.step(use_graph=True)
            r = loop.sync()
            recs.append((r.accept_len.tolist(), r.n_new.tolist(), r.new_tokens.tolist(), r.draft_tokens.tolist(), r.target_ids.tolist(),
                         r.cur_len.tolist()))
        nodes = loop.graph_nodes
        loop.set_logit_processors(False)
        sess.finish()
        return recs, nodes

    never, n_never = run("never")
    unbound, n_unbound = run("unbound")
    bound, n_bound = run("bound")
    assert never == plain and unbound == plain and bound == plain
    assert n_never > 0 and n_unbound == n_never and n_bound == n_never + 1
