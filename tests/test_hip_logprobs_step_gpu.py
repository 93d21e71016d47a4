"""Per-token log-probs inside the captured step (sd_specdec_set_logprobs; logprobs= / best_of= on the pipeline) on the small synthetic
pair with a softened target (soft_pair of test_hip_typical_step_gpu.py: the synthetic target is otherwise one-hot and every log-prob
would be ~0): the tokens do not move; every record entry equals the float64 restatement (tests/logprobs_ref.py) of the row the kernel
read; launch-ahead slots; token-to-row alignment end to end, through an admission and void steps; processed rows; off is off;
best_of."""

import numpy as np
import pytest
import torch

import logprobs_ref as R
from helpers import synthetic_prompts, tiny_pair

pytestmark = pytest.mark.gpu

K = 4


def _pipe(drf, tgt, policy="longest_prefix", policy_params=None, k=K):
    from src.specdec import HipLM, SpeculativePipeline

    return SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=HipLM(drf.to("cuda")), controller="fixed", controller_params={"k": k},
                               seed=1234, policy=policy, policy_params=policy_params)


@pytest.fixture(scope="module")
def soft_pair():
    drf, tgt = tiny_pair(flip_fraction=0.25)
    tgt.final_norm_w = (tgt.final_norm_w.float() * (4.0 / tgt.config.d_model)).to(tgt.final_norm_w.dtype)
    return drf, tgt


@pytest.fixture(scope="module")
def pipe(soft_pair):
    return _pipe(*soft_pair)


def _rows(results, steps=False):
    return [(r["generated_tokens"], r["proposed"], r["accepted"]) + ((r["steps"],) if steps else ()) for r in results]


# ---------------------------------------------------------------------------------------------------- 1. the tokens do not move
@pytest.mark.parametrize("B", [1, 2])
def test_tokens_are_unchanged(pipe, soft_pair, B):
    V = soft_pair[1].config.vocab
    prompts = synthetic_prompts(B, 12, V).tolist()
    plain, with_lp = pipe.generate_batch(prompts, max_tokens=24), pipe.generate_batch(prompts, max_tokens=24, logprobs=5)
    assert _rows(plain) == _rows(with_lp)
    assert "logprobs" not in plain[0] and all(len(r["logprobs"]) == r["num_generated"] for r in with_lp)
    assert _rows(pipe.generate_batch(prompts, max_tokens=24)) == _rows(plain)          # and the loop is what it was afterwards


def test_tokens_are_unchanged_through_an_admission(pipe, soft_pair):
    V = soft_pair[1].config.vocab
    prompts = synthetic_prompts(3, 10, V, seed=77).tolist()                            # 3 prompts through 2 slots
    plain = pipe.generate_many(prompts, max_tokens=16, batch_size=2)
    with_lp = pipe.generate_many(prompts, max_tokens=16, batch_size=2, logprobs=5)
    assert _rows(plain, True) == _rows(with_lp, True)


# ---------------------------------------------------------------------------------------------------- 2. the numbers
MODES = {
    "greedy": ("longest_prefix", None, None),
    "do_sample": ("longest_prefix", None, {"temperature": 0.9, "top_k": 20, "top_p": None, "seed": 31}),
    "rejection": ("rejection", {"backend": "device", "temperature": 0.9, "seed": 7}, "spec"),
    "typical": ("typical", {"backend": "device", "p": 0.09, "delta": 0.3, "temperature": 0.7}, None),
}


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("mode", list(MODES))
def test_every_record_entry_equals_the_restatement(soft_pair, pipe, monkeypatch, mode, B):
    """After every advance(), with one step in flight at a time, each active row's entries i < n_new against logprobs_ref of
    step_logits[b, i] — the rows the kernel read: rank and top ids EQUAL, log-probs within logprobs_ref.bounds. Entries i >= n_new
    and the rows that are not active carry the "not emitted" record."""
    from specdec_hip.engine import HipSpecDec

    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", "0")
    drf, tgt = soft_pair
    V, N = tgt.config.vocab, 5
    policy, params, sampling = MODES[mode]
    p = pipe if policy == "longest_prefix" else _pipe(drf, tgt, policy, params)
    if sampling == "spec":
        sampling = p._spec_sampling_config({})
    sess = p.start_session(synthetic_prompts(B, 12, V).tolist(), 60, HipSpecDec.EMIT_BONUS, sampling, logprobs=N)
    assert not sess._early and sess.loop.logprobs == N
    compared, worst = 0, {}
    while sess.any_active() and sess.step < 8:
        if B == 2 and sess.step == 4 and sess.rows[1].active:      # stop row 1 the way the rules stop a row: frozen at the next launch
            sess.rows[1].active = False
            sess._flagged[1] = "freeze"
        active = [r.active for r in sess.rows]
        assert sess.advance()
        rec = sess.last_record
        rows = sess.loop.step_logits.to(torch.float64).cpu().numpy()
        for b in range(B):
            n_new = int(rec.n_new[b]) if active[b] else 0
            for i in range(K + 1):
                got = (rec.logprob[b, i], rec.rank[b, i], rec.top_ids[b, i], rec.top_logprobs[b, i])
                if i >= n_new:
                    assert R.none_record(got), (sess.step, b, i, got)
                    continue
                tok = int(rec.new_tokens[b][i])
                R.check_row(rows[b, i], tok, N, 8, got, worst)
            compared += 1 if n_new else 0
    sess.finish()
    assert compared >= 6, compared
    print(f"[logprobs step] {mode} B={B}: {compared} row-steps, measured / bound {worst.get('ratio', 0.0):.3f}  "
          f"worst abs error {worst.get('abs', 0.0):.3e}")


# ---------------------------------------------------------------------------------------------------- 3. slots
def _run_session(pipe, prompts, max_tokens, **kw):
    from specdec_hip.engine import HipSpecDec

    sess = pipe.start_session(prompts, max_tokens, HipSpecDec.EMIT_BONUS, step_limit=max_tokens, **kw)
    early = sess._early
    while sess.any_active():
        assert sess.advance()
    sess.finish()
    return early, [(list(r.generated), [(e.token, e.logprob, e.rank, tuple(e.top)) for e in r.token_info]) for r in sess.rows]


def test_launch_ahead_slots_give_the_same_numbers(pipe, soft_pair, monkeypatch):
    V = soft_pair[1].config.vocab
    prompts = synthetic_prompts(2, 12, V).tolist()
    early, ahead = _run_session(pipe, prompts, 32, logprobs=5)
    assert early
    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", "0")
    early, in_order = _run_session(pipe, prompts, 32, logprobs=5)
    assert not early
    assert ahead == in_order                                       # floats compared exactly: bit-identical numbers
    assert all(len(info) == len(gen) >= 8 for gen, info in ahead)


# ---------------------------------------------------------------------------------------------------- 4. alignment end to end
def _assert_aligned(results):
    for r in results:
        g = r["generated_tokens"]
        assert len(r["logprobs"]) == len(r["token_ranks"]) == len(r["top_logprobs"]) == r["num_generated"] == len(g)
        for j, tok in enumerate(g):
            assert r["token_ranks"][j] == 0, (j, tok, r["token_ranks"])
            assert r["top_logprobs"][j][0][0] == tok and r["top_logprobs"][j][0][1] == r["logprobs"][j], (j, tok, r["top_logprobs"][j][0])
        total = 0.0
        for x in r["logprobs"]:
            total += x
        assert r["cumulative_logprob"] == total and total < 0.0


def test_every_greedy_token_is_its_rows_argmax(pipe, soft_pair):
    """a greedy run without processors: a log-prob attached to the wrong token, row or step would not be rank 0 with itself on top"""
    V = soft_pair[1].config.vocab
    _assert_aligned(pipe.generate_batch(synthetic_prompts(2, 12, V).tolist(), max_tokens=32, logprobs=5))
    out = pipe.generate_many(synthetic_prompts(3, 10, V, seed=77).tolist(), max_tokens=16, batch_size=2, logprobs=5)
    _assert_aligned(out)
    assert all(r["num_generated"] >= 8 for r in out)
    # a run the host rules rewrite: the synthetic successor (7919 t + 1) mod 1000 has the 2-cycle 18 <-> 543, so a prompt that ends
    # inside it generates its own tail again, the overlap rules strip and delete tokens, and the row is resynchronised (steps launched
    # ahead are void for it)
    assert V == 1000 and (7919 * 18 + 1) % V == 543 and (7919 * 543 + 1) % V == 18
    prompts = synthetic_prompts(2, 12, V).tolist()
    prompts[0][-3:] = [18, 543, 18]
    out = pipe.generate_batch(prompts, max_tokens=32, logprobs=5)
    assert out[0]["batch_metrics"]["resyncs"] > 0
    _assert_aligned(out)
    assert all(r["num_generated"] >= 4 for r in out)


# ---------------------------------------------------------------------------------------------------- 5. processed rows
def test_a_banned_token_is_never_a_finite_alternative(pipe, soft_pair):
    V = soft_pair[1].config.vocab
    prompts = synthetic_prompts(1, 12, V).tolist()
    x = pipe.generate_batch(prompts, max_tokens=12)[0]["generated_tokens"][0]
    out = pipe.generate_batch(prompts, max_tokens=12, bad_token_ids=[x], logprobs=20)[0]
    assert x not in out["generated_tokens"] and out["num_generated"] >= 8
    for j, top in enumerate(out["top_logprobs"]):
        assert all(not (t == x and np.isfinite(lp)) for t, lp in top), (j, top)
        assert np.isfinite(out["logprobs"][j])


def test_under_a_grammar_every_finite_alternative_is_allowed(pipe, soft_pair):
    from specdec_hip.grammar import TokenFSM

    V = soft_pair[1].config.vocab
    eos = pipe.base_lm.get_tokenizer_info()["eos_token_id"]
    prompts = synthetic_prompts(2, 12, V).tolist()
    choices = [[10, 20, 30, 40], [10, 21, 31], [11, 22], [12, 23, 33, 43, 53]]
    fsm = TokenFSM.from_choices(choices, V, eos)
    out = pipe.generate_batch(prompts, max_tokens=12, grammar=fsm, logprobs=20)
    for r in out:
        g = r["generated_tokens"]
        assert g[-1] == eos and g[:-1] in choices and len(r["top_logprobs"]) == len(g)
        for j in range(len(g)):
            allowed = set(int(t) for t in fsm.allowed(fsm.walk(fsm.start, g[:j])))
            finite = [t for t, lp in r["top_logprobs"][j] if np.isfinite(lp)]
            assert finite and set(finite) <= allowed, (j, finite, sorted(allowed))
            assert g[j] in finite and np.isfinite(r["logprobs"][j])


# ---------------------------------------------------------------------------------------------------- 6. off is off
def test_off_returns_the_step_launch_for_launch(soft_pair):
    from specdec_hip.engine import HipSpecDec

    p = _pipe(*soft_pair)                                           # a loop that never had the mode
    V = soft_pair[1].config.vocab
    prompts = synthetic_prompts(1, 12, V).tolist()

    def nodes(**kw):
        sess = p.start_session(prompts, 40, HipSpecDec.EMIT_BONUS, **kw)
        for _ in range(3):
            assert sess.advance()
        n, loop = sess.loop.graph_nodes, sess.loop
        sess.finish()
        return n, loop

    fresh, loop = nodes()
    assert fresh > 0 and loop.logprobs is None
    on, loop_on = nodes(logprobs=5)
    assert loop_on is loop and loop.logprobs == 5
    assert on > fresh                                               # the three launches for the fused tail, and the log-prob launch
    off, loop_off = nodes()
    assert loop_off is loop and loop.logprobs is None
    assert off == fresh                                             # back on the fused tail
    print(f"[logprobs step] graph nodes: never enabled {fresh}, on {on}, off again {off}")
    loop.set_logprobs(5)
    loop.set_logprobs(None)
    assert loop.logprobs is None and loop.sync().logprob is None


# ---------------------------------------------------------------------------------------------------- 7. best_of
def test_best_of_returns_the_most_likely_rows(pipe, soft_pair):
    V = soft_pair[1].config.vocab
    prompts = synthetic_prompts(2, 12, V).tolist()
    kw = dict(max_tokens=16, do_sample=True, temperature=1.0, seed=11)
    every = pipe.generate_batch(prompts, n=4, logprobs=0, **kw)
    best = pipe.generate_batch(prompts, n=2, best_of=4, **kw)
    assert len(every) == 8 and len(best) == 4 and best[0]["batch_metrics"]["best_of"] == 4
    assert len({tuple(r["generated_tokens"]) for r in every}) > 2          # the rows differ: there is something to rank
    for p in range(2):
        group = every[4 * p:4 * p + 4]
        order = sorted(range(4), key=lambda j: (-group[j]["cumulative_logprob"], j))[:2]
        got = best[2 * p:2 * p + 2]
        assert [r["generated_tokens"] for r in got] == [group[j]["generated_tokens"] for j in order]
        assert [r["cumulative_logprob"] for r in got] == [group[j]["cumulative_logprob"] for j in order]
        assert got[0]["cumulative_logprob"] >= got[1]["cumulative_logprob"]
    with pytest.raises(ValueError, match="best_of needs a sampling mode"):
        pipe.generate_batch(prompts, n=2, best_of=4, max_tokens=8)
