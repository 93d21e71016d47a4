"""Lossy acceptance inside the captured step (sd_specdec_set_acceptance; policy "typical" / "topk_agree" with backend "device") on
the small synthetic pair: top-k agreement at k = 1 IS longest_prefix; a self-draft is always fully accepted; the device's
decisions equal the float64 restatement (tests/typical_ref.py) on the target's rows recomputed by a second engine; bans and
grammars count; rule off leaves the step what it was."""

import numpy as np
import pytest
import torch

import typical_ref as R
from helpers import synthetic_prompts, tiny_pair

pytestmark = pytest.mark.gpu

K = 4


def _pipe(drf, tgt, policy="longest_prefix", policy_params=None, k=K):
    from src.specdec import HipLM, SpeculativePipeline

    return SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=HipLM(drf.to("cuda")), controller="fixed", controller_params={"k": k},
                               seed=1234, policy=policy, policy_params=policy_params)


@pytest.fixture(scope="module")
def pair():
    return tiny_pair(flip_fraction=0.25)


@pytest.fixture(scope="module")
def soft_pair():
    """The drafted pair with a target that is NOT all but one-hot. The synthetic target puts ~d_model nats between its successor
    token and the rest, so every token but the argmax has probability 0 at T = 0.7 and a lossy rule has nothing to accept. Its
    final norm weight is scaled by g = 4 / d_model: the successor then leads by ~4 logits over noise of ~4 / sqrt(d_model), the
    distribution is broad (H of several nats), min(0.09, 0.3 e^{-H}) is a few 1e-4, and the token a flipped draft proposes —
    an arbitrary one to the target — passes or fails by its own noise: lossy acceptances and rejections both occur."""
    drf, tgt = tiny_pair(flip_fraction=0.25)
    tgt.final_norm_w = (tgt.final_norm_w.float() * (4.0 / tgt.config.d_model)).to(tgt.final_norm_w.dtype)
    return drf, tgt


def _rows(results):
    return [(r["generated_tokens"], r["proposed"], r["accepted"]) for r in results]


# ---------------------------------------------------------------------------------------------------- a. k = 1 is longest_prefix
def test_topk_agree_k1_equals_longest_prefix(pair):
    drf, tgt = pair
    V = tgt.config.vocab
    exact = _pipe(drf, tgt)
    lossy = _pipe(drf, tgt, "topk_agree", {"backend": "device", "k": 1})
    for B in (1, 3):
        prompts = synthetic_prompts(B, 12, V).tolist()
        a, b = exact.generate_batch(prompts, max_tokens=24), lossy.generate_batch(prompts, max_tokens=24)
        assert _rows(a) == _rows(b), B
        assert a[0]["batch_metrics"]["total_steps"] == b[0]["batch_metrics"]["total_steps"]
    # launch-ahead is on for the rule (steps are queued ahead of the host's rules, as for greedy steps)
    from specdec_hip.engine import HipSpecDec
    sess = lossy.start_session(synthetic_prompts(1, 12, V).tolist(), 24, HipSpecDec.EMIT_BONUS)
    assert sess._early and sess._accept and sess.loop.acceptance == "topk_agree"
    sess.finish()
    # one admission: 3 prompts through 2 slots
    prompts = synthetic_prompts(3, 10, V, seed=77).tolist()
    a, b = exact.generate_many(prompts, max_tokens=16, batch_size=2), lossy.generate_many(prompts, max_tokens=16, batch_size=2)
    assert [(r["generated_tokens"], r["proposed"], r["accepted"], r["steps"]) for r in a] == \
           [(r["generated_tokens"], r["proposed"], r["accepted"], r["steps"]) for r in b]


# ---------------------------------------------------------------------------------------------------- b. self-draft
def test_self_draft_is_always_fully_accepted(pair):
    """p_max >= e^{-H} for any distribution (H >= -log p_max), so the target's own argmax passes min(0.3, 0.3 e^{-H}) whatever the
    bf16 near-ties between the draft pass and the verify pass do to WHICH token is the argmax."""
    from specdec_hip.engine import HipSpecDec

    _, tgt = pair
    pipe = _pipe(tgt, tgt, "typical", {"backend": "device", "p": 0.3, "delta": 0.3})
    sess = pipe.start_session(synthetic_prompts(2, 12, tgt.config.vocab).tolist(), 40, HipSpecDec.EMIT_BONUS)
    steps = 0
    while sess.any_active() and steps < 8:
        assert sess.advance()
        assert [int(x) for x in sess.last_record.accept_len] == [K, K], steps
        steps += 1
    sess.finish()
    assert steps >= 4


# ---------------------------------------------------------------------------------------------------- c. decisions against fp64
@pytest.mark.parametrize("do_sample", [False, True], ids=["greedy", "sampled"])
def test_device_decisions_equal_the_restatement(soft_pair, monkeypatch, do_sample):
    """Each step's draft tokens and accept length from the record; the K + 1 target rows for seq + drafts from a second engine over
    the same weights (HipLM.verify_tokens, rounded to the bf16 the step stores); the restatement must give the same accept
    length unless a position sits within 1e-3 of its threshold (at most 2 % of the positions). Emitted: d_1..d_a plus one — the
    row's argmax, or under do_sample the token sd_sample_token draws from that row with the same seed and draw index.
    Figures of the first run are in profiles/typical_accept.md."""
    from specdec_hip.engine import HipSpecDec
    from specdec_hip.ops import sample_token_hip
    from src.specdec import HipLM

    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", "0")       # one step at a time: the host's view of a row is the device's
    drf, tgt = soft_pair
    V = tgt.config.vocab
    eps, delta, T, seed = 0.09, 0.3, 0.7, 31
    pipe = _pipe(drf, tgt, "typical", {"backend": "device", "p": eps, "delta": delta, "temperature": T})
    second = HipLM(tgt.to("cuda"))
    prompts = synthetic_prompts(2, 12, V).tolist()
    sampling = {"temperature": 0.9, "top_k": 20, "top_p": None, "seed": seed} if do_sample else None
    sess = pipe.start_session(prompts, 40, HipSpecDec.EMIT_BONUS, sampling)
    under = total = lossy_accepts = compared = 0
    while sess.any_active() and sess.step < 10:
        before = [(list(r.seq), r.draws, r.active) for r in sess.rows]
        assert sess.advance()
        rec = sess.last_record
        for b, (seq, draws, active) in enumerate(before):
            if not active:
                continue
            d = [int(x) for x in rec.draft_tokens[b]]
            a = int(rec.accept_len[b])
            _, lg = second.verify_tokens(torch.tensor([seq]), torch.tensor([d]))
            rows = lg[0].to(torch.bfloat16)
            want, stats, margins = R.accept(rows.to(torch.float64).cpu().numpy()[None], [d], "typical", T=T, eps=eps, delta=delta)
            under += int((margins < 1e-3).sum())
            total += margins.size
            if margins.min() < 1e-3:
                continue
            compared += 1
            assert a == int(want[0]), (sess.step, b, a, want, stats[0], margins)
            arg = rows.float().argmax(dim=-1).cpu().tolist()
            lossy_accepts += sum(1 for i in range(a) if d[i] != arg[i])
            new = [int(x) for x in rec.new_tokens[b][: int(rec.n_new[b])]]
            assert new[:a] == d[:a] and len(new) == a + 1
            if do_sample:
                tok = sample_token_hip(rows[a], 0.9, 20, None, seed=seed, draw=draws,
                                       stream_ids=torch.tensor([b], dtype=torch.int32, device="cuda"))
                assert new[a] == int(tok.item()), (sess.step, b)
            else:
                assert new[a] == arg[a], (sess.step, b)
    sess.finish()
    print(f"[typical step] do_sample={do_sample}: {compared} row-steps compared, {under}/{total} positions under 1e-3, "
          f"{lossy_accepts} accepted tokens that are not the target's argmax")
    assert under <= 0.02 * total
    assert compared >= 6
    assert lossy_accepts >= 1, "no accepted token differs from the target's argmax: the run shows nothing longest_prefix does not"


# ---------------------------------------------------------------------------------------------------- d. with the processor stage
def test_bans_and_grammars_count(soft_pair, monkeypatch):
    from specdec_hip.engine import HipSpecDec
    from specdec_hip.grammar import TokenFSM

    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", "0")
    drf, tgt = soft_pair
    V = tgt.config.vocab
    eps, delta, T = 0.09, 0.3, 0.7
    pipe = _pipe(drf, tgt, "typical", {"backend": "device", "p": eps, "delta": delta, "temperature": T})
    prompts = synthetic_prompts(2, 12, V).tolist()
    free = pipe.generate_batch(prompts, max_tokens=16)
    banned = sorted({t for r in free for t in r["generated_tokens"][:6]})
    sess = pipe.start_session(prompts, 24, HipSpecDec.EMIT_BONUS, bad_token_ids=banned)
    checked = 0
    while sess.any_active() and sess.step < 6:
        active = [r.active for r in sess.rows]
        assert sess.advance()
        rec = sess.last_record
        rows = sess.loop.step_logits.to(torch.float64).cpu().numpy()          # the PROCESSED rows of this step
        for b in range(len(prompts)):
            if not active[b]:
                continue
            d, a = [int(x) for x in rec.draft_tokens[b]], int(rec.accept_len[b])
            assert all(np.isneginf(rows[b, :, t]).all() for t in banned)
            for i in range(a):                                               # every accepted token satisfies the rule on the processed row
                keep, pd, H, thr, _, margin = R.decide(rows[b, i], d[i], "typical", T=T, eps=eps, delta=delta)
                assert keep or margin < 1e-4, (b, i, pd, thr)
                checked += 1
            assert not set(int(x) for x in rec.new_tokens[b][: int(rec.n_new[b])]) & set(banned)
    sess.finish()
    assert checked >= 1
    assert not any(set(r.generated) & set(banned) for r in sess.rows)
    # a grammar: only the listed sequences can be emitted
    eos = pipe.base_lm.get_tokenizer_info()["eos_token_id"]
    choices = [[5, 6, 7, 8], [5, 9, 10], [11, 12]]
    fsm = TokenFSM.from_choices(choices, V, eos)
    out = pipe.generate_batch(prompts, max_tokens=8, grammar=fsm)
    for r in out:
        toks = [t for t in r["generated_tokens"] if t != eos]
        assert toks in choices, toks


# ---------------------------------------------------------------------------------------------------- e. off means unchanged
def test_rule_off_leaves_the_step_unchanged(pair):
    from specdec_hip.engine import HipSpecDec

    drf, tgt = pair
    prompts = synthetic_prompts(2, 12, tgt.config.vocab).tolist()

    def greedy_records(pipe, n=6):
        sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
        recs = []
        for _ in range(n):
            sess.loop.step(use_graph=True)
            r = sess.loop.sync()
            recs.append((r.accept_len.tolist(), r.new_tokens.tolist(), r.draft_tokens.tolist(), r.target_ids.tolist(), r.cur_len.tolist()))
        nodes = sess.loop.graph_nodes
        sess.finish()
        return recs, nodes

    never, nodes = greedy_records(_pipe(drf, tgt))
    assert nodes > 0
    pipe = _pipe(drf, tgt)
    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    loop = sess.loop
    loop.sync()
    loop.set_acceptance("typical", 0.7, 0.09, 0.3)
    for _ in range(3):
        loop.step(use_graph=True)
    loop.sync()
    on_nodes = loop.graph_nodes
    loop.set_acceptance(None)
    assert loop.graph_nodes == 0          # switching the rule off drops the captured step
    sess.finish()
    again, nodes2 = greedy_records(pipe)
    assert (again, nodes2) == (never, nodes)
    assert on_nodes != nodes               # the rule's step is another graph: stored logits, two launches in place of the fused tail
    # refusals of the setter
    from specdec_hip import _abi
    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    loop = sess.loop
    loop.sync()
    for kw, word in (({"temperature": 0.0}, "temperature"), ({"epsilon": 0.0}, "epsilon"), ({"delta": -1.0}, "delta")):
        with pytest.raises(_abi.HipLibraryError, match=word):
            loop.set_acceptance("typical", **kw)
    with pytest.raises(_abi.HipLibraryError, match="agree_k"):
        loop.set_acceptance("topk_agree", agree_k=0)
    loop.set_acceptance("typical")
    with pytest.raises(_abi.HipLibraryError, match="acceptance"):
        loop.set_spec_sampling(True, 1.0, 0)
    with pytest.raises(_abi.HipLibraryError, match="acceptance"):
        loop.set_adaptive(True, 2, 1, K)
    loop.set_acceptance(None)
    sess.finish()
