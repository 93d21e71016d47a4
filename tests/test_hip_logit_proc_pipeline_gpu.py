"""Logit processors through the pipeline surface: generate_batch / generate / generate_many / start_session with
repetition_penalty, presence_penalty, frequency_penalty, logit_bias, bad_token_ids and allowed_token_ids, against a CPU greedy
decode of OracleLM with the restatement (tests/logit_proc_ref.py) applied to every row — the target's own greedy decoding under
the processors, which speculation must reproduce token for token — and the refusals of the pipeline level."""

import numpy as np
import pytest
import torch

import logit_proc_ref as L
from helpers import synthetic_prompts, tiny_pair
from oracle.model_ref import OracleLM
from test_hip_spec_sample_gpu import _pipe

pytestmark = pytest.mark.gpu

PEN = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2)
K = 4


def _row_bits(logits_row):
    return logits_row.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)


def oracle_greedy(lm, prompt, n, repetition_penalty=1.0, presence_penalty=0.0, frequency_penalty=0.0, bias=None):
    """n tokens of the target's own greedy decoding under the processors: the restatement on each next-token row, counts = the
    prompt's ids + everything generated so far"""
    V = lm.cfg.vocab
    counts = L.counts_set(V, prompt)
    logits, past = lm.forward(torch.tensor([list(prompt)], dtype=torch.int64))
    out = []
    for _ in range(n):
        row = L.process_row(_row_bits(logits[0, -1]), counts, (), repetition_penalty, presence_penalty, frequency_penalty, bias)
        t = L.argmax_bits(row)
        out.append(t)
        counts = L.counts_add(counts[None], [[t]], [1])[0]
        logits, past = lm.forward(torch.tensor([[t]], dtype=torch.int64), past)
    return out


@pytest.fixture(scope="module")
def pair():
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(3, 12, tgt.config.vocab).tolist()
    return drf, tgt, prompts, OracleLM(tgt, "bf16")


RP4 = dict(repetition_penalty=4.0)


def _seen_prompts(lm, prompts):
    """The synthetic pairs put ~120 on the successor token against ~40 on the best other one, which the penalties of PEN never
    bridge: they run, but leave these walks as they are. These prompts carry tokens 1-3 and 6-8 of their own greedy continuation
    in front; a repetition penalty of 4 (120 / 4 < 40) then turns the walk away wherever it would step on one of them. The
    restatement's smallest top-2 margin on these runs is 1.0, four bf16 steps at that magnitude."""
    out = []
    for p in prompts:
        w = oracle_greedy(lm, p, 8)
        out.append(w[:3] + w[5:8] + list(p))
    return out


def _tokens(results):
    return [r["generated_tokens"] for r in results]


def test_generate_batch_with_penalties_is_the_targets_own_greedy_decoding(pair):
    drf, tgt, prompts, lm = pair
    pipe = _pipe(drf, tgt, k=K)
    plain = _tokens(pipe.generate_batch(prompts[:2], max_tokens=16, do_sample=False))
    got = pipe.generate_batch(prompts[:2], max_tokens=16, do_sample=False, **PEN)
    assert all(loop.logit_processors for rt in pipe._runtimes.values() for loop in rt["loops"].values())
    for p, g, r in zip(prompts, _tokens(got), got):
        want = oracle_greedy(lm, p, len(g), **PEN)
        assert len(g) >= 16 and g == want, (g, want)
        assert r["accepted"] > 0
    # a case the processors change: the device run follows the restatement, not the plain walk
    seen = _seen_prompts(lm, prompts[1:3])
    plain_seen = _tokens(pipe.generate_batch(seen, max_tokens=16, do_sample=False))
    got = _tokens(pipe.generate_batch(seen, max_tokens=16, do_sample=False, **RP4))
    for p, g, pl in zip(seen, got, plain_seen):
        assert g == oracle_greedy(lm, p, len(g), **RP4) and g[0] != pl[0], (g, pl)
    # identity values switch the mode off again, and the run is the plain one
    again = pipe.generate_batch(prompts[:2], max_tokens=16, do_sample=False, repetition_penalty=1.0, presence_penalty=0, frequency_penalty=0)
    assert _tokens(again) == plain
    assert not any(loop.logit_processors for rt in pipe._runtimes.values() for loop in rt["loops"].values())


def test_ban_allowed_set_and_bias(pair):
    drf, tgt, prompts, lm = pair
    V = tgt.config.vocab
    pipe = _pipe(drf, tgt, k=K)
    plain = _tokens(pipe.generate_batch(prompts[:2], max_tokens=12, do_sample=False))
    banned = plain[0][2]
    assert all(banned in g for g in plain[:1])                     # the unprocessed run emits it
    got = _tokens(pipe.generate_batch(prompts[:2], max_tokens=12, do_sample=False, bad_token_ids=[banned]))
    assert all(banned not in g for g in got)
    bias = np.zeros(V, np.float32)
    bias[banned] = -np.inf
    assert got[0] == oracle_greedy(lm, prompts[0], len(got[0]), bias=bias)
    assert got[0][:2] == plain[0][:2] and got[0][2] != banned
    allowed = [5, 77, 300, 301, 999]
    got = _tokens(pipe.generate_batch(prompts[:2], max_tokens=12, do_sample=False, allowed_token_ids=allowed, repetition_penalty=1.2))
    # (a token emitted twice in a row meets the reference's overlap rules on the host, which drop it: such runs come out short)
    assert all(g and set(g) <= set(allowed) for g in got), got
    assert len(set(got[0])) > 1                                    # (the penalty moves the choice inside the set)
    assert got[0][:4] == oracle_greedy(lm, prompts[0], 4, repetition_penalty=1.2, bias=np.where(np.isin(np.arange(V), allowed), 0, -np.inf).astype(np.float32))


def test_logit_bias_of_100_makes_every_token_that_id():
    """The synthetic pairs put ~ sqrt(d_model) * |e| = 120-130 on the successor token by construction, more than any bias of 100 can
    overcome; with layer_gain = 5 the random layers drown that signal and the target's logits stay within +-45, so the biased id
    leads every row by more than 10."""
    drf, tgt = tiny_pair(flip_fraction=0.25, layer_gain=5.0)
    prompts = synthetic_prompts(2, 12, tgt.config.vocab).tolist()
    pipe = _pipe(drf, tgt, k=K)
    got = _tokens(pipe.generate_batch(prompts, max_tokens=10, do_sample=False, logit_bias={321: 100.0}))
    assert all(len(g) >= 2 and set(g) == {321} for g in got), got     # (the host's overlap rules drop immediate repeats: the run is short)


def test_generate_in_draft_emit_mode_and_config_key(pair, tmp_path):
    from src.specdec import HipLM, SpeculativePipeline

    drf, tgt, prompts, lm = pair
    pipe = _pipe(drf, tgt, k=K)
    r = pipe.generate(prompts[0], max_tokens=14, do_sample=False, **PEN)
    assert r["generated_tokens"] == oracle_greedy(lm, prompts[0], 14, **PEN) and r["accepted"] > 0
    seen = _seen_prompts(lm, prompts[1:2])[0]
    r = pipe.generate(seen, max_tokens=14, do_sample=False, **RP4)
    assert r["generated_tokens"] == oracle_greedy(lm, seen, 14, **RP4) != oracle_greedy(lm, seen, 14)
    # repetition_penalty in the config alone is honoured (1.3 as a call argument would be; 4.0 visibly); 1.0 leaves the mode off
    for value, on in ((1.3, True), (4.0, True), (1.0, False)):
        cfg = tmp_path / f"rp{value}.yaml"
        cfg.write_text(f"repetition_penalty: {value}\n")
        p2 = SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=HipLM(drf.to("cuda")), config_path=str(cfg), controller="fixed",
                                 controller_params={"k": K}, seed=1234)
        g = p2.generate(seen, max_tokens=14, do_sample=False)["generated_tokens"]
        assert g == oracle_greedy(lm, seen, 14, repetition_penalty=value)
        assert [loop.logit_processors for rt in p2._runtimes.values() for loop in rt["loops"].values()] == [on]
        if on:   # a call argument takes precedence over the config
            assert p2.generate(seen, max_tokens=14, do_sample=False, repetition_penalty=1.0)["generated_tokens"] == oracle_greedy(lm, seen, 14)


def test_generate_many_with_a_late_row_and_shared_prefix_rows_keep_their_own_counts(pair):
    drf, tgt, prompts, lm = pair
    pipe = _pipe(drf, tgt, k=K)
    prompts = _seen_prompts(lm, prompts)     # (every row's penalty acts on tokens of its own prompt only: mixed-up counts would show)
    single = [_tokens(pipe.generate_batch([p], max_tokens=14, do_sample=False, **RP4))[0] for p in prompts]
    for p, g in zip(prompts, single):
        assert g == oracle_greedy(lm, p, len(g), **RP4) != oracle_greedy(lm, p, len(g))
    many = pipe.generate_many(prompts, max_tokens=14, batch_size=2, do_sample=False, **RP4)      # the third prompt is admitted late
    assert _tokens(many) == single
    assert many[0]["batch_size"] == 2
    shared = pipe.generate_batch(prompts[:2], max_tokens=14, do_sample=False, share_prefix=True, n=2, **RP4)
    assert _tokens(shared) == [single[0], single[0], single[1], single[1]]
    assert shared[0]["batch_metrics"]["forked_rows"] == 2


def test_refusals_at_the_pipeline_level(pair):
    from src.specdec import HipLM, SpeculativePipeline

    drf, tgt, prompts, _ = pair
    V = tgt.config.vocab
    pipe = _pipe(drf, tgt, k=K)
    for kw, exc, word in (({"repetition_penalty": 0.0}, ValueError, "repetition_penalty"), ({"repetition_penalty": -2.0}, ValueError, "repetition_penalty"),
                          ({"repetition_penalty": float("nan")}, ValueError, "repetition_penalty"), ({"presence_penalty": float("inf")}, ValueError, "finite"),
                          ({"allowed_token_ids": []}, ValueError, "empty"), ({"bad_token_ids": [V]}, ValueError, "outside the vocabulary"),
                          ({"allowed_token_ids": [-1]}, ValueError, "outside the vocabulary"), ({"logit_bias": {V + 3: 1.0}}, ValueError, "outside the vocabulary")):
        for call in (lambda: pipe.generate_batch(prompts[:1], max_tokens=4, do_sample=False, **kw),
                     lambda: pipe.generate(prompts[0], max_tokens=4, do_sample=False, **kw),
                     lambda: pipe.generate_many(prompts[:1], max_tokens=4, do_sample=False, **kw)):
            with pytest.raises(exc, match=word):
                call()
    with pytest.raises(NotImplementedError, match="do_sample"):
        pipe.generate(prompts[0], max_tokens=4, do_sample=True, repetition_penalty=1.3)
    # the host-loop routes
    for policy, pp in (("typical", {"p": 0.9}), ("topk_agree", {"k": 5}), ("conf_threshold", {"tau": 0.5}), ("rejection", {"backend": "host"})):
        hp = _pipe(drf, tgt, k=K, policy=policy, policy_params=pp)
        with pytest.raises(NotImplementedError, match="logit processors"):
            hp.generate_batch(prompts[:1], max_tokens=4, do_sample=False, repetition_penalty=1.3)
        if policy != "rejection":
            with pytest.raises(NotImplementedError, match="logit processors"):
                hp.generate(prompts[0], max_tokens=4, do_sample=False, bad_token_ids=[7])
    # draft modes other than vanilla, adaptive K
    for mode in ("medusa", "eagle"):
        mp = SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=HipLM(drf.to("cuda")), controller="fixed", controller_params={"k": K},
                                 draft_mode=mode, seed=1234)
        with pytest.raises(NotImplementedError, match="draft-model mode"):
            mp.generate(prompts[0], max_tokens=4, do_sample=False, repetition_penalty=1.3)
    for cp in ({}, {"per_row": True, "initial_k": 2, "min_k": 1, "max_k": 4}):
        ap = SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=HipLM(drf.to("cuda")), controller="adaptive", controller_params=cp, seed=1234)
        with pytest.raises(NotImplementedError, match="fixed K"):
            ap.generate_batch(prompts[:1], max_tokens=4, do_sample=False, presence_penalty=0.5)
    # the device's speculative sampling is a legal route: the run goes through with the mode on
    sp = _pipe(drf, tgt, k=K, policy="rejection", policy_params={"backend": "device", "temperature": 20.0, "seed": 3})
    out = sp.generate_batch(prompts[:2], max_tokens=8, bad_token_ids=[960, 977], **PEN)
    assert all(len(r["generated_tokens"]) >= 8 and not {960, 977} & set(r["generated_tokens"]) for r in out)
