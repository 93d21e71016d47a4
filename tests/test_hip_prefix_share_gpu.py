"""share_prefix / n of SpeculativePipeline on the GPU: rows that hold the same prompt are prefilled once and forked
(HipModel.fork_row), with the tokens of the unshared run; rows with a common prefix are forked over it."""

import pytest
import torch

from helpers import synthetic_prompts, tiny_pair

pytestmark = pytest.mark.gpu

L = 100          # prompt length: seq[:-1] is 99 >= 96 positions, so every prefilled row counts in prefill_counts()


def _pipe(policy="longest_prefix", policy_params=None, k=3, **lm_kw):
    from src.specdec import HipLM, SpeculativePipeline

    drf, tgt = tiny_pair()
    return SpeculativePipeline(base_lm=HipLM(tgt.to("cuda"), **lm_kw), draft_lm=HipLM(drf.to("cuda"), **lm_kw), controller="fixed",
                               controller_params={"k": k}, seed=1234, policy=policy, policy_params=policy_params)


def _prompt(seed=77):
    drf, _ = tiny_pair()
    return synthetic_prompts(1, L, drf.config.vocab, seed=seed)[0].tolist()


def _counts(pipe):
    """prompt rows absorbed so far, per engine, over every runtime of the pipeline"""
    out = {"target": 0, "draft": 0}
    for rt in pipe._runtimes.values():
        for role in out:
            out[role] += sum(rt[role].prefill_counts().values())
    return out


def _same(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        for key in ("generated_tokens", "proposed", "accepted", "sequence"):
            assert g[key] == w[key], key


MODES = {
    "greedy": ({}, {"do_sample": False}),
    "sampled": ({}, {"do_sample": True, "temperature": 0.8, "seed": 5}),
    "rejection_device": ({"policy": "rejection", "policy_params": {"backend": "device", "temperature": 0.9, "seed": 11}}, {}),
}


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("lm_kw", [{}, {"kv_page_len": 32}], ids=["dense", "paged"])
def test_equal_prompts_are_prefilled_once_with_the_tokens_of_the_unshared_run(mode, lm_kw):
    pkw, gkw = MODES[mode]
    pipe = _pipe(**pkw, **lm_kw)
    p = _prompt()
    c0 = _counts(pipe)
    want = pipe.generate_batch([p] * 4, max_tokens=20, **gkw)
    c1 = _counts(pipe)
    got = pipe.generate_batch([p] * 4, max_tokens=20, share_prefix=True, **gkw)
    c2 = _counts(pipe)
    _same(got, want)
    for role in ("target", "draft"):
        assert c1[role] - c0[role] >= 4          # (>=: a row the host rules rewrote is prefilled again)
        assert c2[role] - c1[role] == (c1[role] - c0[role]) - 3, role        # one prompt row instead of four
    bm = got[0]["batch_metrics"]
    assert (bm["forked_rows"], bm["prefilled_rows"], bm["shared_positions"]) == (3, 1, 3 * (L - 1))
    wm = want[0]["batch_metrics"]
    assert (wm["forked_rows"], wm["prefilled_rows"], wm["shared_positions"]) == (0, 4, 0)     # defaults: nothing is forked
    if lm_kw:
        for rt in pipe._runtimes.values():
            for role in ("target", "draft"):
                assert rt[role].page_len == 32 and rt[role].pages_in_use() > 0
                for b in range(4):
                    rt[role].release(b)
                assert rt[role].pages_in_use() == 0


def test_n_completions_equal_the_unshared_rows():
    pipe = _pipe()
    p = _prompt(seed=91)
    kw = {"do_sample": True, "temperature": 0.8, "seed": 3, "max_tokens": 16}
    want = pipe.generate_batch([p] * 4, **kw)
    got = pipe.generate_batch([p], n=4, **kw)
    _same(got, want)
    assert got[0]["batch_metrics"]["forked_rows"] == 3 and [r["batch_index"] for r in got] == [0, 1, 2, 3]
    # two prompts, n = 2: prompt-major
    q = _prompt(seed=92)
    both = pipe.generate_batch([p, q], n=2, **kw)
    assert [r["sequence"][:L] for r in both] == [p, p, q, q]
    assert both[0]["batch_metrics"]["forked_rows"] == 2 and both[0]["batch_metrics"]["prefilled_rows"] == 2


def test_generate_many_forks_over_a_common_prefix():
    """6 prompts = one 64-token prefix + 36 tokens of their own, two slots: the first row is prefilled, every other row —
    the second at the start, four admitted later — is forked over the 64 shared positions and forwards only its own part.
    (No token equality with the unshared run is asserted: the suffix is computed in other chunks than a whole-prompt
    prefill uses, so the two may differ at bf16 rounding level.)"""
    pipe = _pipe()
    V = pipe.base_lm.vocab_size
    prefix = synthetic_prompts(1, 64, V, seed=500)[0].tolist()
    prompts = [prefix + synthetic_prompts(1, L - 64, V, seed=600 + i)[0].tolist() for i in range(6)]
    assert all(a[64] != b[64] for i, a in enumerate(prompts) for b in prompts[i + 1:])      # exactly 64 tokens in common
    out = pipe.generate_many(prompts, max_tokens=12, batch_size=2, share_prefix=True, do_sample=False)
    assert len(out) == 6
    bm = out[0]["batch_metrics"]
    assert (bm["prefilled_rows"], bm["forked_rows"], bm["shared_positions"]) == (1, 5, 5 * 64)
    for p, r in zip(prompts, out):
        assert r["sequence"][:len(p)] == p and len(r["sequence"]) > len(p)
        assert r["num_generated"] == len(r["generated_tokens"]) >= 1
        assert r["steps"] >= 1 and r["proposed"] == 3 * r["steps"] and 0 <= r["accepted"] <= r["proposed"] + r["steps"]
        assert all(0 <= t < V for t in r["generated_tokens"])
    # a prefix shorter than min_shared_prefix is not worth a fork
    pipe.config["min_shared_prefix"] = 65
    out = pipe.generate_many(prompts[:3], max_tokens=4, batch_size=2, share_prefix=True, do_sample=False)
    assert out[0]["batch_metrics"]["forked_rows"] == 0 and out[0]["batch_metrics"]["prefilled_rows"] == 3


def test_defaults_fork_nothing_and_the_refusals():
    pipe = _pipe()
    p = _prompt(seed=8)
    out = pipe.generate_batch([p, p], max_tokens=6, do_sample=False)
    assert out[0]["batch_metrics"]["forked_rows"] == 0 and out[0]["batch_metrics"]["shared_positions"] == 0
    many = pipe.generate_many([p, p, p], max_tokens=6, batch_size=2, do_sample=False)
    assert many[0]["batch_metrics"]["forked_rows"] == 0 and many[0]["batch_metrics"]["prefilled_rows"] == 3
    sess = pipe.start_session([p, p], 6, 0)
    assert sess.stats["forked_rows"] == 0
    sess.finish()
    sess = pipe.start_session([p, p], 6, 0, share_prefix=True)
    assert sess.stats["forked_rows"] == 1 and sess.stats["shared_positions"] == L - 1
    sess.finish()
    torch.cuda.synchronize()
    with pytest.raises(NotImplementedError):
        pipe.generate(p, max_tokens=4, share_prefix=True)
    with pytest.raises(NotImplementedError):
        pipe.generate(p, max_tokens=4, n=2)
    with pytest.raises(ValueError):
        pipe.generate_batch([p], n=0)
    host = _pipe(policy="typical")
    with pytest.raises(NotImplementedError):
        host.generate_batch([p], max_tokens=4, n=2)
