"""The rolling context window through the pipeline (context_window / attention_sinks; src/specdec/core/rolling.py, DecodeSession's
rolls, csrc/kv_evict.hip): rows that generate far past their cache, replayed on the CPU oracle under their own eviction schedule
(tests/rolling_ref.py); a run on undamped weights teacher-forced through the fp32 oracle; a window that is never reached; the
window next to the other modes of the captured step; and continuous batching.

The synthetic pair's greedy continuation is the successor walk t -> (7919 t + 1) mod 1000 with margins around 80: check (i) is a
check of bookkeeping (positions, schedule, lengths), not of numerics. Its prompts end in tokens whose walk has period 50 and does not
meet the EOS token, so no row ends early and the reference's de-duplication rules stay dormant. Check (ii) is the numerical one."""

import pytest
import torch

import grammar_ref as G
import rolling_ref as RR
import step_audit
from helpers import synthetic_prompts, tiny_pair
from oracle.model_ref import OracleLM
from specdec_hip import weights as W
from test_hip_spec_sample_gpu import _pipe

pytestmark = pytest.mark.gpu

K, WINDOW, SINKS = 4, 96, 4
V = 1000
EOS = V - 1


def _succ(t):
    return (7919 * t + 1) % V


def _walk(t, n):
    out = []
    for _ in range(n):
        t = _succ(t)
        out.append(t)
    return out


def _starts(n):
    """n tokens whose successor walk has period 50 and never meets EOS"""
    out = []
    for t in range(100, V):
        w = _walk(t, 50)
        if w[-1] == t and len(set(w)) == 50 and EOS not in w and not any(t in _walk(s, 50) for s in out):
            out.append(t)
        if len(out) == n:
            return out
    raise AssertionError("no such tokens")


def _prompts(lengths, seed=300):
    starts = _starts(len(lengths))
    out = []
    for i, n in enumerate(lengths):
        p = synthetic_prompts(1, n, V, seed=seed + i)[0].tolist()
        p[-1] = starts[i]
        out.append(p)
    return out


@pytest.fixture(scope="module")
def pair():
    drf, tgt = tiny_pair(flip_fraction=0.25)
    return drf, tgt, OracleLM(tgt, "bf16")


def _replays(lm, tgt, prompt, r, n_min):
    g = r["generated_tokens"]
    assert len(g) >= n_min and EOS not in g, (len(g), n_min)
    assert r["window_rebuilds"] == [] and r["sequence"] == list(prompt) + g
    want = RR.greedy_replay(lm, prompt, len(g), r["evictions"], SINKS, tgt.rope_cos, tgt.rope_sin)
    assert g == want, next((i, a, b) for i, (a, b) in enumerate(zip(g, want)) if a != b)


def test_rows_generate_past_their_cache_and_replay_on_the_oracle(pair):
    """(i) 300 tokens per row through caches of 128 positions"""
    drf, tgt, lm = pair
    prompts = _prompts((12, 24, 40))
    pipe = _pipe(drf, tgt, k=K)
    res = pipe.generate_batch(prompts, max_tokens=300, do_sample=False, context_window=WINDOW, attention_sinks=SINKS)
    rts = list(pipe._runtimes.values())
    assert rts and all(rt["l_max"] < 200 and rt["target"].l_max < 200 and rt["draft"].l_max < 200 for rt in rts)   # not sized by max_tokens
    for p, r in zip(prompts, res):
        assert len(r["evictions"]) >= 3 and all(d == 40 for _, d in r["evictions"]), r["evictions"]
        gs = [g for g, _ in r["evictions"]]
        assert gs == sorted(set(gs)) and all(len(p) + g - 40 * i <= WINDOW for i, g in enumerate(gs))     # the cache never held more than W
        _replays(lm, tgt, p, r, 300)
    m = res[0]["batch_metrics"]
    assert m["evictions"] == sum(len(r["evictions"]) for r in res) and m["evicted_positions"] == 40 * m["evictions"]
    print(f"[rolling] evictions per row {[r['evictions'] for r in res]}, resyncs {m['resyncs']}")


def test_a_window_that_is_never_reached_changes_nothing(pair):
    """(iii)"""
    drf, tgt, _ = pair
    prompts = _prompts((12, 24, 40))
    pipe = _pipe(drf, tgt, k=K)
    plain = pipe.generate_batch(prompts, max_tokens=48, do_sample=False)
    rolled = pipe.generate_batch(prompts, max_tokens=48, do_sample=False, context_window=512)
    for a, b in zip(plain, rolled):
        assert a["generated_tokens"] == b["generated_tokens"] and (a["proposed"], a["accepted"]) == (b["proposed"], b["accepted"])
        assert b["evictions"] == [] and "evictions" not in a
    for key in ("total_steps", "total_proposed", "total_accepted", "resyncs"):
        assert plain[0]["batch_metrics"][key] == rolled[0]["batch_metrics"][key], key


MODES = {
    "logprobs": dict(logprobs=0),
    "grammar": dict(grammar=True),
    "do_sample": dict(do_sample=True, temperature=0.7, top_k=50, seed=11),
    "rejection": dict(),
}


@pytest.mark.parametrize("mode", sorted(MODES))
def test_next_to_the_other_modes_of_the_step(pair, mode):
    """(iv) one short run each, every row rolling at least once"""
    from specdec_hip.grammar import TokenFSM

    drf, tgt, _ = pair
    prompts = _prompts((12, 40))
    kw = dict(MODES[mode])
    fsm = None
    if kw.pop("grammar", False):
        # whole 3-digit tokens, and no end before 160 of them: the row cannot stop on the automaton's eos within this run
        vocab = [b"%03d" % i for i in range(V - 1)] + [None]
        fsm = kw["grammar"] = TokenFSM.from_regex(r"(\d\d\d){160,160}", vocab, EOS)
    kw.setdefault("do_sample", False)
    n = 110

    def run():
        pipe = (_pipe(drf, tgt, k=K, policy="rejection", policy_params={"backend": "device", "temperature": 0.7, "seed": 5})
                if mode == "rejection" else _pipe(drf, tgt, k=K))
        if mode == "rejection":
            kw.pop("do_sample", None)
        return pipe.generate_batch(prompts, max_tokens=n, context_window=WINDOW, attention_sinks=SINKS, **kw)
    res = run()
    for p, r in zip(prompts, res):
        g = r["generated_tokens"]
        assert len(g) >= n and len(r["evictions"]) >= 1, (len(g), r["evictions"])
        if mode == "logprobs":
            assert len(r["logprobs"]) == len(g) == len(r["token_ranks"]) and all(lp <= 0.0 for lp in r["logprobs"])
        if fsm is not None:
            assert fsm.walk(fsm.start, g) != G.DEAD and EOS not in g
    if mode in ("do_sample", "rejection"):
        again = run()
        assert [r["generated_tokens"] for r in again] == [r["generated_tokens"] for r in res]
        assert [r["evictions"] for r in again] == [r["evictions"] for r in res]


def test_continuous_batching_rolls_every_admitted_row(pair):
    """(v) 5 prompts over 2 slots"""
    drf, tgt, lm = pair
    prompts = _prompts((40, 12, 24, 17, 33), seed=320)
    pipe = _pipe(drf, tgt, k=K)
    res = pipe.generate_many(prompts, max_tokens=100, batch_size=2, do_sample=False, context_window=WINDOW, attention_sinks=SINKS)
    assert len(res) == 5
    for p, r in zip(prompts, res):
        assert len(r["evictions"]) >= 1
        _replays(lm, tgt, p, r, 100)
    assert res[0]["batch_metrics"]["evictions"] == sum(len(r["evictions"]) for r in res)


LLAMA3 = {"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 64, "rope_type": "llama3"}


def test_undamped_weights_follow_the_fp32_oracle_over_its_rolled_cache():
    """(ii) Sensitivity. A 2-layer random_init(std=0.1) target with a rolled-head draft, one row, 240 tokens through a window of 96.
    The fp32 oracle is teacher-forced along the device's own tokens and eviction events (its cache rolled as the kernel rolls, bf16
    rounding of the moved keys included): every emitted token's oracle logit must lie within the gate — 3 % of the row's max
    |logit| — of the row's maximum, at most 2 % of the positions excepted. The EOS token is banned (bad_token_ids) so that the row
    cannot end early; the oracle's rows are masked alike. The same walk with the cache moved but not rotated must leave more than
    half of the positions after the first eviction outside the gate (a CPU-side condition: the test can see the defect), and
    acceptance over the steps after the first eviction must be at least half of what it was before (a draft cache left unrolled
    agrees with the target at about 15 % of the positions)."""
    from specdec_hip.engine import HipSpecDec
    from src.specdec import HipLM, SpeculativePipeline

    D, vocab, n_tokens = 32, 512, 240
    cfg = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=2, d_model=4 * D, n_heads=4, n_kv_heads=2, head_dim=D, d_ff=256, vocab=vocab, max_pos=512,
                        rope_theta=500000.0, rope_scaling=LLAMA3, tie_embeddings=False, name="roll-undamped")
    tgt = W.random_init(cfg, seed=1, std=0.1)
    tgt_dev = tgt.to("cuda")
    drf_dev = step_audit.rolled_draft(tgt_dev, 0.25, seed=3)
    eos = vocab - 1
    prompt = torch.randint(4, vocab - 1, (24,), generator=torch.Generator().manual_seed(5)).tolist()
    pipe = SpeculativePipeline(base_lm=HipLM(tgt_dev), draft_lm=HipLM(drf_dev), controller="fixed", controller_params={"k": K}, seed=1234)
    sess = pipe.start_session([prompt], n_tokens, HipSpecDec.EMIT_BONUS, context_window=WINDOW, attention_sinks=SINKS, bad_token_ids=[eos])
    while sess.any_active():
        assert sess.advance()
    sess.finish()
    torch.cuda.synchronize()
    r = sess.rows[0]
    gen = r.seq[r.n_prompt:]
    assert len(gen) >= n_tokens and eos not in gen and len(r.evictions) >= 3, (len(gen), r.evictions)
    lm = OracleLM(tgt, "fp32")

    def outside(rotate):
        rows = RR.replay_logits(lm, prompt, gen, r.evictions, SINKS, tgt.rope_cos, tgt.rope_sin, rotate=rotate, rebuilds=r.rebuilds)
        rows[:, eos] = float("-inf")
        gate = 0.03 * rows[:, :eos].abs().amax(-1)
        mine = rows.gather(1, torch.tensor(gen).view(-1, 1))[:, 0]
        return (mine < rows.amax(-1) - gate)
    out = outside(True)
    first = r.evictions[0][0]
    print(f"[rolling] undamped: {len(gen)} tokens, evictions {r.evictions}, rebuilds {r.rebuilds}, resyncs {sess.stats['resyncs']}, "
          f"outside the gate {int(out.sum())} (after the first eviction {int(out[first:].sum())})")
    defect = outside(False)
    assert int(defect[first:].sum()) > 0.5 * (len(gen) - first), int(defect[first:].sum())
    assert int(out.sum()) <= 0.02 * len(gen), out.nonzero().view(-1).tolist()
    before = [c for c in r.counters if c[2] <= first]
    after = [c for c in r.counters if c[2] > first]
    rate = lambda cs: sum(c[3] for c in cs) / (K * max(len(cs), 1))
    print(f"[rolling] undamped: acceptance {rate(before):.3f} over {len(before)} steps before the first eviction, {rate(after):.3f} over {len(after)} after")
    assert len(after) >= 10 and rate(after) >= 0.5 * rate(before), (rate(before), rate(after))
