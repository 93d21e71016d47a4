"""Confidence-gated draft length on the device (csrc/draft_confidence.hip; sd_draft_confidence, sd_specdec_set_draft_confidence): the op
against the float64 restatement (tests/draft_confidence_ref.py) inside the bound derived there, and the step on the soft synthetic pair
(cases.policy_pair, K = 4): the record's k is the rule applied to the step's own confidences, accept length and emitted tokens follow
from it, the device's k equals the CPU oracle's away from the threshold, the tokens do not depend on k, the pipeline's counters are
those of the record, the mode adds at most two graph nodes per judged forward and none once it is off, and the setter's refusals."""

import math

import numpy as np
import pytest
import torch

import cases
import draft_confidence_ref as R
from helpers import synthetic_prompts
from oracle.model_ref import OracleLM

pytestmark = pytest.mark.gpu

K = 4
STEPS = 24
# Case 3's threshold. The issue names 0.70, unless the oracle alone nearly uses up the 10 % cap there — it does: on the CPU oracle's
# own runs over these prompts 8.9 % of the judged positions sit in row-steps with a margin under 0.01 (17 of 192; the pair's
# confidences hold 8 to 16 values per 0.01 between 0.69 and 0.74). The widest gap between pooled oracle confidences inside [0.6, 0.8]
# is 0.6477 .. 0.6627; its midpoint, to three digits, is the threshold (6 of 432 pooled confidences within 0.01 of it).
TAU_ORACLE = 0.655
DTYPES = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}


# ---------------------------------------------------------------------------------------------------- 1. the op
def _bits(t):
    return t.view(torch.int32).cpu().tolist()


@pytest.mark.parametrize("dtype_name", list(DTYPES))
@pytest.mark.parametrize("V", [1, 7, 160, 1000, 4099, 128256])
def test_op_against_the_restatement(V, dtype_name):
    """Planted rows (exact: NaN-ness, 1, 1/V, 1/n to the bound) and random rows at scales 0.1 and 8, in launches of B = 3 and B = 1,
    contiguous (16-byte aligned rows where V allows) and as a view with row_stride = V + 5 whose rows start 3 elements into the
    buffer's rows. Error bound: the kernel keeps typical_row_kernel's summation shape, so the `p` bound of tests/typical_ref.py
    (draft_confidence_ref.bound). Two runs are bit-identical."""
    from specdec_hip.ops import draft_confidence

    dtype = DTYPES[dtype_name]
    planted = R.planted_rows(V)
    rows = [r for _, r, _ in planted] + list(R.random_rows(2, V, 0.1, 5)) + list(R.random_rows(2, V, 8.0, 6))
    names = [n for n, _, _ in planted] + ["random/0.1"] * 2 + ["random/8"] * 2
    host = torch.from_numpy(np.stack(rows)).to(dtype)                       # the STORED values
    stored = host.to(torch.float64).numpy()
    want = [R.conf(r) for r in stored]
    for (name, _, exact), w in zip(planted, want):                          # the planted expectations survive the rounding
        assert (math.isnan(exact) and math.isnan(w)) or w == pytest.approx(exact, rel=1e-9), name
    N = len(rows)
    wide = torch.zeros((N, V + 5), dtype=dtype)
    wide[:, 3:3 + V] = host
    worst = 0.0
    for layout, dev, aligned in (("contiguous", host.cuda(), True), ("strided", wide.cuda()[:, 3:3 + V], False)):
        assert dev.stride(0) == (V if aligned else V + 5)
        if not aligned:
            assert dev.data_ptr() % 16 != 0                                # (later rows land where V + 5 puts them: some aligned, most not)
        got = torch.empty(N, dtype=torch.float32, device="cuda")
        again = torch.empty_like(got)
        for out in (got, again):
            i = 0
            while i < N:                                                    # launches of B = 3, the tail in launches of B = 1
                n = 3 if i + 3 <= N else 1
                out[i:i + n] = draft_confidence(dev[i:i + n])
                i += n
        torch.cuda.synchronize()
        assert _bits(got) == _bits(again), (layout, "two runs differ")
        for i, (g, w) in enumerate(zip(got.cpu().tolist(), want)):
            if math.isnan(w):
                assert math.isnan(g), (layout, names[i], g)
                continue
            b = R.bound(stored[i], dtype_name, dev[i].data_ptr() % 16 == 0)      # (the walker goes by the row's own address)
            err = abs(g - w) / w
            worst = max(worst, err / b)
            assert err <= b, (layout, names[i], g, w, err, b)
    print(f"[draft_confidence op] V={V} {dtype_name}: worst measured / bound = {worst:.3f}")


def test_op_refusals():
    from specdec_hip import _abi
    from specdec_hip.ops import draft_confidence

    x = torch.zeros((2, 16), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(ValueError, match=r"need logits \[B, V\]"):
        draft_confidence(x[0])
    with pytest.raises(TypeError):
        draft_confidence(x.to(torch.int32))
    with pytest.raises(ValueError, match="out must be"):
        draft_confidence(x, out=torch.zeros(3, device="cuda"))
    lib = _abi.load()
    out = torch.zeros(2, device="cuda")
    assert lib.sd_draft_confidence(x.data_ptr(), _abi.SD_BF16, 8, 2, 16, out.data_ptr(), None) != 0 and "row_stride 8 below V" in _abi.last_error()


# ---------------------------------------------------------------------------------------------------- the step
@pytest.fixture(scope="module")
def pair():
    return cases.policy_pair(torch.bfloat16)


@pytest.fixture(scope="module")
def lms(pair):
    from src.specdec import HipLM

    drf, tgt = pair
    return HipLM(drf.to("cuda")), HipLM(tgt.to("cuda"))


def _pipe(lms, k=K):
    from src.specdec import SpeculativePipeline

    dlm, blm = lms
    return SpeculativePipeline(base_lm=blm, draft_lm=dlm, controller="fixed", controller_params={"k": k}, seed=1234)


def _prompts(B, V):
    return synthetic_prompts(B, 12, V).tolist()


def _device_run(lms, B, tau, min_k, steps=STEPS):
    """`steps` device-advanced steps of the captured step (no host rule touches a row): per step the record and the step's confidences."""
    from specdec_hip.engine import HipSpecDec

    pipe = _pipe(lms)
    prompts = _prompts(B, lms[1].vocab_size)
    kw = {} if tau is None else {"draft_confidence": tau, "draft_min_k": min_k}
    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None, **kw)
    loop = sess.loop
    assert loop.draft_confidence == (None if tau is None else (tau, min_k))
    seqs, out = [list(p) for p in prompts], []
    for _ in range(steps):
        before = [list(s) for s in seqs]
        loop.step(use_graph=True)
        rec = loop.sync()
        conf = None if tau is None else loop.draft_conf.cpu().numpy().copy()
        for b in range(B):
            seqs[b] += [int(x) for x in rec.new_tokens[b][: int(rec.n_new[b])]]
        out.append((before, rec, conf))
    nodes = loop.graph_nodes
    sess.finish()
    return seqs, out, nodes


CASE2 = [(0.85, 1), (0.85, 2), (0.70, 1), (0.70, 2)]       # both thresholds with both min_k
RUNS = CASE2 + [(TAU_ORACLE, 1)]


@pytest.fixture(scope="module")
def runs(lms):
    return {(B, tau, m): _device_run(lms, B, tau, m) for B in (1, 3) for tau, m in RUNS + [(None, 1)]}


def _longest_match(d, t):
    a = 0
    while a < len(d) and d[a] == t[a]:
        a += 1
    return a


@pytest.mark.parametrize("tau,min_k", CASE2)
def test_step_is_consistent_with_its_own_confidences(runs, tau, min_k):
    """For every step and row: record [5+3K] == k_rule(conf_out[b], tau, min_k) exactly (tau as the float the kernel compares with); the
    accept length is min(longest match of the record's draft against its target ids, k); the emitted tokens are target_ids[:a + 1];
    conf_out is a number exactly where a judged forward ran. At least two different k occur per tau."""
    tau32 = float(np.float32(tau))
    seen = set()
    for B in (1, 3):
        _, steps, _ = runs[(B, tau, min_k)]
        for s, (_, rec, conf) in enumerate(steps):
            ks = [int(rec.k_row[b]) for b in range(B)]
            for b in range(B):
                c = [float(x) for x in conf[b]]
                assert ks[b] == R.k_rule(c, tau32, min_k), (B, s, b, ks[b], c)
                d, t = [int(x) for x in rec.draft_tokens[b]], [int(x) for x in rec.target_ids[b]]
                a = int(rec.accept_len[b])
                assert a == min(_longest_match(d[:ks[b]], t), ks[b]), (B, s, b, a, ks[b], d, t)
                assert int(rec.n_new[b]) == a + 1 and [int(x) for x in rec.new_tokens[b][: a + 1]] == t[: a + 1], (B, s, b)
                ran = [j for j in R.judged(K, min_k) if j == min_k - 1 or max(ks) > j]      # forward j > min_k - 1 runs iff some row has k > j
                assert [j for j in range(K) if not math.isnan(c[j])] == ran, (B, s, b, c, ks)
                seen.add(ks[b])
    print(f"[draft_confidence step] tau={tau} min_k={min_k}: k values {sorted(seen)}")
    assert len(seen) >= 2 and min(seen) >= min_k


def test_step_against_the_oracle(runs, pair):
    """The TAU_ORACLE runs: c_i recomputed by OracleLM(draft, "bf16") on the device's own sequence and draft tokens of each step (stateless),
    rounded to the bf16 the forward stores. The oracle's k must equal the device's wherever every margin |c_i - tau| of the row's step is
    >= 0.01; the judged positions of the row-steps left out are at most 10 % of all."""
    drf, _ = pair
    oracle = OracleLM(drf, "bf16")
    left_out = judged = compared = 0
    for B in (1, 3):
        _, steps, _ = runs[(B, TAU_ORACLE, 1)]
        for s, (before, rec, _) in enumerate(steps):
            for b in range(B):
                d = [int(x) for x in rec.draft_tokens[b]]
                lg, _ = oracle.forward(torch.tensor([before[b] + d[: K - 1]]))
                rows = lg[0, len(before[b]) - 1:].to(torch.bfloat16).to(torch.float64).numpy()      # row i: after d_1..d_i
                c = [R.conf(rows[i]) for i in range(K)]
                m = R.margins(c, TAU_ORACLE, 1)
                judged += len(m)
                if min(m) < 0.01:
                    left_out += len(m)
                    continue
                compared += 1
                assert int(rec.k_row[b]) == R.k_rule(c, TAU_ORACLE, 1), (B, s, b, int(rec.k_row[b]), c)
    print(f"[draft_confidence oracle] {compared} row-steps compared, {left_out}/{judged} judged positions left out")
    assert left_out <= 0.10 * judged
    assert compared >= 48


def test_tokens_do_not_depend_on_k(runs):
    for B in (1, 3):
        off, _, _ = runs[(B, None, 1)]
        for tau, m in RUNS:
            on, _, _ = runs[(B, tau, m)]
            for b in range(B):
                n = min(len(on[b]), len(off[b]))
                assert n > 12 + STEPS and on[b][:n] == off[b][:n], (B, tau, m, b)


# ---------------------------------------------------------------------------------------------------- 5. the pipeline
def _rows(results):
    return [(r["generated_tokens"], r["proposed"], r["accepted"]) for r in results]


@pytest.mark.parametrize("early", ["1", "0"])
def test_pipeline(lms, monkeypatch, early):
    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", early)
    V = lms[1].vocab_size
    pipe = _pipe(lms)
    for B in (1, 3):
        prompts = _prompts(B, V)
        plain = pipe.generate_batch(prompts, max_tokens=24)
        never = pipe.generate_batch(prompts, max_tokens=24, draft_confidence=1e-6)          # never stops: the step without the option
        assert _rows(never) == _rows(plain), B
        assert all(r["k_trace"] == [K] * len(r["k_trace"]) for r in never) and "k_trace" not in plain[0]
        assert never[0]["batch_metrics"]["mean_k"] == K and never[0]["batch_metrics"]["draft_forwards_skipped"] == 0
        one = pipe.generate_batch(prompts, max_tokens=24, draft_confidence=1.0)             # always stops at min_k = 1
        k1 = _pipe(lms, k=1).generate_batch(prompts, max_tokens=24)
        assert _rows(one) == _rows(k1), B
        for r in one:
            assert r["k_trace"] == [1] * len(r["k_trace"]) and r["proposed"] == len(r["k_trace"])
        bm = one[0]["batch_metrics"]
        # (K - 1 forwards skipped in every step the host took tokens from: at least one per step of the longest row)
        assert bm["mean_k"] == 1 and bm["draft_forwards_skipped"] % (K - 1) == 0 and bm["draft_forwards_skipped"] >= (K - 1) * bm["total_steps"]
        assert bm["total_steps"] == k1[0]["batch_metrics"]["total_steps"]
        mid = pipe.generate_batch(prompts, max_tokens=24, draft_confidence=0.7)              # in between: the target's greedy tokens all the same
        for a, b in zip(mid, plain):
            n = min(len(a["generated_tokens"]), len(b["generated_tokens"]))
            assert a["generated_tokens"][:n] == b["generated_tokens"][:n] and a["proposed"] == sum(a["k_trace"])


def test_generate_many_admits_without_state(lms):
    """3 prompts through 2 slots (one admission): each result equals that prompt's own single-row run."""
    V = lms[1].vocab_size
    pipe = _pipe(lms)
    prompts = synthetic_prompts(3, 10, V, seed=77).tolist()
    many = pipe.generate_many(prompts, max_tokens=16, batch_size=2, draft_confidence=0.7)
    for p, r in zip(prompts, many):
        own = pipe.generate_batch([p], max_tokens=16, draft_confidence=0.7)[0]
        assert (r["generated_tokens"], r["proposed"], r["accepted"], r["k_trace"]) == \
               (own["generated_tokens"], own["proposed"], own["accepted"], own["k_trace"])


# ---------------------------------------------------------------------------------------------------- 6. launch counts
def test_launch_counts(lms, runs):
    from specdec_hip.engine import HipSpecDec

    for B in (1, 3):
        never = runs[(B, None, 1)][2]
        assert never > 0
        for tau, m in CASE2:
            on = runs[(B, tau, m)][2]
            n_judged = len(R.judged(K, m))
            assert never < on <= never + 2 * n_judged, (B, tau, m, never, on)
        # set, then disable: the graph of the loop that never had the mode
        pipe = _pipe(lms)
        prompts = _prompts(B, lms[1].vocab_size)
        sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None, draft_confidence=0.7)
        loop = sess.loop
        for _ in range(3):
            loop.step(use_graph=True)
        loop.sync()
        assert loop.graph_nodes > never
        loop.set_draft_confidence(None)
        assert loop.graph_nodes == 0          # either call drops the captured step
        for _ in range(3):
            loop.step(use_graph=True)
        rec = loop.sync()
        assert loop.graph_nodes == never and [int(x) for x in rec.k_row] == [K] * B
        sess.finish()


def test_min_k_equal_to_K_judges_nothing(lms, runs):
    """min_k = K is accepted: no forward is judged, no launch is added, every row proposes K, and conf_out reads NaN (the setter fills it)."""
    for B in (1, 3):
        seqs, steps, nodes = _device_run(lms, B, 0.9, K, steps=4)
        assert nodes == runs[(B, None, 1)][2]
        for _, rec, conf in steps:
            assert [int(x) for x in rec.k_row] == [K] * B and np.isnan(conf).all()
        off = runs[(B, None, 1)][0]
        assert all(seqs[b] == off[b][: len(seqs[b])] for b in range(B))


# ---------------------------------------------------------------------------------------------------- 7. refusals through the C ABI
def test_setter_refusals(lms):
    from specdec_hip import _abi
    from specdec_hip.engine import HipSpecDec

    pipe = _pipe(lms)
    prompts = _prompts(2, lms[1].vocab_size)
    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    loop, lib = sess.loop, _abi.load()
    loop.sync()
    for tau in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(_abi.HipLibraryError, match=r"tau .* outside \(0, 1\]"):
            loop.set_draft_confidence(tau)
    for mk in (0, K + 1):
        with pytest.raises(_abi.HipLibraryError, match=r"min_k -?\d+ outside 1\.\.K"):
            loop.set_draft_confidence(0.5, mk)
    need = lib.sd_specdec_draft_confidence_bytes(2, lms[1].vocab_size)
    buf = torch.zeros(need + 32, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for ptr, n, word in ((None, 0, "NULL logits buffer"), (buf.data_ptr(), need - 2, r"logits buffer \d+ B < \d+ B"),
                         (buf.data_ptr() + 2, need, "16-byte aligned")):
        assert lib.sd_specdec_set_draft_confidence(loop.handle, 1, 0.5, 1, ptr, n, None) != 0
        import re
        assert re.search(word, _abi.last_error()), _abi.last_error()
    # while another mode is on
    loop.set_adaptive(True, 2, 1, K)
    with pytest.raises(_abi.HipLibraryError, match="per-row adaptive K is on"):
        loop.set_draft_confidence(0.5)
    loop.set_adaptive(False)
    loop.set_spec_sampling(True, 1.0, 0)
    with pytest.raises(_abi.HipLibraryError, match="speculative sampling is enabled"):
        loop.set_draft_confidence(0.5)
    loop.set_spec_sampling(False)
    loop.set_acceptance("typical")
    with pytest.raises(_abi.HipLibraryError, match="an acceptance rule is on"):
        loop.set_draft_confidence(0.5)
    loop.set_acceptance(None)
    loop.set_logit_processors(True)
    with pytest.raises(_abi.HipLibraryError, match="logit processors / a grammar are on"):
        loop.set_draft_confidence(0.5)
    loop.set_logit_processors(False)
    from specdec_hip.sampling_params import SamplingParams
    loop.set_sampling(True, 0.8, 20, None, 3)
    loop.set_row_sampling([SamplingParams(0.7, 20, seed=1)] * 2)
    with pytest.raises(_abi.HipLibraryError, match="a row-sampling table is bound"):
        loop.set_draft_confidence(0.5)
    loop.set_row_sampling(None)
    loop.set_sampling(False)
    # and the other setters while this one is
    from specdec_hip.grammar import TokenFSM
    loop.set_draft_confidence(0.5, 2)
    fsm = TokenFSM.from_choices([[5, 6, 7], [8, 9]], lms[1].vocab_size, pipe.base_lm.get_tokenizer_info()["eos_token_id"])
    for call, args in ((loop.set_adaptive, (True, 2, 1, K)), (loop.set_spec_sampling, (True, 1.0, 0)), (loop.set_acceptance, ("typical",)),
                       (loop.set_logit_processors, (True,)), (loop.set_grammar, (fsm,))):
        with pytest.raises(_abi.HipLibraryError, match="confidence-gated draft length is on"):
            call(*args)
    loop.set_sampling(True, 0.8, 20, None, 3)         # the sampled-bonus mode stays allowed ...
    with pytest.raises(_abi.HipLibraryError, match="confidence-gated draft length is on"):
        loop.set_row_sampling([SamplingParams(0.7, 20, seed=1)] * 2)      # ... a row table next to it does not
    loop.set_sampling(False)
    loop.set_draft_confidence(None)
    sess.finish()
    # loops without a draft model, and the draft-emit mode
    self_draft = HipSpecDec(None, loop.target, 2, K)
    with pytest.raises(_abi.HipLibraryError, match="needs a draft model"):
        self_draft.set_draft_confidence(0.5)
    self_draft.close()
    emit = HipSpecDec(loop.draft, loop.target, 2, K, HipSpecDec.EMIT_DRAFT)
    with pytest.raises(_abi.HipLibraryError, match="SD_EMIT_DRAFT is not supported"):
        emit.set_draft_confidence(0.5)
    emit.close()
