"""Speculative sampling on the device (csrc/spec_sample.hip) against its CPU restatement (tests/spec_sample_ref.py): the
stand-alone op, the step of HipSpecDec (graph and eager, launch path and persistent draft), and generate_batch with
policy="rejection", policy_params={"backend": "device"}.

Outputs are integers (accept lengths, token ids, counters) and must be EQUAL; the one float output, `ratios`, has a derived
bound (ratio_rtol below). The device's exp / log and its summation order differ from numpy's in the last bits, so a
comparison u < ratio or a Gumbel maximum within rounding of a tie could legitimately differ. Such a case may be excused only
if the restatement itself reports a margin below CAP = 1e-9 — and every test first asserts that the restatement reports
ZERO such cases for its inputs (fixed seeds), so nothing is ever excused."""

import numpy as np
import pytest
import torch

import spec_sample_ref as R
from helpers import synthetic_prompts, tiny_pair
from oracle import sampling_ref as S
from oracle.model_ref import OracleLM
from specdec_hip import weights as W

pytestmark = pytest.mark.gpu

CAP = 1e-9


def ratio_rtol(V: int) -> float:
    """Relative bound on ratio_i = exp(A), A = (p_d/T - lse p) - (q_d/T - lse q), device against numpy, both float64
    (u = 2^-53). Both sides form x/T, the row maxima and the arguments x/T - max with the same IEEE operations, so they differ
    only in (a) exp / log being faithful rather than correctly rounded: <= 2u relative per call, and (b) the order in which
    the V terms of S = sum exp(.) are added: each side's sum carries a relative error <= (V - 1) u whatever its order (every
    term is positive, so the condition number of the sum is 1). Hence |dS / S| <= 2 (V - 1) u + 4u between the two sides,
    |d lse| <= that + 4u (log, one addition, lse of size < 2^6), |dA| <= 2 |d lse| + 8u (four more roundings of terms below
    2^7, i.e. absolute 2^7 u each — counted as 1024u), and d ratio / ratio = |dA| + 2u to first order:
        rtol = (4 V + 2048) u     -> 5.7e-11 at V = 128256, 2.3e-11 at V = 50257.
    The observed difference is far smaller (the errors of a sum behave like sqrt(V) u): the bound is what is asserted."""
    return (4 * V + 2048) * 2.0 ** -53


def _bf16(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16)


def _op_case(V, K, B, T, seed):
    """Rows built for a known accept length j = b mod (K + 1) (B = 1: j = K): q_i = p_i bitwise for i < j (ratio exactly 1,
    always accepted), q_j has a 30-logit spike on a token the target finds unlikely (drawn almost surely, ratio ~ e^-30);
    rows past the first K + 1 are 0.5-noise neighbours of p with whatever accept length the draws give."""
    rng = np.random.default_rng(seed)
    p = _bf16(rng.normal(0, 3.0, (B, K + 1, V))).float().numpy()
    q = p[:, :K].copy()
    want_len = []
    for b in range(B):
        j = K if B == 1 else b % (K + 1)
        if b >= K + 1:
            q[b] = _bf16(p[b, :K] + rng.normal(0, 0.5, (K, V))).float().numpy()
            want_len.append(None)
            continue
        if j < K:
            tok = int(np.argmin(p[b, j]))
            q[b, j, tok] = _bf16(np.float32(p[b, j].max() + 30.0)).item()
        want_len.append(j)
    return p, q, want_len


@pytest.mark.parametrize("V", [128256, 50257])
@pytest.mark.parametrize("K", [1, 4, 8])
def test_op_matches_restatement(V, K):
    from specdec_hip.ops import spec_sample_accept_hip

    seen = set()
    for B in (1, 8):
        for ti, T in enumerate((0.7, 1.0, 1.5)):
            seed = 1000 * K + 10 * B + ti
            p, q, want_len = _op_case(V, K, B, T, seed)
            counters = [17 * b + 3 for b in range(B)]
            sids = [b + 2 for b in range(B)]
            d = np.array([[R.draft_draw_ref(q[b, i], T, seed, counters[b], i, sids[b]) for i in range(K)] for b in range(B)], dtype=np.int32)
            want = [R.spec_accept_ref(q[b], p[b], d[b], T, seed, counters[b], sids[b]) for b in range(B)]
            # the excuse cap: the restatement alone reports no decision within 1e-9 of a tie for these seeds
            assert sum(w.close_calls(CAP) for w in want) == 0, (V, K, B, T)
            for b in range(B):
                if want_len[b] is not None:
                    assert want[b].accept_len == want_len[b], (V, K, B, T, b)
            ctr = torch.tensor(counters, dtype=torch.int32, device="cuda")
            acc, nxt, ratios = spec_sample_accept_hip(
                _bf16(q).cuda(), _bf16(p).cuda(), torch.from_numpy(d).cuda(), T, seed=seed, draw_counters=ctr,
                stream_ids=torch.tensor(sids, dtype=torch.int32, device="cuda"), return_ratios=True)
            assert acc.cpu().tolist() == [w.accept_len for w in want], (V, K, B, T)
            assert nxt.cpu().tolist() == [w.next_tok for w in want], (V, K, B, T)
            assert ctr.cpu().tolist() == [c + K + 1 for c in counters]
            got_r, want_r = ratios.cpu().numpy(), np.stack([w.ratios for w in want])
            rel = np.abs(got_r - want_r) / np.maximum(want_r, np.finfo(np.float64).tiny)
            print(f"[spec op] V={V} K={K} B={B} T={T}: max relative ratio difference {rel.max():.3e} (bound {ratio_rtol(V):.3e})")
            assert (rel <= ratio_rtol(V)).all(), (V, K, B, T, rel.max())
            for b in range(B):   # q bitwise equal to p: ratio exactly 1 on the device too
                for i in range(K):
                    if np.array_equal(q[b, i], p[b, i]):
                        assert got_r[b, i] == 1.0
            seen |= {w.accept_len for w in want}
    assert seen == set(range(K + 1)), seen


def test_op_draw0_inactive_rows_non_finite_and_refusals():
    from specdec_hip import _abi
    from specdec_hip.ops import spec_sample_accept_hip

    V, K, B, T, seed = 4099, 3, 4, 1.5, 77      # V not a multiple of 8: the scalar row walk
    rng = np.random.default_rng(3)
    p = _bf16(rng.normal(0, 2, (B, K + 1, V))).float().numpy()
    q = _bf16(p[:, :K] + rng.normal(0, 1.0, (B, K, V))).float().numpy()
    p[1, 0, 7] = np.nan            # position 0 of row 1: rejected, redrawn from p with NaN first
    q[2, 1, 9] = np.inf            # position 1 of row 2: rejected
    p[3, 0, 5] = -np.inf           # a -inf entry of a finite row: probability 0, no special case
    d = np.array([[R.draft_draw_ref(q[b, i], T, seed, 40, i, b) for i in range(K)] for b in range(B)], dtype=np.int32)
    want = [R.spec_accept_ref(q[b], p[b], d[b], T, seed, 40, b) for b in range(B)]
    assert sum(w.close_calls(CAP) for w in want) == 0
    assert want[1].accept_len == 0 and want[1].next_tok == 7 and want[2].accept_len <= 1
    active = torch.tensor([1, 1, 1, 1], dtype=torch.int32, device="cuda")
    acc, nxt, ratios = spec_sample_accept_hip(_bf16(q).cuda(), _bf16(p).cuda(), torch.from_numpy(d).cuda(), T, seed=seed, draw=40,
                                              active=active, return_ratios=True)
    assert acc.cpu().tolist() == [w.accept_len for w in want] and nxt.cpu().tolist() == [w.next_tok for w in want]
    r = ratios.cpu().numpy()
    assert np.isnan(r[1, 0]) and np.isnan(r[2, 1]) and not np.isnan(r[0]).any()
    # inactive rows: accept length 0, nothing else written, no draws consumed
    active = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device="cuda")
    ctr = torch.full((B,), 40, dtype=torch.int32, device="cuda")
    acc2, nxt2 = spec_sample_accept_hip(_bf16(q).cuda(), _bf16(p).cuda(), torch.from_numpy(d).cuda(), T, seed=seed, draw_counters=ctr, active=active)
    assert acc2.cpu().tolist() == [want[0].accept_len, 0, want[2].accept_len, 0]
    assert nxt2.cpu().tolist() == [want[0].next_tok, -1, want[2].next_tok, -1]
    assert ctr.cpu().tolist() == [40 + K + 1, 40, 40 + K + 1, 40]
    for bad_t in (0.0, -1.0, float("nan")):
        with pytest.raises(_abi.HipLibraryError, match="temperature"):
            spec_sample_accept_hip(_bf16(q).cuda(), _bf16(p).cuda(), torch.from_numpy(d).cuda(), bad_t)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        spec_sample_accept_hip(_bf16(q), _bf16(p), torch.from_numpy(d), T)


# ------------------------------------------------------------------------------------------------------- the step
SEL_TGT = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=3, d_model=256, n_heads=4, n_kv_heads=2, head_dim=64, d_ff=512,
                        vocab=2048, max_pos=1024, rope_theta=500000.0, tie_embeddings=False, name="select-target")
SEL_DRF = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=2, d_model=256, n_heads=4, n_kv_heads=1, head_dim=64, d_ff=512,
                        vocab=2048, max_pos=1024, rope_theta=500000.0, tie_embeddings=False, name="select-draft")


def _persist_pair(flip=0.3):
    """a pair whose draft is eligible for the persistent launch (and, one row, the device-selected forward 0)"""
    tgt = W.synthetic_llama(SEL_TGT, seed=0, device="cpu", layer_gain=0.05)
    drf = W.synthetic_llama(SEL_DRF, seed=1, device="cpu", layer_gain=0.05, embed_from=tgt, flip_fraction=flip)
    return drf, tgt


def _pipe(drf, tgt, k=4, policy="longest_prefix", policy_params=None, eos=None, **lm_kw):
    """eos: the EOS id of the pipeline's tokenizer (default: the synthetic tokenizer's, vocab - 1)"""
    from src.specdec import HipLM, SpeculativePipeline
    from src.specdec.models.hip_lm import IdTokenizer

    tok = IdTokenizer(tgt.config.vocab, eos_token_id=eos) if eos is not None else None
    return SpeculativePipeline(base_lm=HipLM(tgt.to("cuda"), tokenizer=tok, **lm_kw), draft_lm=HipLM(drf.to("cuda"), **lm_kw), controller="fixed",
                               controller_params={"k": k}, seed=1234, policy=policy, policy_params=policy_params)


def _device_steps(pipe, prompts, K, T, seed, n_steps, use_graph, counters0=None):
    """n_steps of the loop in the new mode, the device advancing its own state (no host rule touches a row). Every step is
    checked against the restatement applied to THE DEVICE'S OWN stored logits; returns the per-step records."""
    from specdec_hip.engine import HipSpecDec

    B = len(prompts)
    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    loop = sess.loop
    counters = list(counters0) if counters0 else [5 * b for b in range(B)]
    loop.sync()
    loop.set_spec_sampling(True, T, seed, stream_ids=list(range(B)), draw_counts=counters)
    cur_len = [len(p) - 1 for p in prompts]
    out, close = [], 0
    for step in range(n_steps):
        loop.step(use_graph=use_graph)
        rec = loop.sync()
        q = loop.spec_draft_logits.float().cpu().numpy()
        p = loop.step_logits.float().cpu().numpy()
        for b in range(B):
            d, res, emitted, c2 = R.spec_step_ref(q[b], p[b], T, seed, counters[b], b)
            close += res.close_calls(CAP)
            assert [int(x) for x in rec.draft_tokens[b]] == d, (step, b)                 # the draft ids ARE the Gumbel draws of q_i
            assert int(rec.accept_len[b]) == res.accept_len, (step, b, res.ratios)
            assert int(rec.n_new[b]) == len(emitted)
            assert [int(x) for x in rec.new_tokens[b]] == emitted + [-1] * (K + 1 - len(emitted)), (step, b)
            assert [int(x) for x in rec.target_ids[b]] == [int(np.argmax(p[b, i])) for i in range(K + 1)], (step, b)
            cur_len[b] += len(emitted)
            assert int(rec.cur_len[b]) == cur_len[b], (step, b)
            counters[b] = c2
            out.append((b, d, res.accept_len, emitted))
        assert loop.draw_counts == counters, step
    assert close == 0    # (checked after the fact here: the inputs are the device's own logits)
    loop.set_spec_sampling(False)
    sess.finish()
    return out


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("use_graph", [True, False])
def test_step_reproduces_restatement_on_its_own_logits(B, use_graph):
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(B, 12, tgt.config.vocab).tolist()
    out = _device_steps(_pipe(drf, tgt), prompts, 4, 20.0, 4321, 14, use_graph)
    lens = [a for _, _, a, _ in out]
    print(f"[spec step] B={B} graph={use_graph}: accept lengths {sorted(set(lens))}, mean {np.mean(lens):.2f}")
    assert len(set(lens)) >= 2, lens     # the run exercises accepted and rejected positions


def test_persistent_draft_and_launch_path_give_the_same_kind_of_records(monkeypatch):
    """One row, a draft served by persistent launches (both forms of draft forward 0, device-picked) and the same run with
    SPECDEC_PERSIST_MAX_T=0 (launch path, 2-token forward 0 only): each is checked step by step against the restatement on
    its own stored logits, with the same seed and counters."""
    drf, tgt = _persist_pair()
    prompts = synthetic_prompts(1, 9, SEL_TGT.vocab, seed=3).tolist()
    pipe = _pipe(drf, tgt)
    a = _device_steps(pipe, prompts, 4, 6.0, 99, 14, True)
    assert pipe._runtimes and all(rt["draft"].persist_tokens >= 2 for rt in pipe._runtimes.values()), "the draft must be on the persistent launch"
    monkeypatch.setenv("SPECDEC_PERSIST_MAX_T", "0")
    pipe0 = _pipe(drf, tgt)
    _device_steps(pipe0, prompts, 4, 6.0, 99, 14, True)
    assert all(rt["draft"].persist_tokens == 0 for rt in pipe0._runtimes.values())
    monkeypatch.delenv("SPECDEC_PERSIST_MAX_T")
    lens = [x[2] for x in a]
    assert 4 in lens and min(lens) < 4, lens     # full acceptances (2-token forward 0 next) and rejections (1-token form)


@pytest.mark.parametrize("lm_kw", [{"weight_dtype": "fp8"}, {"kv_page_len": 64}], ids=["fp8", "paged64"])
def test_step_under_fp8_storage_and_paged_kv(lm_kw):
    """fp8 weight storage and paged KV (64-position pages): draws, ratios, accept lengths, hand-over and counters of every step
    equal the restatement on the device's own stored logits, as for bf16 / dense."""
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(3, 12, tgt.config.vocab).tolist()
    out = _device_steps(_pipe(drf, tgt, **lm_kw), prompts, 4, 20.0, 77, 12, True)
    assert len({a for _, _, a, _ in out}) >= 2


def test_enable_then_disable_returns_to_the_greedy_records():
    from specdec_hip.engine import HipSpecDec

    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(2, 12, tgt.config.vocab).tolist()

    def greedy_records(pipe, n):
        sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
        recs = []
        for _ in range(n):
            sess.loop.step(use_graph=True)
            r = sess.loop.sync()
            recs.append((r.accept_len.tolist(), r.new_tokens.tolist(), r.draft_tokens.tolist(), r.target_ids.tolist(), r.cur_len.tolist()))
        sess.finish()
        return recs

    never = greedy_records(_pipe(drf, tgt), 8)
    pipe = _pipe(drf, tgt)
    _device_steps(pipe, prompts, 4, 20.0, 1, 4, True)
    assert greedy_records(pipe, 8) == never


# ------------------------------------------------------------------------------------------------------- the pipeline
def _gen(pipe, prompts, n, **kw):
    return [r["generated_tokens"] for r in pipe.generate_batch(prompts, max_tokens=n, **kw)]


def test_pipeline_device_backend_against_oracle_replay(monkeypatch):
    """generate_batch(policy="rejection", backend="device") replayed by the CPU: OracleLM (bf16) forwards give the oracle's
    q_i and p_i for the step's inputs, the restatement decides on them with the same seed and counters. The device's decisions
    come from ITS logits, which differ from the oracle's by the bf16 forward error, so the comparison follows the divergence
    discipline of tests/test_hip_fulldepth_parity_gpu.py with its band: a step may differ only if a decision of the oracle
    sits within 6 x the measured RMS logit error — each step's error first asserted under the suite's 3 % max / 1.5 % RMS logits bound — (here in
    units of logit / T: |log u - log ratio| of a flag, the score gap of a
    draw), and the comparison ends there. The steps run one at a time (SPECDEC_EARLY_LAUNCH=0) so that the stored logits
    of every step can be read for the error measurement."""
    from specdec_hip.engine import HipSpecDec

    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", "0")
    drf, tgt = tiny_pair(flip_fraction=0.25)
    K, T, seed, V = 4, 20.0, 2024, tgt.config.vocab
    prompts = synthetic_prompts(2, 12, V).tolist()
    pipe = _pipe(drf, tgt, K, "rejection", {"backend": "device", "temperature": T, "seed": seed})
    sess = pipe.start_session(prompts, 24, HipSpecDec.EMIT_BONUS, pipe._spec_sampling_config({}))
    o_t, o_d = OracleLM(tgt, "bf16"), OracleLM(drf, "bf16")
    compared = diverged = 0
    sq, n_el = 0.0, 0
    while sess.any_active() and not diverged:
        before = [(list(r.seq), r.draws, r.active) for r in sess.rows]
        assert sess.advance()
        rec = sess.last_record
        q_dev = sess.loop.spec_draft_logits.float().cpu().numpy()
        p_dev = sess.loop.step_logits.float().cpu().numpy()
        for b, (seq, c, active) in enumerate(before):
            if not active:
                continue
            d_dev = [int(x) for x in rec.draft_tokens[b]]
            n0 = len(seq) - 1
            p_or = o_t.forward(torch.tensor([seq + d_dev], dtype=torch.int64))[0][0, n0:n0 + K + 1].float().numpy()
            q_or = o_d.forward(torch.tensor([seq + d_dev[:K - 1]], dtype=torch.int64))[0][0, n0:n0 + K].float().numpy()
            # the error that becomes the band is first held to the suite's logits bound against the bf16 oracle
            # (tests/test_hip_fullshape_parity_gpu.py: max |got - want| < 3 % of max |want|, RMS(got - want) < 1.5 % of RMS(want)),
            # every step, both models: a device forward that is off fails here instead of widening its own excuse
            for what, dev, orc in (("target", p_dev[b], p_or), ("draft", q_dev[b], q_or)):
                diff = (dev - orc).astype(np.float64)
                e_max = float(np.abs(diff).max() / np.abs(orc).max())
                e_rms = float(np.sqrt((diff ** 2).mean()) / np.sqrt((orc.astype(np.float64) ** 2).mean()))
                assert e_max < 0.03 and e_rms < 0.015, (what, b, e_max, e_rms)
            sq += float(((p_dev[b] - p_or) ** 2).sum() + ((q_dev[b] - q_or) ** 2).sum())
            n_el += p_or.size + q_or.size
            band = 6 * np.sqrt(sq / n_el) / T
            d_or, res, emitted, _ = R.spec_step_ref(q_or, p_or, T, seed, c, b)
            got = [int(x) for x in rec.new_tokens[b][: int(rec.n_new[b])]]
            if d_or == d_dev and emitted == got:
                compared += 1
                assert sess.rows[b].draws == c + K + 1
                continue
            # the oracle's smallest decision margin in this step, in logit / T units
            gaps = [R.best_of(R.scaled(q_or[i], T) + R.gumbel_noise(V, seed, c + i, b))[1] for i in range(K)]
            flags = [abs(np.log(max(x.u, 1e-300)) - np.log(max(x.ratio, 1e-300))) for x in res.positions[:-1]]
            margin = min(gaps + flags + [x.gap for x in res.positions])
            print(f"[spec pipeline] first divergence after {compared} equal row-steps: oracle margin {margin:.4f}, band {band:.4f}")
            assert margin <= band, (b, margin, band, d_or, d_dev, emitted, got)
            diverged = 1
            break
    sess.finish()
    print(f"[spec pipeline] {compared} row-steps equal to the oracle replay; rms logit error {np.sqrt(sq / max(n_el, 1)):.4f}")
    assert compared >= 4


def test_pipeline_modes_cuts_and_refusals(monkeypatch):
    from src.specdec import HipLM, SpeculativePipeline

    drf, tgt = tiny_pair(flip_fraction=0.25)
    V = tgt.config.vocab
    prompts = synthetic_prompts(3, 12, V).tolist()
    pp = {"backend": "device", "temperature": 20.0, "seed": 7}
    pipe = _pipe(drf, tgt, 4, "rejection", pp)
    eos = pipe.base_lm.get_tokenizer_info()["eos_token_id"]
    assert eos == V - 1
    first = pipe.generate_batch(prompts, max_tokens=24)
    toks = [r["generated_tokens"] for r in first]
    # the budget: a row ends at the step that reaches max_tokens (generate_batch does not truncate). No row of this run meets
    # the EOS (asserted, so the bound below is not conditional); the EOS cuts have a test of their own below
    for r in first:
        g = r["generated_tokens"]
        assert eos not in g and all(0 <= t < V for t in g)
        assert 24 <= len(g) <= 24 + 4, len(g)
    # reproducible per seed (steps queued ahead included), another seed draws differently
    assert _gen(pipe, prompts, 24) == toks
    assert _gen(pipe, prompts, 24, seed=8) != toks
    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", "0")
    assert _gen(_pipe(drf, tgt, 4, "rejection", pp), prompts, 24) == toks       # launch -> wait -> rules order: the same tokens
    monkeypatch.delenv("SPECDEC_EARLY_LAUNCH")
    # the cached loop returns to greedy afterwards, and the host backend is still the host loop
    greedy = _gen(_pipe(drf, tgt, 4), prompts, 24, do_sample=False)
    pipe.policy_name, pipe.rejection_backend = "longest_prefix", "host"
    assert _gen(pipe, prompts, 24, do_sample=False) == greedy
    # fp8 weight storage and paged KV through the pipeline, once each: reproducible (the step itself is pinned against the
    # restatement under both in test_step_under_fp8_storage_and_paged_kv)
    for kw in ({"weight_dtype": "fp8"}, {"kv_page_len": 64}):
        a = _gen(_pipe(drf, tgt, 4, "rejection", pp, **kw), prompts, 16)
        assert a == _gen(_pipe(drf, tgt, 4, "rejection", pp, **kw), prompts, 16) and all(len(x) >= 16 or eos in x[-2:] for x in a), kw
    # ---- refusals
    with pytest.raises(NotImplementedError, match="generate_batch policy"):
        pipe2 = _pipe(drf, tgt, 4, "rejection", pp)
        pipe2.generate(prompts[0], max_tokens=8)
    with pytest.raises(NotImplementedError, match="top-k / top-p"):
        pipe2.generate_batch(prompts, max_tokens=8, top_k=50)
    with pytest.raises(NotImplementedError, match="top-k / top-p"):
        pipe2.generate_batch(prompts, max_tokens=8, top_p=0.9)
    with pytest.raises(ValueError, match="backend"):
        _pipe(drf, tgt, 4, "rejection", {"backend": "gpu"})
    with pytest.raises(ValueError, match="temperature"):
        _pipe(drf, tgt, 4, "rejection", {"backend": "device", "temperature": 0.0})
    with pytest.raises(ValueError, match="rejection"):
        _pipe(drf, tgt, 4, "longest_prefix", {"backend": "device"})
    adaptive = SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=HipLM(drf.to("cuda")), controller="adaptive", seed=1,
                                   policy="rejection", policy_params=pp)
    with pytest.raises(NotImplementedError, match="fixed K"):
        adaptive.generate_batch(prompts, max_tokens=8)
    with pytest.raises(NotImplementedError):
        SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=None, draft_model="none", draft_mode="medusa", policy="rejection", policy_params=pp)


def _trace(pipe, prompt, max_tokens):
    """One row through DecodeSession.advance in the new mode: per step (accept length, tokens the device emitted, generated
    before, generated after, sequence's last token before, active after, host draws after, rows flagged by the step)."""
    from specdec_hip.engine import HipSpecDec

    sess = pipe.start_session([prompt], max_tokens, HipSpecDec.EMIT_BONUS, pipe._spec_sampling_config({}))
    steps = []
    while sess.any_active():
        r = sess.rows[0]
        gen0, last0 = list(r.generated), r.seq[-1]
        assert sess.advance()
        rec, r = sess.last_record, sess.rows[0]
        steps.append((int(rec.accept_len[0]), [int(x) for x in rec.new_tokens[0][: int(rec.n_new[0])]], gen0, list(r.generated), last0,
                      r.active, r.draws, dict(sess._flagged)))
    sess.finish()
    return steps, sess


@pytest.mark.parametrize("early", ["0", "1"], ids=["in-order", "queued-ahead"])
def test_eos_cuts_in_the_new_mode(early, monkeypatch):
    """The EOS rules of generate_batch under speculative sampling, forced: a baseline run (EOS = vocab - 1, never drawn) gives
    the steps; each case then re-runs the same seed with the tokenizer's EOS set to a token of a chosen step — the run is the
    same up to that step (the EOS only acts in the host rules), where the rule must produce exactly:
      accepted draft EOS, a < K : the accepted tokens before the EOS + the token redrawn after the accepted prefix (the rule
                                  as it stands for greedy steps: it cuts before the EOS and appends t[a]); the row stops;
      accepted draft EOS, a == K: the accepted tokens before the EOS + the EOS; the row stops;
      redrawn / bonus EOS, a >= 1: the accepted tokens + the EOS; the row stops;
      redrawn EOS, a == 0        : nothing is emitted (the zero-accept rule drops it); the row stops.
    In every case the row is frozen on the device, the host has counted (steps so far) x (K + 1) draws, and after the session
    the device's counter equals the host's (steps queued ahead drew for the stopped row and are written back).
    Steps whose emitted tokens overlap the generated tail (the de-duplication rules) are not eligible as cases."""
    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", early)
    drf, tgt = tiny_pair(flip_fraction=0.25)
    K, V = 4, tgt.config.vocab
    pp = {"backend": "device", "temperature": 20.0, "seed": 31}
    prompt = synthetic_prompts(1, 12, V)[0].tolist()
    base, sess = _trace(_pipe(drf, tgt, K, "rejection", pp), prompt, 48)
    assert sess.eos == V - 1 and all(V - 1 not in new for _, new, *_ in base)
    gen = base[-1][3]
    assert 48 <= len(gen) <= 48 + K and not base[-1][5]                   # the budget stop: the step that reaches max_tokens
    assert [s[6] for s in base] == [(i + 1) * (K + 1) for i in range(len(base))]

    def fresh(i, tok):      # the token has not been emitted before step i, and step i's tokens do not overlap the tail
        return all(tok not in new for _, new, *_ in base[:i]) and base[i][4] not in base[i][1] and tok not in prompt

    def pick(cond):
        for i, (a, new, *_rest) in enumerate(base):
            j = cond(a, new)
            if j is not None and fresh(i, new[j]) and new.count(new[j]) == 1:
                return i, j
        raise AssertionError(f"no eligible step in the baseline run: {[(a, new) for a, new, *_ in base]}")

    cases = {
        "accepted a<K": pick(lambda a, new: 0 if 1 <= a < K else None),
        "accepted a==K": pick(lambda a, new: 1 if a == K else None),
        "next token a>=1": pick(lambda a, new: a if a >= 1 else None),
        "next token a==0": pick(lambda a, new: 0 if a == 0 else None),
    }
    for name, (i, j) in cases.items():
        a, new, gen0 = base[i][0], base[i][1], base[i][2]
        eos = new[j]
        if j < a:
            want = new[:j] + ([new[a]] if a < K else [eos])
        else:
            want = new[:a] + [eos] if a >= 1 else []
        steps, sess = _trace(_pipe(drf, tgt, K, "rejection", pp, eos=eos), prompt, 48)
        assert sess.eos == eos
        assert len(steps) == i + 1, (name, len(steps), i)
        assert [(s[0], s[1]) for s in steps] == [(s[0], s[1]) for s in base[: i + 1]], name       # the same run up to the cut
        assert steps[i][3] == gen0 + want, (name, steps[i][3][len(gen0):], want)
        assert steps[i][5] is False and steps[i][7] == {0: "freeze"}, name
        assert sess.rows[0].draws == (i + 1) * (K + 1)
        assert sess.loop.draw_counts == [sess.rows[0].draws], name
        got = _gen(_pipe(drf, tgt, K, "rejection", pp, eos=eos), [prompt], 48)[0]                     # generate_batch itself
        assert got == gen0 + want, name


def test_draft_equal_to_target_accepts_everything(monkeypatch):
    """draft == target (one row: the draft's 1- and 2-token passes and the 5-token verify pass run the same kernels): the stored
    q_i and p_i agree, every ratio is 1 up to the derived bound, every proposal is accepted."""
    from specdec_hip.engine import HipSpecDec

    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", "0")
    _, tgt = tiny_pair(flip_fraction=0.25)
    K, T, seed = 4, 20.0, 5
    prompts = synthetic_prompts(1, 12, tgt.config.vocab).tolist()
    pipe = _pipe(tgt, tgt, K, "rejection", {"backend": "device", "temperature": T, "seed": seed})
    sess = pipe.start_session(prompts, 30, HipSpecDec.EMIT_BONUS, pipe._spec_sampling_config({}))
    steps = 0
    while sess.any_active() and steps < 6:
        c = sess.rows[0].draws
        assert sess.advance()
        rec = sess.last_record
        q = sess.loop.spec_draft_logits.float().cpu().numpy()[0]
        p = sess.loop.step_logits.float().cpu().numpy()[0]
        d = [int(x) for x in rec.draft_tokens[0]]
        res = R.spec_accept_ref(q, p, d, T, seed, c, 0)
        print(f"[spec same] step {steps}: ratios {res.ratios.tolist()}, q == p bitwise: {[bool(np.array_equal(q[i], p[i])) for i in range(K)]}")
        assert (np.abs(res.ratios - 1.0) <= ratio_rtol(tgt.config.vocab)).all(), res.ratios
        assert int(rec.accept_len[0]) == K
        steps += 1
    sess.finish()
    assert steps >= 4


def test_engine_refusals():
    from specdec_hip import _abi
    from specdec_hip.engine import HipModel, HipSpecDec

    drf, tgt = tiny_pair(flip_fraction=0.25)
    t, d = HipModel(tgt.to("cuda"), batch=2, l_max=128), HipModel(drf.to("cuda"), batch=2, l_max=128)
    for loop, msg in ((HipSpecDec(d, t, 2, 4, HipSpecDec.EMIT_DRAFT), "SD_EMIT_DRAFT"), (HipSpecDec(None, t, 2, 4, HipSpecDec.EMIT_BONUS), "draft model")):
        with pytest.raises(_abi.HipLibraryError, match=msg):
            loop.set_spec_sampling(True, 1.0, 1)
    loop = HipSpecDec(d, t, 2, 4, HipSpecDec.EMIT_BONUS)
    for bad in (0.0, -2.0, float("nan")):
        with pytest.raises(_abi.HipLibraryError, match="temperature"):
            loop.set_spec_sampling(True, bad, 1)
    loop.set_adaptive(True, 2, 1, 4)
    with pytest.raises(_abi.HipLibraryError, match="adaptive"):
        loop.set_spec_sampling(True, 1.0, 1)
    loop.set_adaptive(False)
    loop.set_sampling(True, 1.0, 50, 0.9, 1)
    with pytest.raises(_abi.HipLibraryError, match="mutually exclusive"):
        loop.set_spec_sampling(True, 1.0, 1)
    loop.set_sampling(False)
    loop.set_spec_sampling(True, 1.0, 1)
    with pytest.raises(_abi.HipLibraryError, match="mutually exclusive"):
        loop.set_sampling(True, 1.0, 50, 0.9, 1)
    with pytest.raises(_abi.HipLibraryError, match="fixed K"):
        loop.set_adaptive(True, 2, 1, 4)
    V = tgt.config.vocab
    buf = torch.empty(2 * 4 * V, dtype=torch.bfloat16, device="cuda")       # one row short for the target's [B][K+1][V]
    rc = loop.lib.sd_specdec_set_spec_sampling(loop.handle, 1, 1.0, 1, buf.data_ptr(), buf.numel() * 2, buf.data_ptr(), buf.numel() * 2,
                                               loop._draw.data_ptr(), None)
    assert rc != 0 and "target logits buffer" in _abi.last_error()
    big = torch.empty(2 * 5 * V + 8, dtype=torch.bfloat16, device="cuda")
    rc = loop.lib.sd_specdec_set_spec_sampling(loop.handle, 1, 1.0, 1, buf.data_ptr(), (2 * 4 * V - 1) * 2, big.data_ptr(), 2 * 5 * V * 2,
                                               loop._draw.data_ptr(), None)
    assert rc != 0 and "draft logits buffer" in _abi.last_error()
    for q_off, p_off in ((2, 0), (0, 2)):       # a buffer 2 bytes off a 16-byte boundary
        rc = loop.lib.sd_specdec_set_spec_sampling(loop.handle, 1, 1.0, 1, big.data_ptr() + q_off, 2 * 4 * V * 2, big.data_ptr() + p_off,
                                                   2 * 5 * V * 2, loop._draw.data_ptr(), None)
        assert rc != 0 and "16-byte aligned" in _abi.last_error()
    rc = loop.lib.sd_specdec_set_spec_sampling(loop.handle, 1, 1.0, 1, None, 0, big.data_ptr(), 2 * 5 * V * 2, loop._draw.data_ptr(), None)
    assert rc != 0 and "NULL" in _abi.last_error()
    loop.set_spec_sampling(False)
