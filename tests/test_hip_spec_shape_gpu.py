"""Top-k / top-p shaped speculative sampling on the device (csrc/spec_sample.hip: spec_draft_draw_shaped_kernel,
spec_stats_shaped_kernel) against its CPU restatement (tests/spec_shape_ref.py): the stand-alone op, the step of HipSpecDec and
generate_batch with policy="rejection", policy_params={"backend": "device", "top_k": .., "top_p": ..}.

Outputs are integers (accept lengths, token ids, counters) and must be EQUAL; the one float output, `ratios`, has a derived
bound (ratio_rtol below). The device's exp differs from numpy's in the last bits, so a comparison within rounding of a tie (a
flag u < ratio, an inversion boundary, the nucleus cut) could legitimately differ. Such a case may be excused only if the
restatement itself reports a margin below CAP = 1e-9 — and every test first asserts that the restatement reports ZERO such
cases for its inputs (fixed seeds), so nothing is ever excused."""

import numpy as np
import pytest
import torch

import spec_shape_ref as R
from helpers import synthetic_prompts, tiny_pair
from specdec_hip import weights as W

pytestmark = pytest.mark.gpu

CAP = 1e-9
SHAPES = [(50, 0.9), (1, 1.0), (1024, 1.0), (40, 0.5)]


def ratio_rtol(n: int) -> float:
    """Relative bound on ratio = (e_p(d)/Z_p) / (e_q(d)/Z_q), device against numpy, both float64 (u = 2^-53), n = the number of
    summed terms of a Z (kept-set size <= top_k). Both sides form x/T, the maximum and the arguments x/T - max with the same
    IEEE operations and add the SAME terms in the SAME sequential order, so they differ only in (a) exp being faithful rather
    than correctly rounded: <= 2u relative per call and side, 4u between the sides, for e_p(d), e_q(d) and every term of a sum;
    (b) the additions of a sum rounding differently because their inputs differ: each side's sum carries <= (n - 1) u whatever
    the inputs (positive terms, condition number 1), so |dZ/Z| <= 4u + 2 (n - 1) u for each of Z_p, Z_q; (c) three divisions,
    u per side each: 6u. First order: 4u + 4u + 2 (4u + 2 (n - 1) u) + 6u = (4 n + 18) u, asserted as
        rtol = (4 n + 32) u     (the second-order terms rounded up)   -> 2.6e-14 at n = 50, 4.6e-13 at n = 1024.
    This is ratio_rtol of tests/test_hip_spec_sample_gpu.py with n in place of V, the divisions counted and without the
    log-sum-exp terms that formula carries. The observed difference is printed next to it."""
    return (4 * n + 32) * 2.0 ** -53


def _bf16(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16)


def _op_case(V, K, B, seed):
    """Rows built for a known accept length j = b mod (K + 1) (B = 1: j = K), as _op_case of tests/test_hip_spec_sample_gpu.py:
    q_i = p_i bitwise for i < j (ratio exactly 1), q_j has a 30-logit spike on the token the target finds least likely (drawn
    almost surely; outside the target's kept set: ratio 0); rows past the first K + 1 are 0.5-noise neighbours of p."""
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


def _restate(p, q, T, top_k, top_p, seed, counters, sids):
    """-> (draft ids [B][K], per-row StepResult, close calls) of the restatement alone"""
    B, K = q.shape[:2]
    d, want, close = [], [], 0
    for b in range(B):
        kq = [R.kept_set(q[b, i], T, top_k, top_p) for i in range(K)]
        draws = [R.draft_draw_ref(q[b, i], T, top_k, top_p, seed, counters[b], i, sids[b], kq[i]) for i in range(K)]
        d.append([t for t, _ in draws])
        want.append(R.spec_accept_ref(q[b], p[b], d[-1], T, top_k, top_p, seed, counters[b], sids[b], kq))
        close += want[-1].close_calls(CAP) + sum(1 for _, m in draws if m < CAP)
    return np.array(d, dtype=np.int32), want, close


def _run_op(p, q, d, T, top_k, top_p, seed, counters, sids):
    from specdec_hip.ops import spec_sample_accept_hip

    ctr = torch.tensor(counters, dtype=torch.int32, device="cuda")
    acc, nxt, ratios = spec_sample_accept_hip(
        _bf16(q).cuda(), _bf16(p).cuda(), torch.from_numpy(d).cuda(), T, seed=seed, draw_counters=ctr,
        stream_ids=torch.tensor(sids, dtype=torch.int32, device="cuda"), return_ratios=True, top_k=top_k, top_p=top_p)
    return acc.cpu().tolist(), nxt.cpu().tolist(), ratios.cpu().numpy(), ctr.cpu().tolist()


def _check_op(tag, p, q, T, top_k, top_p, seed, want_len=None):
    from specdec_hip.ops import sample_token_hip

    B, K, V = q.shape
    counters = [17 * b + 3 for b in range(B)]
    sids = [b + 2 for b in range(B)]
    d, want, close = _restate(p, q, T, top_k, top_p, seed, counters, sids)
    # the excuse cap: the restatement alone reports no decision within 1e-9 of a tie for these seeds
    assert close == 0, (tag, close)
    for b in range(B):
        if want_len and want_len[b] is not None:
            assert want[b].accept_len == want_len[b], (tag, b)
    # step 1 on the device is sd_sample_token itself: the same ids from the stored q rows
    for i in range(K):
        got = sample_token_hip(_bf16(q[:, i]).cuda(), T, top_k, top_p, seed=seed,
                               draw_counters=torch.tensor([c + i for c in counters], dtype=torch.int32, device="cuda"),
                               stream_ids=torch.tensor(sids, dtype=torch.int32, device="cuda"))
        assert got.cpu().tolist() == d[:, i].tolist(), (tag, i)
    acc, nxt, got_r, ctr = _run_op(p, q, d, T, top_k, top_p, seed, counters, sids)
    assert acc == [w.accept_len for w in want], tag
    assert nxt == [w.next_tok for w in want], tag
    assert ctr == [c + K + 1 for c in counters]
    want_r = np.stack([w.ratios for w in want])
    rel = np.abs(got_r - want_r) / np.maximum(want_r, np.finfo(np.float64).tiny)
    bound = ratio_rtol(min(top_k, V))
    print(f"[shaped op] {tag}: max relative ratio difference {rel.max():.3e} (bound {bound:.3e})")
    assert (rel <= bound).all(), (tag, rel.max())
    for b in range(B):   # q bitwise equal to p: ratio exactly 1 on the device too
        for i in range(K):
            if np.array_equal(q[b, i], p[b, i]):
                assert got_r[b, i] == 1.0
    return {w.accept_len for w in want}


@pytest.mark.parametrize("V", [128256, 50257])
@pytest.mark.parametrize("K", [1, 4, 8])
def test_op_matches_restatement(V, K):
    seen = set()
    for B in (1, 8):
        for si, (top_k, top_p) in enumerate(SHAPES):
            T = (0.7, 1.0, 1.5, 0.7)[si]
            seed = 1000 * K + 10 * B + si
            p, q, want_len = _op_case(V, K, B, seed)
            seen |= _check_op((V, K, B, T, top_k, top_p), p, q, T, top_k, top_p, seed, want_len)
    assert seen == set(range(K + 1)), seen


def _coarse_case(V, K, B, seed, step):
    """values on a grid of `step` logits: many equal values, so the top-k cut and the nucleus cut fall between equal logits"""
    rng = np.random.default_rng(seed)
    p = _bf16(np.round(rng.normal(0, 2.0, (B, K + 1, V)) / step) * step).float().numpy()
    q = _bf16(np.round((p[:, :K] + rng.normal(0, 0.7, (B, K, V))) / step) * step).float().numpy()
    return p, q


@pytest.mark.parametrize("V", [50257, 4099])
def test_op_with_ties_at_the_cuts(V):
    """Coarse rows: the k-th and (k+1)-th largest values are equal (asserted), as are the values on both sides of the nucleus
    cut of at least one row (asserted); the index-ascending rule decides, the same way on both sides."""
    K, B = 3, 4
    for si, (top_k, top_p, T) in enumerate([(50, 0.9, 1.0), (40, 0.5, 0.7), (1024, 1.0, 1.5), (7, 0.6, 1.0)]):
        p, q = _coarse_case(V, K, B, 300 + si, 0.5)
        ties_k = ties_p = 0
        for row in list(p.reshape(-1, V)) + list(q.reshape(-1, V)):
            s = np.sort(row)[::-1]
            ties_k += int(s[top_k - 1] == s[top_k])
            n = len(R.kept_set(row, T, top_k, top_p).ids)
            ties_p += int(n < top_k and s[n - 1] == s[n])
        assert ties_k > 0 and (top_p >= 1.0 or ties_p > 0), (top_k, top_p, ties_k, ties_p)
        _check_op(("coarse", V, top_k, top_p, T), p, q, T, top_k, top_p, 900 + si)


def test_op_draw0_inactive_rows_non_finite_and_refusals():
    from specdec_hip import _abi
    from specdec_hip.ops import spec_sample_accept_hip

    V, K, B, T, seed, top_k, top_p = 4099, 3, 4, 1.5, 77, 50, 0.9      # V not a multiple of 8: the scalar row walk
    rng = np.random.default_rng(3)
    p = _bf16(rng.normal(0, 2, (B, K + 1, V))).float().numpy()
    q = _bf16(p[:, :K] + rng.normal(0, 1.0, (B, K, V))).float().numpy()
    p[1, 0, 7] = np.nan            # on top of the target row: the point mass on id 7
    q[2, 1, 9] = np.inf            # on top of the draft row: d_2 = 9 for sure
    p[3, 0, 5] = -np.inf           # a -inf entry of a finite row: no special case
    d, want, close = _restate(p, q, T, top_k, top_p, seed, [40] * B, list(range(B)))
    assert close == 0 and d[2, 1] == 9 and want[1].positions[0].cand == 7
    assert not any(np.isnan(w.ratios).any() for w in want)       # no "rejected non-finite position" in the shaped mode
    dd = torch.from_numpy(d).cuda()
    acc, nxt, ratios = spec_sample_accept_hip(_bf16(q).cuda(), _bf16(p).cuda(), dd, T, seed=seed, draw=40, return_ratios=True,
                                              top_k=top_k, top_p=top_p)
    assert acc.cpu().tolist() == [w.accept_len for w in want] and nxt.cpu().tolist() == [w.next_tok for w in want]
    assert not np.isnan(ratios.cpu().numpy()).any()
    # a draft id outside q's kept set (only a caller of the op can produce one): NaN, rejected
    d2 = d.copy()
    d2[0, 0] = int(np.argmin(q[0, 0]))
    w0 = R.spec_accept_ref(q[0], p[0], d2[0], T, top_k, top_p, seed, 40, 0)
    acc2, nxt2, r2 = spec_sample_accept_hip(_bf16(q).cuda(), _bf16(p).cuda(), torch.from_numpy(d2).cuda(), T, seed=seed, draw=40,
                                            return_ratios=True, top_k=top_k, top_p=top_p)
    assert np.isnan(r2.cpu().numpy()[0, 0]) and acc2[0].item() == 0 == w0.accept_len and nxt2[0].item() == w0.next_tok
    # inactive rows: accept length 0, nothing else written, no draws consumed
    active = torch.tensor([1, 0, 1, 0], dtype=torch.int32, device="cuda")
    ctr = torch.full((B,), 40, dtype=torch.int32, device="cuda")
    acc3, nxt3 = spec_sample_accept_hip(_bf16(q).cuda(), _bf16(p).cuda(), dd, T, seed=seed, draw_counters=ctr, active=active,
                                        top_k=top_k, top_p=top_p)
    assert acc3.cpu().tolist() == [want[0].accept_len, 0, want[2].accept_len, 0]
    assert nxt3.cpu().tolist() == [want[0].next_tok, -1, want[2].next_tok, -1]
    assert ctr.cpu().tolist() == [40 + K + 1, 40, 40 + K + 1, 40]
    for kw, msg in (({"top_p": 0.9}, "without top_k"), ({"top_k": 2000}, "top_k=2000"), ({"top_k": 50, "top_p": 0.0}, "top_p")):
        with pytest.raises(_abi.HipLibraryError, match=msg):
            spec_sample_accept_hip(_bf16(q).cuda(), _bf16(p).cuda(), dd, T, **kw)
    with pytest.raises(_abi.HipLibraryError, match="temperature"):
        spec_sample_accept_hip(_bf16(q).cuda(), _bf16(p).cuda(), dd, 0.0, top_k=50)


# ------------------------------------------------------------------------------------------------------- the step
SEL_TGT = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=3, d_model=256, n_heads=4, n_kv_heads=2, head_dim=64, d_ff=512,
                        vocab=2048, max_pos=1024, rope_theta=500000.0, tie_embeddings=False, name="select-target")
SEL_DRF = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=2, d_model=256, n_heads=4, n_kv_heads=1, head_dim=64, d_ff=512,
                        vocab=2048, max_pos=1024, rope_theta=500000.0, tie_embeddings=False, name="select-draft")


def _pipe(drf, tgt, k=4, policy="longest_prefix", policy_params=None, eos=None, **lm_kw):
    from src.specdec import HipLM, SpeculativePipeline
    from src.specdec.models.hip_lm import IdTokenizer

    tok = IdTokenizer(tgt.config.vocab, eos_token_id=eos) if eos is not None else None
    return SpeculativePipeline(base_lm=HipLM(tgt.to("cuda"), tokenizer=tok, **lm_kw), draft_lm=HipLM(drf.to("cuda"), **lm_kw), controller="fixed",
                               controller_params={"k": k}, seed=1234, policy=policy, policy_params=policy_params)


def _records(loop, n, use_graph=True):
    out = []
    for _ in range(n):
        loop.step(use_graph=use_graph)
        r = loop.sync()
        out.append((r.accept_len.tolist(), r.new_tokens.tolist(), r.draft_tokens.tolist(), r.target_ids.tolist(), r.cur_len.tolist()))
    return out


def _device_steps(pipe, prompts, K, T, top_k, top_p, seed, n_steps, use_graph):
    """n_steps of the loop in the shaped mode, the device advancing its own state. Every step is checked against the
    restatement applied to THE DEVICE'S OWN stored logits: draws, accept lengths, hand-over tokens, counters."""
    from specdec_hip.engine import HipSpecDec

    B = len(prompts)
    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    loop = sess.loop
    counters = [5 * b for b in range(B)]
    loop.sync()
    loop.set_spec_sampling(True, T, seed, stream_ids=list(range(B)), draw_counts=counters, top_k=top_k, top_p=top_p)
    assert loop.spec_shape == (top_k, 1.0 if top_p is None else top_p)
    cur_len = [len(p) - 1 for p in prompts]
    out, close = [], 0
    for step in range(n_steps):
        loop.step(use_graph=use_graph)
        rec = loop.sync()
        q = loop.spec_draft_logits.float().cpu().numpy()
        p = loop.step_logits.float().cpu().numpy()
        for b in range(B):
            d, res, emitted, c2, m = R.spec_step_ref(q[b], p[b], T, top_k, top_p, seed, counters[b], b)
            close += res.close_calls(CAP) + int(m < CAP)
            assert [int(x) for x in rec.draft_tokens[b]] == d, (step, b)
            assert int(rec.accept_len[b]) == res.accept_len, (step, b, res.ratios)
            assert int(rec.n_new[b]) == len(emitted)
            assert [int(x) for x in rec.new_tokens[b]] == emitted + [-1] * (K + 1 - len(emitted)), (step, b)
            assert [int(x) for x in rec.target_ids[b]] == [int(np.argmax(p[b, i])) for i in range(K + 1)], (step, b)
            cur_len[b] += len(emitted)
            assert int(rec.cur_len[b]) == cur_len[b], (step, b)
            counters[b] = c2
            out.append((b, d, res.accept_len, emitted, res.ratios))
        assert loop.draw_counts == counters, step
    assert close == 0    # (checked after the fact here: the inputs are the device's own logits)
    loop.set_spec_sampling(False)
    sess.finish()
    return out


@pytest.mark.parametrize("B,use_graph", [(1, True), (8, True), (3, False)])
def test_step_reproduces_restatement_on_its_own_logits(B, use_graph):
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(B, 12, tgt.config.vocab).tolist()
    out = _device_steps(_pipe(drf, tgt), prompts, 4, 20.0, 50, 0.9, 4321, 12, use_graph)
    lens = [x[2] for x in out]
    print(f"[shaped step] B={B} graph={use_graph}: accept lengths {sorted(set(lens))}, mean {np.mean(lens):.2f}")
    assert len(set(lens)) >= 2, lens


def test_persistent_draft_and_launch_path(monkeypatch):
    """One row, a draft served by persistent launches (both forms of draft forward 0) and the same run on the launch path:
    each is checked step by step against the restatement on its own stored logits."""
    tgt = W.synthetic_llama(SEL_TGT, seed=0, device="cpu", layer_gain=0.05)
    drf = W.synthetic_llama(SEL_DRF, seed=1, device="cpu", layer_gain=0.05, embed_from=tgt, flip_fraction=0.3)
    prompts = synthetic_prompts(1, 9, SEL_TGT.vocab, seed=3).tolist()
    pipe = _pipe(drf, tgt)
    a = _device_steps(pipe, prompts, 4, 6.0, 40, 0.9, 99, 14, True)
    assert pipe._runtimes and all(rt["draft"].persist_tokens >= 2 for rt in pipe._runtimes.values()), "the draft must be on the persistent launch"
    monkeypatch.setenv("SPECDEC_PERSIST_MAX_T", "0")
    pipe0 = _pipe(drf, tgt)
    _device_steps(pipe0, prompts, 4, 6.0, 40, 0.9, 99, 14, True)
    assert all(rt["draft"].persist_tokens == 0 for rt in pipe0._runtimes.values())
    monkeypatch.delenv("SPECDEC_PERSIST_MAX_T")
    assert len({x[2] for x in a}) >= 2, [x[2] for x in a]


@pytest.mark.parametrize("lm_kw", [{"weight_dtype": "fp8"}, {"kv_page_len": 64}], ids=["fp8", "paged64"])
def test_step_under_fp8_storage_and_paged_kv(lm_kw):
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(3, 12, tgt.config.vocab).tolist()
    out = _device_steps(_pipe(drf, tgt, **lm_kw), prompts, 4, 20.0, 50, 0.9, 77, 10, True)
    assert len({x[2] for x in out}) >= 2


def test_top_k_1_is_the_greedy_step():
    """top_k = 1: both distributions are point masses on their argmax — draft argmax proposals, accepted iff equal to the
    target's argmax, next = the target's argmax: the records of a greedy session of the same pair."""
    from specdec_hip.engine import HipSpecDec

    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(2, 12, tgt.config.vocab).tolist()
    sess = _pipe(drf, tgt).start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    greedy = _records(sess.loop, 8)
    sess.finish()
    sess = _pipe(drf, tgt).start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    sess.loop.sync()
    sess.loop.set_spec_sampling(True, 0.7, 5, top_k=1)
    assert _records(sess.loop, 8) == greedy
    assert sess.loop.draw_counts == [8 * 5, 8 * 5]
    sess.loop.set_spec_sampling(False)
    sess.finish()
    assert len({a for r in greedy for a in r[0]}) >= 2


def test_draft_equal_to_target_accepts_everything(monkeypatch):
    """draft == target (one row: the draft's and the verify passes store the same logits): every ratio is exactly 1.0 and every
    proposal is accepted."""
    from specdec_hip.engine import HipSpecDec

    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", "0")
    _, tgt = tiny_pair(flip_fraction=0.25)
    K, T, seed, top_k, top_p = 4, 20.0, 5, 50, 0.9
    prompts = synthetic_prompts(1, 12, tgt.config.vocab).tolist()
    pipe = _pipe(tgt, tgt, K, "rejection", {"backend": "device", "temperature": T, "seed": seed, "top_k": top_k, "top_p": top_p})
    sess = pipe.start_session(prompts, 30, HipSpecDec.EMIT_BONUS, pipe._spec_sampling_config({}))
    steps = 0
    while sess.any_active() and steps < 6:
        c = sess.rows[0].draws
        assert sess.advance()
        rec = sess.last_record
        q = sess.loop.spec_draft_logits.float().cpu().numpy()[0]
        p = sess.loop.step_logits.float().cpu().numpy()[0]
        d = [int(x) for x in rec.draft_tokens[0]]
        res = R.spec_accept_ref(q, p, d, T, top_k, top_p, seed, c, 0)
        print(f"[shaped same] step {steps}: ratios {res.ratios.tolist()}, q == p bitwise: {[bool(np.array_equal(q[i], p[i])) for i in range(K)]}")
        assert (res.ratios == 1.0).all(), res.ratios
        assert int(rec.accept_len[0]) == K
        steps += 1
    sess.finish()
    assert steps >= 4


def test_shaping_off_returns_to_the_unshaped_and_the_greedy_records():
    from specdec_hip.engine import HipSpecDec

    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(2, 12, tgt.config.vocab).tolist()
    T, seed = 20.0, 11

    def run(pipe, shaped_first):
        sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
        loop = sess.loop
        loop.sync()
        if shaped_first:
            loop.set_spec_sampling(True, T, seed, top_k=50, top_p=0.9)
            _records(loop, 3)
            loop.set_spec_sampling(False)
            sess.finish()
            sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
            loop = sess.loop
            loop.sync()
        loop.set_spec_sampling(True, T, seed)
        assert loop.spec_shape is None
        unshaped = _records(loop, 6)
        loop.set_spec_sampling(False)
        sess.finish()
        sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
        greedy = _records(sess.loop, 6)
        sess.finish()
        return unshaped, greedy

    fresh = run(_pipe(drf, tgt), False)
    again = run(_pipe(drf, tgt), True)
    assert again[0] == fresh[0]
    assert again[1] == fresh[1]
    assert fresh[0] != fresh[1]


# ------------------------------------------------------------------------------------------------------- the pipeline
def _gen(pipe, prompts, n, **kw):
    return [r["generated_tokens"] for r in pipe.generate_batch(prompts, max_tokens=n, **kw)]


def test_pipeline_shape_from_the_policy_and_refusals(monkeypatch):
    from src.specdec import HipLM, SpeculativePipeline

    drf, tgt = tiny_pair(flip_fraction=0.25)
    V = tgt.config.vocab
    prompts = synthetic_prompts(3, 12, V).tolist()
    pp = {"backend": "device", "temperature": 20.0, "seed": 7, "top_k": 50, "top_p": 0.9}
    pipe = _pipe(drf, tgt, 4, "rejection", pp)
    toks = _gen(pipe, prompts, 24)
    eos = pipe.base_lm.get_tokenizer_info()["eos_token_id"]
    # the budget: a row ends at the step that reaches max_tokens (generate_batch does not truncate), or at a drawn EOS
    assert all(len(g) <= 24 + 4 and (len(g) >= 24 or eos in g[-2:]) and all(0 <= t < V for t in g) for g in toks)
    # reproducible per seed (steps queued ahead included); another seed and another shape draw differently
    assert _gen(pipe, prompts, 24) == toks
    assert _gen(pipe, prompts, 24, seed=8) != toks
    assert _gen(_pipe(drf, tgt, 4, "rejection", {**pp, "top_k": 5}), prompts, 24) != toks
    assert _gen(_pipe(drf, tgt, 4, "rejection", {**pp, "top_p": 0.3}), prompts, 24) != toks
    assert _gen(_pipe(drf, tgt, 4, "rejection", {k: v for k, v in pp.items() if k not in ("top_k", "top_p")}), prompts, 24) != toks
    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", "0")
    assert _gen(_pipe(drf, tgt, 4, "rejection", pp), prompts, 24) == toks       # launch -> wait -> rules order: the same tokens
    monkeypatch.delenv("SPECDEC_EARLY_LAUNCH")
    # ---- refusals
    with pytest.raises(NotImplementedError, match="top-k / top-p"):          # call-level shaping stays refused: the policy shapes
        pipe.generate_batch(prompts, max_tokens=8, top_k=50)
    with pytest.raises(NotImplementedError, match="top-k / top-p"):
        pipe.generate_batch(prompts, max_tokens=8, top_p=0.9)
    with pytest.raises(NotImplementedError, match="backend='host'"):
        _pipe(drf, tgt, 4, "rejection", {"temperature": 1.0, "top_k": 50})
    with pytest.raises(NotImplementedError, match="backend='host'"):
        _pipe(drf, tgt, 4, "rejection", {"backend": "host", "top_p": 0.9})
    with pytest.raises(NotImplementedError, match="without top_k"):
        _pipe(drf, tgt, 4, "rejection", {"backend": "device", "top_p": 0.9})
    with pytest.raises(NotImplementedError, match="1..1024"):
        _pipe(drf, tgt, 4, "rejection", {"backend": "device", "top_k": 2000})
    with pytest.raises(ValueError, match="top_p"):
        _pipe(drf, tgt, 4, "rejection", {"backend": "device", "top_k": 50, "top_p": 0.0})


def test_engine_refusals_and_order_of_calls():
    from specdec_hip import _abi
    from specdec_hip.engine import HipModel, HipSpecDec

    drf, tgt = tiny_pair(flip_fraction=0.25)
    t, d = HipModel(tgt.to("cuda"), batch=2, l_max=128), HipModel(drf.to("cuda"), batch=2, l_max=128)
    loop = HipSpecDec(d, t, 2, 4, HipSpecDec.EMIT_BONUS)
    for kw, msg in (({"top_k": 2000}, "top_k=2000"), ({"top_p": 0.9}, "without top_k"), ({"top_k": 50, "top_p": float("nan")}, "top_p")):
        with pytest.raises(_abi.HipLibraryError, match=msg):
            loop.set_spec_sampling(True, 1.0, 1, **kw)
    # legal before and after the mode is enabled
    _abi.check(loop.lib.sd_specdec_set_spec_shaping(loop.handle, 50, 0.9), "before")
    loop.set_spec_sampling(True, 1.0, 1, top_k=50, top_p=0.9)
    _abi.check(loop.lib.sd_specdec_set_spec_shaping(loop.handle, 0, 1.0), "after")
    loop.set_spec_sampling(False)


def _trace(pipe, prompt, max_tokens):
    from specdec_hip.engine import HipSpecDec

    sess = pipe.start_session([prompt], max_tokens, HipSpecDec.EMIT_BONUS, pipe._spec_sampling_config({}))
    steps = []
    while sess.any_active():
        r = sess.rows[0]
        gen0 = list(r.generated)
        assert sess.advance()
        rec, r = sess.last_record, sess.rows[0]
        steps.append((int(rec.accept_len[0]), [int(x) for x in rec.new_tokens[0][: int(rec.n_new[0])]], gen0, list(r.generated), r.active, r.draws))
    sess.finish()
    return steps, sess


@pytest.mark.parametrize("early", ["0", "1"], ids=["in-order", "queued-ahead"])
def test_eos_cut_keeps_the_in_order_counters(early, monkeypatch):
    """A baseline run (EOS = vocab - 1) gives the steps; the same seed is then re-run with the tokenizer's EOS set to
    the redrawn / bonus token of a chosen step: the run is the same up to that step, the row stops there, the host has counted
    (steps so far) x (K + 1) draws, and after the session the device's counter equals the host's (steps queued ahead drew for
    the stopped row and are written back with the repair)."""
    monkeypatch.setenv("SPECDEC_EARLY_LAUNCH", early)
    drf, tgt = tiny_pair(flip_fraction=0.25)
    K, V = 4, tgt.config.vocab
    pp = {"backend": "device", "temperature": 20.0, "seed": 31, "top_k": 50, "top_p": 0.9}
    prompt = synthetic_prompts(1, 12, V)[0].tolist()
    base, sess = _trace(_pipe(drf, tgt, K, "rejection", pp), prompt, 40)
    assert sess.eos == V - 1
    assert [s[5] for s in base] == [(i + 1) * (K + 1) for i in range(len(base))]
    assert sess.loop.draw_counts == [base[-1][5]]
    seen = set(prompt)
    pick = None
    for i, (a, new, *_rest) in enumerate(base):
        last0 = base[i][2][-1] if base[i][2] else prompt[-1]      # (steps whose tokens overlap the generated tail are not eligible)
        if pick is None and i >= 2 and a >= 1 and new[a] not in seen and new.count(new[a]) == 1 and last0 not in new and new[a] != V - 1:
            pick = (i, new[a])
        seen |= set(new)
    assert pick is not None, [(a, new) for a, new, *_ in base]
    i, eos = pick
    steps, sess = _trace(_pipe(drf, tgt, K, "rejection", pp, eos=eos), prompt, 40)
    assert sess.eos == eos and len(steps) == i + 1
    assert [(s[0], s[1]) for s in steps] == [(s[0], s[1]) for s in base[: i + 1]]
    assert steps[i][3][-1] == eos and steps[i][4] is False
    assert sess.rows[0].draws == (i + 1) * (K + 1)
    assert sess.loop.draw_counts == [sess.rows[0].draws]
