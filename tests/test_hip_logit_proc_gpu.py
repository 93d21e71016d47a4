"""Logit processors on the device (csrc/logit_proc.hip) against their CPU restatement (tests/logit_proc_ref.py): the stand-alone
op and the two count kernels bit for bit, the step of HipSpecDec with identity parameters against the unprocessed step, the
step with penalties against the restatement applied to the target's own raw logits (greedy, speculative sampling and its shaped
form, fp8 storage, paged KV), and the refusals of the C level.

Everything compared here is an integer or a bf16 word and must be EQUAL: the transform is a fixed sequence of correctly rounded
float32 operations, so there is no tolerance to derive."""

import numpy as np
import pytest
import torch

import logit_proc_ref as L
import spec_sample_ref as RS
import spec_shape_ref as RH
from helpers import synthetic_prompts, tiny_pair
from test_hip_spec_sample_gpu import SEL_TGT, _persist_pair, _pipe

pytestmark = pytest.mark.gpu

CAP = 1e-9


def _bits_of(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def _bf16_tensor(bits):
    return torch.from_numpy(np.ascontiguousarray(bits).view(np.int16)).view(torch.bfloat16)


def _counts_tensor(counts):
    return torch.from_numpy(np.ascontiguousarray(counts).view(np.int16)).cuda()


def _op_case(V, K, seed):
    """B = 3 rows of R = K + 1 positions: random values with zeros, -0, +-inf and a NaN row; counts with 0, prompt-bit-only, 1 and
    32767; in-step tokens with t_1 == t_2 and one token that has the prompt bit; a two-way tie for the maximum."""
    B, R = 3, K + 1
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 3.0, (B, R, V)).astype(np.float32)
    x[:, :, 0:4] = [0.0, -0.0, 1.5, -1.5]
    x[0, 1 % R, 77] = np.inf
    x[1, 0, 78] = -np.inf
    x[1, R - 1, 1234] = np.nan                # a NaN row: the NaN is the argmax
    x[1, R - 1, 4321] = np.nan
    x[0, 0, [V - 1, V - 3]] = 60.0           # the two largest values of row (0, 0) tie, in the tail elements of an odd V
    bits = _bits_of(torch.from_numpy(x).to(torch.bfloat16))
    counts = np.zeros((B, V), np.uint16)
    idx = rng.permutation(V)
    counts[:, idx[:300]] = L.PROMPT_BIT                       # prompt bit only
    counts[:, idx[300:600]] = 1
    counts[:, idx[600:700]] = L.PROMPT_BIT | 3
    counts[:, idx[700:720]] = L.COUNT_MASK
    counts[:, 0:4] = [L.PROMPT_BIT, 1, 2, L.PROMPT_BIT | 1]  # the zeros and +-1.5 are all penalised
    counts[0, [V - 1, V - 3]] = 0
    fresh = int(idx[800])                                      # count 0, no prompt bit
    prompted = int(idx[5])                                     # prompt bit, never generated
    toks = np.full((B, K), fresh, dtype=np.int32)              # t_1 == t_2 (== ...) == fresh
    if K >= 3:
        toks[:, 2] = prompted
    toks[1, 0] = prompted
    if K >= 4:
        toks[:, 3] = V + 5                                     # an id outside the vocabulary matches nothing
    bias = rng.normal(0, 1.0, (B, V)).astype(np.float32)
    bias[:, idx[900:1000]] = -np.inf
    bias[0, 77] = -np.inf                                      # +inf + -inf = NaN
    return bits, counts, toks, bias


@pytest.mark.parametrize("V", [50257, 128256])
@pytest.mark.parametrize("K", [1, 8])
def test_op_matches_restatement_bit_for_bit(V, K):
    from specdec_hip.ops import logit_process

    bits, counts, toks, bias = _op_case(V, K, 100 * K + (V & 7))
    active = [1, 1, 0]
    rp, pres, freq = 1.3, 0.5, 0.2
    for use_bias in (False, True):
        want, want_ids = L.process_rows(bits, counts, toks, None, rp, pres, freq, bias if use_bias else None, active)
        rows = _bf16_tensor(bits).cuda()
        ids = logit_process(rows, _counts_tensor(counts), rp, pres, freq, bias=torch.from_numpy(bias).cuda() if use_bias else None,
                            tokens=torch.from_numpy(toks).cuda(), active=torch.tensor(active, dtype=torch.int32, device="cuda"),
                            return_ids=True)
        got = _bits_of(rows)
        assert np.array_equal(got[2], bits[2]), "an inactive row was written"
        bad = np.argwhere(got != want)
        assert bad.size == 0, (V, K, use_bias, bad[:5], [hex(got[tuple(i)]) for i in bad[:5]], [hex(want[tuple(i)]) for i in bad[:5]])
        assert ids.cpu().tolist() == want_ids.tolist(), (V, K, use_bias)
        if not use_bias:
            assert want_ids[0, 0] == V - 3, "the tie of row (0, 0) must be decided by the index"
            assert want_ids[1, K] == 1234, "the NaN row"
    # the cases the issue names are really in the data
    x, w = L.bf16_to_f32(bits), L.bf16_to_f32(want)
    assert np.isnan(w[0, 1 % (K + 1), 77]) and np.isposinf(x[0, 1 % (K + 1), 77])
    assert K < 2 or toks[0, 0] == toks[0, 1]                                # t_1 == t_2
    assert K < 3 or counts[0, toks[0, 2]] == L.PROMPT_BIT                   # an in-step token with the prompt bit set
    assert (w[0] != x[0]).any()


def test_op_identity_fixed_token_count_and_a_strided_view():
    """identity parameters keep the rows and give torch's argmax; the draft-forward shape (row M - 1 of a [B][2][V] buffer, every
    row conditioned on the same number of tokens) at a V whose rows are misaligned"""
    from specdec_hip.ops import logit_counts, logit_process

    V, B = 50257, 3
    rng = np.random.default_rng(7)
    buf = torch.from_numpy(rng.normal(0, 3, (B, 2, V)).astype(np.float32)).to(torch.bfloat16).cuda()
    before = _bits_of(buf)
    counts = rng.integers(0, 3, (B, V)).astype(np.uint16) | (rng.integers(0, 2, (B, V)).astype(np.uint16) << 15)
    toks = rng.integers(0, V, (B, 4)).astype(np.int32)
    toks[:, 1] = toks[:, 0]
    ids = logit_process(buf, _counts_tensor(counts), tokens=torch.from_numpy(toks).cuda(), return_ids=True)
    assert np.array_equal(_bits_of(buf), before)
    assert ids.cpu().tolist() == [[L.argmax_bits(before[b, r]) for r in range(2)] for b in range(B)]
    view = buf[:, 1:2, :]
    ids = logit_process(view, _counts_tensor(counts), 1.7, -0.25, 0.125, tokens=torch.from_numpy(toks).cuda(), n_tokens=3, return_ids=True)
    want, want_ids = L.process_rows(before[:, 1:2], counts, toks, 3, 1.7, -0.25, 0.125)
    after = _bits_of(buf)
    assert np.array_equal(after[:, 0], before[:, 0]), "the rows between the processed ones were written"
    assert np.array_equal(after[:, 1:2], want) and ids.cpu().tolist() == want_ids.tolist()
    assert logit_process(view, logit_counts(B, V, "cuda")) is None


def test_count_kernels_match_restatement():
    from specdec_hip.ops import logit_counts, logit_counts_add, logit_counts_set

    V, B = 50257, 3
    rng = np.random.default_rng(11)
    counts = logit_counts(B, V, "cuda")
    counts.fill_(0x1234)                                           # set clears the row first
    prompt = rng.integers(0, V, 3000).astype(np.int32)
    gen = rng.integers(0, 40, 5000).astype(np.int32)               # heavy duplicates; 32767 is not reached here
    gen[:5] = [V - 1, V - 1, V, -1, int(prompt[0])]
    logit_counts_set(counts, 1, torch.from_numpy(prompt).cuda(), torch.from_numpy(gen).cuda())
    logit_counts_set(counts, 2, None, None)
    got = _bits_of(counts)
    assert (got[0] == 0x1234).all() and (got[2] == 0).all()
    want1 = L.counts_set(V, prompt, gen)
    assert np.array_equal(got[1], want1)
    assert want1[int(prompt[0])] & L.PROMPT_BIT and want1[int(prompt[0])] & L.COUNT_MASK
    # advance: a token emitted twice in one step, saturation at 32767 (with and without the prompt bit), -1 padding, an inactive row
    base = np.zeros((B, V), np.uint16)
    base[1] = want1
    base[0, 5] = L.COUNT_MASK - 1
    base[0, 6] = L.PROMPT_BIT | L.COUNT_MASK
    base[2, 9] = 4
    toks = np.array([[5, 5, 5, 6, 7], [7, 7, -1, -1, -1], [9, 9, 9, 9, 9]], dtype=np.int32)
    n_new = [5, 2, 5]
    active = [1, 1, 0]
    dev = _counts_tensor(base)
    logit_counts_add(dev, torch.from_numpy(toks).cuda(), torch.tensor(n_new, dtype=torch.int32, device="cuda"),
                     torch.tensor(active, dtype=torch.int32, device="cuda"))
    want = L.counts_add(base, toks, n_new, active)
    assert np.array_equal(_bits_of(dev), want)
    assert want[0, 5] == L.COUNT_MASK and want[0, 6] == (L.PROMPT_BIT | L.COUNT_MASK) and want[0, 7] == 1
    assert want[1, 7] == base[1, 7] + 2 and want[2, 9] == 4


# ------------------------------------------------------------------------------------------------------------ the step
def _records(pipe, prompts, n, use_graph, lp=None, emit=None):
    from specdec_hip.engine import HipSpecDec

    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS if emit is None else emit, None)
    loop = sess.loop
    loop.sync()
    if lp is not None:
        loop.set_logit_processors(True, *lp)
        for b, p in enumerate(prompts):
            loop.set_logit_counts_row(b, p)
    recs = []
    for _ in range(n):
        loop.step(use_graph=use_graph)
        r = loop.sync()
        recs.append((r.accept_len.tolist(), r.n_new.tolist(), r.new_tokens.tolist(), r.draft_tokens.tolist(), r.target_ids.tolist(),
                     r.cur_len.tolist()))
    if lp is not None:
        loop.set_logit_processors(False)
    sess.finish()
    return recs


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("use_graph", [True, False])
def test_identity_is_the_unprocessed_step_launch_path(B, use_graph):
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(B, 12, tgt.config.vocab).tolist()
    pipe = _pipe(drf, tgt)
    off = _records(pipe, prompts, 8, use_graph)
    on = _records(pipe, prompts, 8, use_graph, lp=(1.0, 0.0, 0.0))
    assert on == off
    assert _records(pipe, prompts, 8, use_graph) == off            # enable-then-disable returns to the greedy records
    assert len({a for r in off for a in r[0]}) >= 2, "the run must both accept and reject"


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("use_graph", [True, False])
def test_identity_is_the_unprocessed_step_persistent_draft(B, use_graph):
    """B = 1 also takes the device-selected two forms of draft forward 0"""
    drf, tgt = _persist_pair()
    prompts = synthetic_prompts(B, 9, SEL_TGT.vocab, seed=3).tolist()
    pipe = _pipe(drf, tgt)
    off = _records(pipe, prompts, 10, use_graph)
    assert B > 1 or all(rt["draft"].persist_tokens >= 2 for rt in pipe._runtimes.values()), "the draft must be on the persistent launch"
    on = _records(pipe, prompts, 10, use_graph, lp=(1.0, 0.0, 0.0))
    assert on == off
    lens = [r[0][0] for r in off]
    assert B > 1 or (4 in lens and min(lens) < 4), lens     # both forms of forward 0 follow


def _greedy_accept(ids, d, K):
    a = 0
    while a < K and ids[a] == d[a]:
        a += 1
    return a


def _check_steps(pipe, prompts, K, params, n_steps, use_graph, mode="greedy", T=20.0, seed=4321, top_k=None, top_p=None, bias_ids=()):
    """n_steps of the loop with processors on. Per step: the target's RAW rows are recomputed by sd_model_forward over the record's
    (last, d_1..d_K) at the step's positions (the same kernels on the same inputs: the K/V it rewrites is identical), the
    restatement with the counts from before the step must give the stored rows byte for byte, the record must follow from the
    processed rows through the existing restatements, and the counts must advance as the restatement's."""
    from specdec_hip.engine import HipSpecDec

    B = len(prompts)
    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    loop = sess.loop
    loop.sync()
    V = loop.target.cfg.vocab
    counters = [5 * b for b in range(B)]
    if mode != "greedy":
        loop.set_spec_sampling(True, T, seed, stream_ids=list(range(B)), draw_counts=counters, top_k=top_k, top_p=top_p)
    loop.set_logit_processors(True, *params, bias=bool(bias_ids))
    bias = None
    if bias_ids:
        bias = np.zeros((B, V), np.float32)
        bias[:, list(bias_ids)] = -np.inf
        loop.logit_bias.copy_(torch.from_numpy(bias))
    counts = np.stack([L.counts_set(V, p) for p in prompts])
    for b, p in enumerate(prompts):
        loop.set_logit_counts_row(b, p)
    torch.cuda.synchronize()
    last = [p[-1] for p in prompts]
    cur = [len(p) - 1 for p in prompts]
    lens, close, changed = [], 0, 0
    for step in range(n_steps):
        loop.step(use_graph=use_graph)
        rec = loop.sync()
        stored = _bits_of(loop.step_logits)
        d = rec.draft_tokens.astype(np.int32)
        toks = torch.from_numpy(np.concatenate([np.array(last, np.int32)[:, None], d], 1)).cuda()
        _, raw = loop.target.forward(toks, torch.tensor(cur, dtype=torch.int32, device="cuda"), want_logits=True, logits_dtype=torch.bfloat16)
        torch.cuda.synchronize()
        raw = _bits_of(raw)
        want, want_ids = L.process_rows(raw, counts, d, None, *params, bias)
        assert np.array_equal(stored, want), (step, np.argwhere(stored != want)[:4])
        changed += int((want != raw).sum())
        assert rec.target_ids.tolist() == want_ids.tolist(), step
        p = L.bf16_to_f32(stored)
        for b in range(B):
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
            assert not set(emitted) & set(bias_ids), (step, b, emitted)
            lens.append(a)
            last[b] = emitted[-1]
            cur[b] += len(emitted)
        assert rec.cur_len.tolist() == cur, step
        counts = L.counts_add(counts, rec.new_tokens, rec.n_new)
        assert np.array_equal(_bits_of(loop.logit_counts), counts), step
    assert close == 0 and changed > 0
    if mode != "greedy":
        loop.set_spec_sampling(False)
    loop.set_logit_processors(False)
    sess.finish()
    return lens


PEN = (1.3, 0.5, 0.2)


@pytest.mark.parametrize("B,use_graph", [(1, True), (3, True), (3, False)])
def test_greedy_step_reproduces_restatement_on_its_own_raw_logits(B, use_graph):
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(B, 12, tgt.config.vocab).tolist()
    lens = _check_steps(_pipe(drf, tgt), prompts, 4, PEN, 10, use_graph, bias_ids=(17, 400, 999))
    assert len(set(lens)) >= 2, lens


def test_greedy_step_persistent_draft_with_penalties():
    drf, tgt = _persist_pair()
    prompts = synthetic_prompts(1, 9, SEL_TGT.vocab, seed=3).tolist()
    lens = _check_steps(_pipe(drf, tgt), prompts, 4, PEN, 12, True)
    assert len(set(lens)) >= 2, lens


@pytest.mark.parametrize("mode,top_k,top_p", [("spec", None, None), ("shaped", 50, 0.9)])
def test_spec_sampling_step_reproduces_restatement_on_processed_rows(mode, top_k, top_p):
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(3, 12, tgt.config.vocab).tolist()
    lens = _check_steps(_pipe(drf, tgt), prompts, 4, PEN, 8, True, mode=mode, top_k=top_k, top_p=top_p)
    assert len(set(lens)) >= 2, lens


@pytest.mark.parametrize("lm_kw", [{"weight_dtype": "fp8"}, {"kv_page_len": 64}], ids=["fp8", "paged64"])
def test_greedy_step_under_fp8_storage_and_paged_kv(lm_kw):
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(3, 12, tgt.config.vocab).tolist()
    _check_steps(_pipe(drf, tgt, **lm_kw), prompts, 4, PEN, 6, True)


def test_draft_emit_mode_and_sampled_bonus_run_on_processed_rows():
    """SD_EMIT_DRAFT is legal: identity equals the unprocessed records there too; with a +1000 bias every token either model
    proposes, and so every emitted token, is the favoured id."""
    from specdec_hip.engine import HipSpecDec

    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(2, 12, tgt.config.vocab).tolist()
    pipe = _pipe(drf, tgt)
    off = _records(pipe, prompts, 6, True, emit=HipSpecDec.EMIT_DRAFT)
    assert _records(pipe, prompts, 6, True, lp=(1.0, 0.0, 0.0), emit=HipSpecDec.EMIT_DRAFT) == off
    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    loop = sess.loop
    loop.sync()
    loop.set_sampling(True, 0.8, top_k=20, seed=5)
    loop.set_logit_processors(True, 1.0, 0.0, 0.0, bias=True)
    loop.logit_bias.zero_()
    loop.logit_bias[:, 321] = 1000.0   # (the synthetic target puts ~130 on its successor token)
    torch.cuda.synchronize()
    for _ in range(4):
        loop.step(use_graph=True)
        r = loop.sync()
        assert (r.draft_tokens == 321).all() and (r.target_ids == 321).all()
        assert all(int(t) in (321, -1) for row in r.new_tokens for t in row) and r.accept_len.tolist() == [4, 4]
    loop.set_logit_processors(False)
    loop.set_sampling(False)
    sess.finish()


def test_refusals_at_the_c_level():
    from specdec_hip import _abi
    from specdec_hip.engine import HipSpecDec
    from specdec_hip.ops import logit_counts, logit_process

    lib = _abi.load()
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(2, 12, tgt.config.vocab).tolist()
    pipe = _pipe(drf, tgt)
    sess = pipe.start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    loop = sess.loop
    loop.sync()
    V, B, K = loop.target.cfg.vocab, loop.B, loop.K
    counts = logit_counts(B, V, "cuda")
    bias = torch.zeros((B, V), dtype=torch.float32, device="cuda")
    logits = torch.empty((B, K + 1, V), dtype=torch.bfloat16, device="cuda")
    ws = torch.empty(max(lib.sd_logit_process_workspace(B, K + 1, V), 16), dtype=torch.uint8, device="cuda")

    def call(rp=1.2, pres=0.0, freq=0.0, c=counts, cb=None, bs=bias, bb=None, lg=logits, lb=None, w=ws, wb=None, handle=None):
        return lib.sd_specdec_set_logit_processors(
            loop.handle if handle is None else handle, 1, rp, pres, freq, c.data_ptr() if c is not None else None,
            (c.numel() * 2 if c is not None else 0) if cb is None else cb, bs.data_ptr() if bs is not None else None,
            (bs.numel() * 4 if bs is not None else 0) if bb is None else bb, lg if isinstance(lg, int) else (lg.data_ptr() if lg is not None else None),
            (logits.numel() * 2) if lb is None else lb, w.data_ptr() if w is not None else None, (w.numel() if w is not None else 0) if wb is None else wb)

    for kw, word in (({"rp": 0.0}, "repetition_penalty"), ({"rp": -1.0}, "repetition_penalty"), ({"rp": float("nan")}, "repetition_penalty"),
                     ({"pres": float("inf")}, "finite"), ({"freq": float("nan")}, "finite"), ({"c": None}, "counts"),
                     ({"cb": B * V * 2 - 2}, "counts"), ({"bb": B * V * 4 - 4}, "bias"), ({"lg": None}, "logits buffer"),
                     ({"lb": B * (K + 1) * V * 2 - 2}, "logits buffer"), ({"w": None}, "workspace"), ({"wb": 8}, "workspace"),
                     ({"lg": logits.data_ptr() + 2}, "aligned")):
        assert call(**kw) != 0, kw
        assert word in _abi.last_error(), (kw, _abi.last_error())
    assert call() == 0
    loop.set_adaptive(False)
    with pytest.raises(_abi.HipLibraryError, match="logit processors keep a fixed K"):
        loop.set_adaptive(True, initial_k=2, min_k=1, max_k=K)
    assert lib.sd_specdec_set_logit_processors(loop.handle, 0, 1.0, 0.0, 0.0, None, 0, None, 0, None, 0, None, 0) == 0
    loop.set_adaptive(True, initial_k=2, min_k=1, max_k=K)
    assert call() != 0 and "adaptive K" in _abi.last_error()
    loop.set_adaptive(False)
    sess.finish()
    # loops without a draft model: self-draft (and with it Medusa heads and EAGLE, which are modes of such a loop)
    selfd = HipSpecDec(None, loop.target, B, K)
    assert call(handle=selfd.handle) != 0 and "draft model" in _abi.last_error()
    selfd.close()
    # the op
    rows = torch.zeros((1, 1, V), dtype=torch.bfloat16, device="cuda")
    c1 = logit_counts(1, V, "cuda")
    for kw, word in (({"repetition_penalty": 0.0}, "repetition_penalty"), ({"presence_penalty": float("inf")}, "finite"),
                     ({"n_tokens": 65}, "in-step tokens"), ({"n_tokens": 2}, "token array")):
        with pytest.raises(_abi.HipLibraryError, match=word):
            logit_process(rows, c1, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        logit_process(rows.cpu(), c1.cpu())
