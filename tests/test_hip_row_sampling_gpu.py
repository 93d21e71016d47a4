"""Per-request sampling parameters on the device (sd_sample_token_rows, sd_spec_sample_accept_rows, sd_logit_process_rows,
sd_specdec_set_row_sampling): row b of a _rows launch must give, bit for bit, what the scalar entry point gives on that row
alone with table[b] normalised, the same draw counter and the same stream id — and what the CPU restatement of that row gives
(oracle/sampling_ref.py, tests/spec_sample_ref.py, tests/spec_shape_ref.py, tests/logit_proc_ref.py).

Integer outputs (ids, accept lengths, counters) and processed bf16 rows are compared with ==, against the scalar ops the float64
ratios too. Against numpy the ratios carry the derived bounds of the two speculative-sampling suites (ratio_rtol_* below; the
device's exp / log are faithful, not correctly rounded). A comparison within rounding of a tie could legitimately differ between
the device and numpy, so every test first asserts that the restatement reports ZERO decisions within CAP = 1e-9 (the cap of
tests/test_hip_spec_shape_gpu.py) for its fixed seeds: nothing is ever excused."""

import numpy as np
import pytest
import torch

import logit_proc_ref as LP
import spec_sample_ref as SS
import spec_shape_ref as R
from helpers import synthetic_prompts, tiny_pair
from oracle import sampling_ref as S
from specdec_hip.sampling_params import RowSampling, SamplingParams, unpack

pytestmark = pytest.mark.gpu

CAP = 1e-9
B = 8
NAN, INF = float("nan"), float("inf")
U = 2.0 ** -53


def ratio_rtol_unshaped(V):
    """ratio_rtol of tests/test_hip_spec_sample_gpu.py (derived there): (4 V + 2048) u."""
    return (4 * V + 2048) * U


def ratio_rtol_shaped(n):
    """ratio_rtol of tests/test_hip_spec_shape_gpu.py (derived there): (4 n + 32) u, n = kept-set size <= top_k."""
    return (4 * n + 32) * U


def _bf16(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16)


def _rec(T=1.0, k=0, p=1.0, seed=0, rp=1.0, pres=0.0, freq=0.0):
    return RowSampling(T, k, p, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF, rp, pres, freq)


def _table(recs):
    raw = b"".join(bytes(r) for r in recs)
    return torch.frombuffer(bytearray(raw), dtype=torch.uint8).view(len(recs), 32).cuda()


# The mixed table: one row of each kind. (record as the device reads it, the scalar arguments of its normalised form for the
# sampler, the same for the speculative-sampling kernels). Row 7 is inactive.
SEEDS = [1000 + 37 * b for b in range(B)]
SEEDS[2] = (3 << 32) | 5            # a seed with a high word
SIDS = [11, 3, 7, 2, 9, 5, 4, 6]
COUNTERS = [17 * b + 3 for b in range(B)]
ACTIVE = [1, 1, 1, 1, 1, 1, 1, 0]
MIXED = [
    (dict(T=0.0, k=40, p=0.5), (1.0, 1, None), (1.0, 1, None)),            # T = 0: greedy, whatever the rest says
    (dict(T=1.0, k=1, p=1.0), (1.0, 1, None), (1.0, 1, None)),             # top_k = 1
    (dict(T=0.7, k=50, p=0.9), (0.7, 50, 0.9), (0.7, 50, 0.9)),            # (coarse row: the cuts fall between equal logits)
    (dict(T=1.0, k=1024, p=1.0), (1.0, 1024, None), (1.0, 1024, None)),
    (dict(T=1.0, k=0, p=0.9), (1.0, None, 0.9), (1.0, 1, None)),           # full-vocabulary nucleus; greedy for the spec kernels
    (dict(T=1.5, k=0, p=1.0), (1.5, None, None), (1.5, None, None)),       # Gumbel-max / the unshaped statistics
    (dict(T=NAN, k=50, p=0.9), (1.0, 1, None), (1.0, 1, None)),            # NaN temperature: greedy
    (dict(T=0.7, k=50, p=0.9), (0.7, 50, 0.9), (0.7, 50, 0.9)),            # inactive
]


def mixed_table():
    return [_rec(seed=SEEDS[b], **MIXED[b][0]) for b in range(B)]


def mixed_logits(V, K, seed):
    """p [B][K+1][V], q [B][K][V], bf16-valued float32. q is a 0.5-noise neighbour of p, bitwise p at position 0 of the even
    rows (ratio exactly 1); row 2 sits on a 0.25 grid (ties at the top-k and nucleus cuts), row 4 is nearly flat (noise 0.01: the
    0.9 nucleus keeps ~0.9 V tokens, at least 3 rank blocks of 1024)."""
    rng = np.random.default_rng(seed)
    p = rng.normal(0, 3.0, (B, K + 1, V))
    p[2] = np.round(rng.normal(0, 2.0, (K + 1, V)) / 0.25) * 0.25
    p[4] = rng.normal(0, 0.01, (K + 1, V))
    p = _bf16(p).float().numpy()
    q = p[:, :K] + rng.normal(0, 0.5, (B, K, V))
    q[2] = np.round(q[2] / 0.25) * 0.25
    q[4] = p[4, :K] + rng.normal(0, 0.01, (K, V))
    q = _bf16(q).float().numpy()
    q[0::2, 0] = p[0::2, 0]
    return p, q


# ------------------------------------------------------------------------------------------------------- the restatements
def sample_ref(row, T, k, p, seed, draw, sid):
    """sample_token_ref with the margin of its one decision: the inversion gap (top-k, nucleus; with the nucleus-cut margin) or
    the top-2 Gumbel-score gap. -> (token, margin)"""
    tok = S.sample_token_ref(row, T, k, p, seed, draw, sid)
    if k:
        ks = R.kept_set(row, T, k, p)
        j, gap = R.invert(ks.e, ks.z, S.draw_uniform(seed, draw, sid))
        assert int(ks.ids[j]) == tok
        return tok, min(gap, ks.cut)
    if p is not None:
        ids, e = S.nucleus_distribution(row, T, p)
        j, gap = R.invert(e, R.seq_sum(e), S.draw_uniform(seed, draw, sid))
        assert int(ids[j]) == tok
        return tok, gap
    score = SS.scaled(row, T) + SS.gumbel_noise(len(row), seed, draw, sid)
    best, gap = SS.best_of(score)
    assert best == tok
    return tok, gap


def spec_row_ref(q, p, T, k, tp, seed, counter, sid):
    """One row of speculative sampling from its logits, shaped (k) or not: -> (draft ids, StepResult, emitted, counter after,
    close calls)."""
    if k:
        d, res, emitted, c2, m = R.spec_step_ref(q, p, T, k, tp, seed, counter, sid)
        return d, res, emitted, c2, res.close_calls(CAP) + int(m < CAP)
    d, res, emitted, c2 = SS.spec_step_ref(q, p, T, seed, counter, sid)
    close = res.close_calls(CAP)
    for i in range(len(d)):      # the draft draws are Gumbel-max draws too
        sc = SS.scaled(q[i], T) + SS.gumbel_noise(q.shape[1], seed, (counter + i) & S.MASK32, sid)
        close += int(SS.best_of(sc)[1] < CAP)
    return d, res, emitted, c2, close


SHAPES = [(4099, 1), (4099, 4), (8192, 1), (8192, 4)]    # 4099: unaligned rows, two process workgroups, four rank blocks; 8192: 16-byte path


# ------------------------------------------------------------------------------------------------------- the ops
@pytest.mark.parametrize("V,K", SHAPES)
def test_sample_token_rows(V, K):
    from specdec_hip.ops import sample_token_hip, sample_token_rows_hip

    p, _ = mixed_logits(V, K, 10 * V + K)
    pos = [b % (K + 1) for b in range(B)]                  # entry b samples row b * (K + 1) + pos[b], as the step does
    want, margins = [], []
    for b in range(B):
        T, k, tp = MIXED[b][1]
        tok, m = sample_ref(p[b, pos[b]], T, k, tp, SEEDS[b], COUNTERS[b], SIDS[b])
        want.append(tok)
        margins.append(m)
    assert sum(1 for b in range(B) if ACTIVE[b] and margins[b] < CAP) == 0, margins
    nuc_ids, _ = S.nucleus_distribution(p[4, pos[4]], 1.0, 0.9)
    assert len(nuc_ids) > 2 * 1024, len(nuc_ids)           # the nucleus row walks at least 3 rank blocks
    s2 = np.sort(p[2, pos[2]])[::-1]
    assert s2[49] == s2[50]                                # the coarse row: a tie at the top-k cut
    dev = dict(device="cuda", dtype=torch.int32)
    logits = _bf16(p.reshape(B * (K + 1), V)).cuda()
    ctr = torch.tensor(COUNTERS, **dev)
    got = sample_token_rows_hip(logits, _table(mixed_table()), pos=torch.tensor(pos, **dev), rows_per_entry=K + 1, draw_counters=ctr,
                                stream_ids=torch.tensor(SIDS, **dev), active=torch.tensor(ACTIVE, **dev)).cpu().tolist()
    ctr = ctr.cpu().tolist()
    for b in range(B):
        if not ACTIVE[b]:
            assert ctr[b] == COUNTERS[b]                   # the inactive row consumes no draw
            continue
        T, k, tp = MIXED[b][1]
        c1 = torch.tensor([COUNTERS[b]], **dev)
        alone = sample_token_hip(logits[b * (K + 1) + pos[b]], T, k, tp, seed=SEEDS[b], draw_counters=c1,
                                 stream_ids=torch.tensor([SIDS[b]], **dev))
        assert got[b] == int(alone.item()) == want[b], (b, got[b], int(alone.item()), want[b])
        assert ctr[b] == int(c1.item()) == COUNTERS[b] + 1
    # the greedy rows: the argmax of their row (value, then lowest index)
    for b in (0, 1, 6):
        assert got[b] == int(np.argmax(p[b, pos[b]]))
    # a list of SamplingParams is packed by the op: the same ids as the raw records of those rows
    ps = [SamplingParams(temperature=0.0), SamplingParams(top_k=1), SamplingParams(0.7, 50, 0.9), SamplingParams(top_k=1024),
          SamplingParams(top_p=0.9), SamplingParams(temperature=1.5)]
    ps = [x.with_seed(SEEDS[b]) for b, x in enumerate(ps)]
    got2 = sample_token_rows_hip(logits[: 6 * (K + 1)], ps, pos=torch.tensor(pos[:6], **dev), rows_per_entry=K + 1,
                                 draw_counters=torch.tensor(COUNTERS[:6], **dev), stream_ids=torch.tensor(SIDS[:6], **dev))
    assert got2.cpu().tolist() == got[:6]


def test_sample_token_rows_f32_and_draw0():
    """float32 logits, no counters (draw0), default stream ids (b): the other argument forms of the scalar op."""
    from specdec_hip.ops import sample_token_hip, sample_token_rows_hip

    V = 4099
    p, _ = mixed_logits(V, 1, 5)
    logits = torch.from_numpy(p[:, 0].copy()).cuda()
    got = sample_token_rows_hip(logits, _table(mixed_table()), draw=9).cpu().tolist()
    margins = []
    for b in range(B):
        T, k, tp = MIXED[b][1]
        tok, m = sample_ref(p[b, 0], T, k, tp, SEEDS[b], 9, b)
        margins.append(m)
        alone = sample_token_hip(logits[b], T, k, tp, seed=SEEDS[b], draw=9, stream_ids=torch.tensor([b], dtype=torch.int32, device="cuda"))
        assert got[b] == int(alone.item()) == tok, b
    assert min(margins) >= CAP, margins


@pytest.mark.parametrize("V,K", SHAPES)
def test_spec_sample_accept_rows(V, K):
    from specdec_hip.ops import spec_sample_accept_hip, spec_sample_accept_rows_hip

    p, q = mixed_logits(V, K, 20 * V + K)
    d, want, close = [], [], 0
    for b in range(B):
        T, k, tp = MIXED[b][2]
        db, res, _, _, c = spec_row_ref(q[b], p[b], T, k, tp, SEEDS[b], COUNTERS[b], SIDS[b])
        d.append(db)
        want.append(res)
        close += c if ACTIVE[b] else 0
    assert close == 0, close                               # the excuse cap: no decision of the restatement is within 1e-9 of a tie
    dev = dict(device="cuda", dtype=torch.int32)
    qd, pd, dd = _bf16(q).cuda(), _bf16(p).cuda(), torch.tensor(d, **dev)
    ctr = torch.tensor(COUNTERS, **dev)
    acc, nxt, ratios = spec_sample_accept_rows_hip(qd, pd, dd, _table(mixed_table()), draw_counters=ctr, stream_ids=torch.tensor(SIDS, **dev),
                                                   active=torch.tensor(ACTIVE, **dev), return_ratios=True)
    acc, nxt, ratios, ctr = acc.cpu().tolist(), nxt.cpu().tolist(), ratios.cpu().numpy(), ctr.cpu().tolist()
    seen = set()
    for b in range(B):
        if not ACTIVE[b]:
            assert (acc[b], nxt[b], ctr[b]) == (0, -1, COUNTERS[b]) and np.isnan(ratios[b]).all()
            continue
        T, k, tp = MIXED[b][2]
        c1 = torch.tensor([COUNTERS[b]], **dev)
        a1, n1, r1 = spec_sample_accept_hip(qd[b:b + 1], pd[b:b + 1], dd[b:b + 1], T, seed=SEEDS[b], draw_counters=c1,
                                            stream_ids=torch.tensor([SIDS[b]], **dev), return_ratios=True, top_k=k, top_p=tp)
        # the scalar op on the row alone: everything equal, the float64 ratios too
        assert (acc[b], nxt[b], ctr[b]) == (int(a1.item()), int(n1.item()), int(c1.item())), b
        assert ctr[b] == COUNTERS[b] + K + 1
        assert (ratios[b] == r1.cpu().numpy()[0]).all(), (b, ratios[b], r1)
        # the restatement of the row
        assert (acc[b], nxt[b]) == (want[b].accept_len, want[b].next_tok), (b, want[b].ratios)
        rel = np.abs(ratios[b] - want[b].ratios) / np.maximum(want[b].ratios, np.finfo(np.float64).tiny)
        bound = ratio_rtol_shaped(min(k, V)) if k else ratio_rtol_unshaped(V)
        print(f"[rows spec op] V={V} K={K} row {b}: max relative ratio difference {rel.max():.3e} (bound {bound:.3e})")
        assert (rel <= bound).all(), (b, rel.max())
        seen.add(acc[b])
    if K > 1:
        assert len(seen) >= 2, seen
    assert ratios[0, 0] == 1.0 and ratios[2, 0] == 1.0     # q bitwise p at position 0 of the even rows
    # (0, 0.9) has no form in the speculative-sampling kernels: the greedy result — argmax proposals, accepted while they are the
    # target's argmax, then the target's argmax
    am_q, am_p = [int(np.argmax(q[4, i])) for i in range(K)], [int(np.argmax(p[4, i])) for i in range(K + 1)]
    assert d[4] == am_q
    a = 0
    while a < K and am_q[a] == am_p[a]:
        a += 1
    assert (acc[4], nxt[4]) == (a, am_p[a])


def _lp_case(V, R_, seed):
    rng = np.random.default_rng(seed)
    rows = LP.f32_to_bf16(rng.normal(0, 3.0, (B, R_, V)).astype(np.float32))
    counts = np.zeros((B, V), dtype=np.uint16)
    for b in range(B):
        counts[b] = LP.counts_set(V, rng.integers(0, V, 40), rng.integers(0, V, 60))
    counts[0, 5] = 0x7FFF                                     # a saturated count
    tokens = rng.integers(0, V, (B, 8)).astype(np.int32)
    tokens[:, 1] = tokens[:, 0]                               # a token proposed twice counts twice
    bias = np.zeros((B, V), dtype=np.float32)
    bias[:, 7] = -np.inf
    bias[:, 11] = 2.5
    return rows, counts, tokens, bias


# per-row penalties as the device reads them, and their normalised form
LP_ROWS = [
    ((1.3, 0.5, 0.25), (1.3, 0.5, 0.25)),
    ((1.0, 0.0, 0.0), (1.0, 0.0, 0.0)),
    ((0.8, -0.5, 0.0), (0.8, -0.5, 0.0)),
    ((-1.0, 0.5, 0.25), (1.0, 0.0, 0.0)),          # rp <= 0: the scalar entry refuses -> identity for the row
    ((1.3, INF, 0.0), (1.0, 0.0, 0.0)),            # a presence penalty that is not finite -> identity
    ((1.0, 0.0, 0.125), (1.0, 0.0, 0.125)),
    ((NAN, 0.0, 0.0), (1.0, 0.0, 0.0)),            # NaN rp -> identity
    ((1.3, 0.5, 0.25), (1.3, 0.5, 0.25)),          # inactive
]


def _as_bits(t):
    return t.view(torch.int16).cpu().numpy().view(np.uint16)


@pytest.mark.parametrize("V", [4099, 8192])
@pytest.mark.parametrize("form", ["verify", "draft", "grammar"])
def test_logit_process_rows(V, form):
    from specdec_hip.ops import fsm_build_masks, logit_process, logit_process_fsm, logit_process_rows_hip

    K = 4
    R_ = 1 if form == "draft" else K + 1
    n_tokens = 2 if form == "draft" else None
    rows, counts, tokens, bias = _lp_case(V, R_, V + len(form))
    table = _table([_rec(rp=a[0], pres=a[1], freq=a[2]) for a, _ in LP_ROWS])
    dev = "cuda"
    rows_d = torch.from_numpy(rows.view(np.int16)).to(dev).view(torch.bfloat16)
    counts_d = torch.from_numpy(counts.view(np.int16)).to(dev)
    tokens_d, bias_d = torch.from_numpy(tokens).to(dev), torch.from_numpy(bias).to(dev)
    active_d = torch.tensor(ACTIVE, dtype=torch.int32, device=dev)
    fsm = {}
    if form == "grammar":
        rng = np.random.default_rng(V)
        S_ = 3
        nxt = rng.integers(0, S_, (S_, V)).astype(np.uint16)
        nxt[rng.random((S_, V)) < 0.5] = 0xFFFF
        nxt_d = torch.from_numpy(nxt.view(np.int16)).to(dev)
        state = torch.tensor([0, 1, -1, 2, 0, 1, 2, 0], dtype=torch.int32, device=dev)
        fsm = dict(nxt=nxt_d, allow=fsm_build_masks(nxt_d), fsm_state=state, eos_id=V - 1)
    got = rows_d.clone()
    ids = logit_process_rows_hip(got, counts_d, table, bias=bias_d, tokens=tokens_d, n_tokens=n_tokens, active=active_d, return_ids=True, **fsm)
    got_bits, ids = _as_bits(got), ids.cpu().numpy()
    changed = 0
    for b in range(B):
        rp, pres, freq = LP_ROWS[b][1]
        alone = rows_d[b:b + 1].clone()
        args = dict(repetition_penalty=rp, presence_penalty=pres, frequency_penalty=freq, bias=bias_d[b:b + 1], tokens=tokens_d[b:b + 1],
                    n_tokens=n_tokens, active=active_d[b:b + 1], return_ids=True)
        if form == "grammar":
            ids1 = logit_process_fsm(alone, counts_d[b:b + 1], fsm["nxt"], fsm["allow"], fsm["fsm_state"][b:b + 1], fsm["eos_id"], **args)
        else:
            ids1 = logit_process(alone, counts_d[b:b + 1], **args)
        assert (got_bits[b] == _as_bits(alone)[0]).all(), (form, b)          # the bytes of the processed rows
        assert (ids[b] == ids1.cpu().numpy()[0]).all(), (form, b)
        if form != "grammar":                                                 # the CPU restatement of the row
            want, want_ids = LP.process_rows(rows[b:b + 1], counts[b:b + 1], tokens[b:b + 1], n_tokens, rp, pres, freq, bias[b:b + 1],
                                             active=[ACTIVE[b]])
            assert (got_bits[b] == want[0]).all() and (ids[b] == want_ids[0]).all(), (form, b)
        changed += int((got_bits[b] != rows[b]).any())
    assert (got_bits[7] == rows[7]).all()                                     # the inactive row is only read
    assert changed == B - 1
    # rows 1 and 3 have the same (normalised) penalties but their own counts; rows 0 and 3 the same raw presence / frequency:
    # the refused repetition penalty takes the whole entry to the identity
    ident, _ = LP.process_rows(rows[3:4], counts[3:4], tokens[3:4], n_tokens, 1.0, 0.0, 0.0, bias[3:4])
    if form != "grammar":
        assert (got_bits[3] == ident[0]).all()


# ------------------------------------------------------------------------------------------------------- the step
K_STEP, T_HOT = 4, 20.0      # a hot temperature: the tiny pair's logits are peaked, accept lengths vary at T = 20


def _pipe(drf, tgt, k=K_STEP, policy="longest_prefix", policy_params=None):
    from src.specdec import HipLM, SpeculativePipeline

    return SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=HipLM(drf.to("cuda")), controller="fixed",
                               controller_params={"k": k}, seed=1234, policy=policy, policy_params=policy_params)


def _session(prompts):
    from specdec_hip.engine import HipSpecDec

    drf, tgt = tiny_pair(flip_fraction=0.25)
    sess = _pipe(drf, tgt).start_session(prompts, 200, HipSpecDec.EMIT_BONUS, None)
    sess.loop.sync()
    return sess


def _prompts(n=4):
    return synthetic_prompts(n, 12, 1000).tolist()


def _records(loop, n, use_graph=True):
    out = []
    for _ in range(n):
        loop.step(use_graph=use_graph)
        r = loop.sync()
        out.append((r.accept_len.tolist(), r.new_tokens.tolist(), r.draft_tokens.tolist(), r.target_ids.tolist(), r.cur_len.tolist()))
    return out


def _set_mode(loop, mode, T, k, p, seed, sids, counters):
    if mode == "bonus":
        loop.set_sampling(True, T, k, p, seed, stream_ids=sids, draw_counts=counters)
    else:
        loop.set_spec_sampling(True, T, seed, stream_ids=sids, draw_counts=counters, top_k=k, top_p=p)


def _mode_off(loop, mode):
    loop.set_row_sampling(None)
    loop.set_sampling(False) if mode == "bonus" else loop.set_spec_sampling(False)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("mode,k,p", [("bonus", 50, 0.9), ("spec", None, None), ("spec", 50, 0.9)])
def test_uniform_table_is_the_scalar_mode(mode, k, p, use_graph):
    """A table whose every entry equals the loop's scalars: the records of 6 steps are those of the scalar mode, token for token."""
    prompts, seed, sids, counters = _prompts(), 4321, [3, 1, 2, 0], [5, 0, 9, 2]
    sess = _session(prompts)
    _set_mode(sess.loop, mode, T_HOT, k, p, seed, sids, counters)
    scalar = _records(sess.loop, 6, use_graph)
    scalar_draws = sess.loop.draw_counts
    _mode_off(sess.loop, mode)
    sess.finish()
    sess = _session(prompts)
    # the loop's own scalars are set to something else: with a table they are not in the launches
    _set_mode(sess.loop, mode, 1.0, 7 if k else None, None, 99, sids, counters)
    sess.loop.set_row_sampling([SamplingParams(T_HOT, k, p, seed)] * 4)
    rows = _records(sess.loop, 6, use_graph)
    assert rows == scalar
    assert sess.loop.draw_counts == scalar_draws
    _mode_off(sess.loop, mode)
    sess.finish()
    assert len({a for r in scalar for a in r[0]}) >= 2, [r[0] for r in scalar]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_uniform_penalty_table_is_the_scalar_stage(use_graph):
    """The logit-processor launches of a greedy step: a table whose every entry carries the stage's scalar penalties gives the
    records of the scalar stage; the loop's own (identity) scalars are not in the launches. The rows' counts hold what the
    unpenalised run emits, and the presence penalty is far above any logit, so the penalties are known to bite."""
    prompts = _prompts()
    rp, pres, freq = 1.5, 1000.0, 0.5

    def run(scalars, table, generated):
        sess = _session(prompts)
        loop = sess.loop
        loop.set_logit_processors(True, *scalars)
        for b, pr in enumerate(prompts):
            loop.set_logit_counts_row(b, pr, generated[b])
        if table is not None:
            loop.set_row_sampling(table)
        recs = _records(loop, 6, use_graph)
        loop.set_row_sampling(None)
        loop.set_logit_processors(False)
        sess.finish()
        return recs

    plain = run((1.0, 0.0, 0.0), None, [[]] * 4)
    emitted = [[t for r in plain for t in r[1][b] if t >= 0] for b in range(4)]
    scalar = run((rp, pres, freq), None, emitted)
    table = run((1.0, 0.0, 0.0), [SamplingParams(repetition_penalty=rp, presence_penalty=pres, frequency_penalty=freq)] * 4, emitted)
    assert table == scalar
    assert [r[1] for r in scalar] != [r[1] for r in plain]      # the penalties change what these rows emit


STEP_SEEDS, STEP_SIDS =[11, (7 << 32) | 3, 13, 14], [9, 4, 6, 1]
STEP_ROWS = {
    "bonus": [SamplingParams(temperature=0.0), SamplingParams(T_HOT, 50, 0.9), SamplingParams(T_HOT, None, 0.9), SamplingParams(T_HOT)],
    "spec": [SamplingParams(temperature=0.0), SamplingParams(T_HOT, 50, 0.9), SamplingParams(T_HOT), SamplingParams(10.0, 1024)],
}


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
@pytest.mark.parametrize("mode", ["bonus", "spec"])
def test_mixed_table_step_reproduces_the_per_row_restatement(mode, use_graph):
    """Every row's drafts, accept lengths and emitted tokens, step by step, from the restatement of that row's own parameters
    applied to THE DEVICE'S OWN stored q / p buffers (the method of test_step_reproduces_restatement_on_its_own_logits)."""
    K, V = K_STEP, 1000
    prompts = _prompts()
    params = [x.with_seed(STEP_SEEDS[b]) for b, x in enumerate(STEP_ROWS[mode])]
    sess = _session(prompts)
    loop = sess.loop
    counters = [5 * b for b in range(4)]
    _set_mode(loop, mode, 1.0, None, None, 0, STEP_SIDS, counters)
    loop.set_row_sampling(params)
    cur_len = [len(x) - 1 for x in prompts]
    close, lens = 0, []
    for step in range(6):
        loop.step(use_graph=use_graph)
        rec = loop.sync()
        p = loop.step_logits.float().cpu().numpy()
        for b in range(4):
            sc = params[b].scalars(spec=(mode == "spec"), vocab=V)
            if mode == "spec":
                q = loop.spec_draft_logits.float().cpu().numpy()
                d, res, emitted, c2, c = spec_row_ref(q[b], p[b], sc["temperature"], sc["top_k"], sc["top_p"], sc["seed"], counters[b], STEP_SIDS[b])
                close += c
                a = res.accept_len
                assert [int(x) for x in rec.draft_tokens[b]] == d, (step, b)
            else:
                d, t = [int(x) for x in rec.draft_tokens[b]], [int(np.argmax(p[b, i])) for i in range(K + 1)]
                a = 0
                while a < K and d[a] == t[a]:
                    a += 1
                tok, m = sample_ref(p[b, a], sc["temperature"], sc["top_k"], sc["top_p"], sc["seed"], counters[b], STEP_SIDS[b])
                close += int(m < CAP)
                emitted, c2 = d[:a] + [tok], counters[b] + 1
            assert int(rec.accept_len[b]) == a, (step, b)
            assert [int(x) for x in rec.new_tokens[b]] == emitted + [-1] * (K + 1 - len(emitted)), (step, b)
            cur_len[b] += len(emitted)
            assert int(rec.cur_len[b]) == cur_len[b], (step, b)
            counters[b] = c2
            lens.append(a)
        assert loop.draw_counts == counters, step
    assert close == 0       # (checked after the fact: the inputs are the device's own logits)
    assert len(set(lens)) >= 2, lens
    _mode_off(loop, mode)
    sess.finish()


def test_greedy_row_of_a_sampled_batch_is_the_greedy_run():
    """A T = 0 row under the sampled-bonus mode emits exactly what that row emits in a greedy run of the same four prompts."""
    prompts = _prompts()
    sess = _session(prompts)
    greedy = _records(sess.loop, 6)
    sess.finish()
    sess = _session(prompts)
    sess.loop.set_sampling(True, 1.0, None, None, 5)
    sess.loop.set_row_sampling([SamplingParams(T_HOT, 50, 0.9, 1), SamplingParams(0.0, seed=2), SamplingParams(T_HOT, seed=3),
                                SamplingParams(0.0, 40, 0.5, 4)])
    mixed = _records(sess.loop, 6)
    _mode_off(sess.loop, "bonus")
    sess.finish()
    for b in (1, 3):
        assert [(r[0][b], r[1][b], r[2][b], r[4][b]) for r in mixed] == [(r[0][b], r[1][b], r[2][b], r[4][b]) for r in greedy], b
    assert [r[1][0] for r in mixed] != [r[1][0] for r in greedy]      # the sampled rows do sample


def test_a_slot_is_rewritten_without_a_new_capture():
    prompts = _prompts()
    sess = _session(prompts)
    loop = sess.loop
    seed, sids = 77, [0, 1, 2, 3]
    loop.set_sampling(True, T_HOT, 50, 0.9, seed)
    _records(loop, 3)
    scalar_nodes = loop.graph_nodes
    assert scalar_nodes > 0
    params = [SamplingParams(T_HOT, 50, 0.9, seed + b) for b in range(4)]
    loop.set_row_sampling(params)
    assert loop.graph_nodes == 0                        # binding a table drops the captured step ...
    _records(loop, 3)                                   # ... (eager, capture, replay)
    _records(loop, 2)                                   # two replayed steps
    nodes = loop.graph_nodes
    assert nodes == scalar_nodes > 0                    # a row launch for every scalar launch
    # a new request in slot 2: its entry, stream id and draw counter, written on the loop's stream
    loop.set_row_params(2, SamplingParams(0.0, seed=5), stream_id=40, draw_count=0)
    new3 = SamplingParams(T_HOT, None, 0.9, 123)
    loop.set_row_params(3, new3, stream_id=41, draw_count=7)
    loop.step(use_graph=True)
    rec = loop.sync()
    assert loop.graph_nodes == nodes                    # the graph is kept
    p = loop.step_logits.float().cpu().numpy()
    a2, a3 = int(rec.accept_len[2]), int(rec.accept_len[3])
    assert int(rec.new_tokens[2][a2]) == int(np.argmax(p[2, a2]))       # slot 2 follows the new entry: greedy
    tok, m = sample_ref(p[3, a3], T_HOT, None, 0.9, 123, 7, 41)
    assert m >= CAP and int(rec.new_tokens[3][a3]) == tok                # slot 3: the new nucleus entry, stream and counter
    assert loop.draw_counts[2:] == [1, 8] and loop.stream_ids == [0, 1, 40, 41]
    entry = unpack(loop.row_table)[3]
    assert (entry.temperature, entry.top_k, entry.seed_lo) == (T_HOT, 0, 123) and abs(entry.top_p - 0.9) < 1e-7
    loop.set_row_sampling(None)
    assert loop.graph_nodes == 0
    _records(loop, 3)
    assert loop.graph_nodes == scalar_nodes             # back on the scalars: the scalar mode's node count
    _mode_off(loop, "bonus")
    sess.finish()


def test_engine_refusals():
    from specdec_hip import _abi

    sess = _session(_prompts())
    loop = sess.loop
    with pytest.raises(_abi.HipLibraryError, match="neither a sampling mode nor the logit-processor stage"):
        loop.set_row_sampling([SamplingParams()] * 4)
    with pytest.raises(ValueError, match="3 entries for 4 rows"):
        loop.set_row_sampling([SamplingParams()] * 3)
    with pytest.raises(RuntimeError, match="no table is bound"):
        loop.set_row_params(0, SamplingParams())
    loop.set_sampling(True, 1.0, None, None, 0)
    table = _table([_rec()] * 5)
    rc = loop.lib.sd_specdec_set_row_sampling(loop.handle, table.data_ptr() + 8)
    assert rc != 0 and "16-byte aligned" in _abi.last_error()
    loop.set_logit_processors(True)                     # the stage alone is enough for a table
    loop.set_sampling(False)
    loop.set_row_sampling([SamplingParams(repetition_penalty=1.2)] * 4)
    _records(loop, 2)
    loop.set_row_sampling(None)
    loop.set_logit_processors(False)
    sess.finish()


# ------------------------------------------------------------------------------------------------------- the pipeline
def test_generate_many_admits_requests_with_their_own_parameters(monkeypatch):
    from src.specdec.core import pipeline as P

    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(5, 12, 1000).tolist()
    params = [SamplingParams(temperature=0.0), SamplingParams(T_HOT, 50, 0.9, seed=21), SamplingParams(T_HOT, seed=22, presence_penalty=0.5),
              SamplingParams(temperature=0.0, repetition_penalty=1.2), SamplingParams(T_HOT, None, 0.9)]
    seen = []
    admit = P.DecodeSession.admit

    def spy(self, b, prompt, grammar_start=-1, params=None, index=None):
        nodes = self.loop.graph_nodes
        admit(self, b, prompt, grammar_start, params=params, index=index)
        entry = unpack(self.loop.row_table)[b]                       # (reads the device: everything enqueued has run)
        seen.append((index, prompt, bytes(entry), self.loop.stream_ids[b], self.row_ids[b], self.loop.draw_counts[b], nodes,
                     self.loop.graph_nodes, self.processors is not None))
    monkeypatch.setattr(P.DecodeSession, "admit", spy)
    # every call that drops the captured step, counted: an admit must make none
    from specdec_hip.engine import HipSpecDec

    drops = {}
    for name in ("set_sampling", "set_spec_sampling", "set_row_sampling", "set_logit_processors", "set_grammar", "invalidate"):
        def counted(self, *a, _f=getattr(HipSpecDec, name), _n=name, **kw):
            drops[_n] = drops.get(_n, 0) + 1
            return _f(self, *a, **kw)
        monkeypatch.setattr(HipSpecDec, name, counted)
    pipe = _pipe(drf, tgt)
    out = pipe.generate_many(prompts, max_tokens=16, batch_size=2, sampling_params=params, seed=1234)
    assert [len(r["generated_tokens"]) >= 1 for r in out] == [True] * 5
    assert drops == {"set_sampling": 1, "set_row_sampling": 1, "set_logit_processors": 1}, drops      # the session's start, nothing after
    assert sorted(s[0] for s in seen) == [2, 3, 4]                   # three requests were admitted to a freed slot
    for index, prompt, entry, sid, row_id, draws, nodes0, nodes1, lp in seen:
        assert prompt == prompts[index]
        assert entry == bytes(params[index].with_seed(1234).record()), index      # the slot's entry is the request's, seed included
        assert sid == row_id == index and draws == 0                 # stream id = the prompt's index
        assert nodes1 == nodes0 > 0                                  # admitting captured nothing again
        assert lp                                                    # requests with penalties switched the stage on
    again = pipe.generate_many(prompts, max_tokens=16, batch_size=2, sampling_params=params, seed=1234)
    assert [r["generated_tokens"] for r in again] == [r["generated_tokens"] for r in out]
    # the greedy requests' tokens are those of the same call with every request greedy
    all_greedy = [SamplingParams(temperature=0.0, repetition_penalty=x.repetition_penalty, presence_penalty=x.presence_penalty) for x in params]
    ref = pipe.generate_many(prompts, max_tokens=16, batch_size=2, sampling_params=all_greedy, seed=1234)
    for i in (0, 3):
        assert out[i]["generated_tokens"] == ref[i]["generated_tokens"], i
    assert any(out[i]["generated_tokens"] != ref[i]["generated_tokens"] for i in (1, 2, 4))
    # what a request samples does not depend on its slot: another batch size, the same tokens
    wide = pipe.generate_batch(prompts, max_tokens=16, sampling_params=params, seed=1234)
    assert [len(r["generated_tokens"]) >= 1 for r in wide] == [True] * 5


def test_pipeline_refusals():
    drf, tgt = tiny_pair(flip_fraction=0.25)
    prompts = synthetic_prompts(2, 12, 1000).tolist()
    ps = [SamplingParams(0.7, 50), SamplingParams(0.0)]
    pipe = _pipe(drf, tgt)
    for kw, err, msg in (({"do_sample": True}, ValueError, "do_sample"), ({"top_k": 5}, ValueError, "top_k"), ({"top_p": 0.5}, ValueError, "top_p"),
                         ({"repetition_penalty": 1.1}, ValueError, "repetition_penalty"), ({"presence_penalty": 0.1}, ValueError, "presence_penalty"),
                         ({"frequency_penalty": 0.1}, ValueError, "frequency_penalty")):
        for call in (pipe.generate_batch, pipe.generate_many):
            with pytest.raises(err, match=msg):
                call(prompts, max_tokens=8, sampling_params=ps, **kw)
    with pytest.raises(ValueError, match="1 entries for 2 prompts"):
        pipe.generate_batch(prompts, max_tokens=8, sampling_params=ps[:1])
    with pytest.raises(TypeError, match="SamplingParams"):
        pipe.generate_batch(prompts, max_tokens=8, sampling_params=[{"temperature": 1.0}, ps[1]])
    with pytest.raises(NotImplementedError, match="generate_batch and generate_many"):
        pipe.generate(prompts[0], max_tokens=8, sampling_params=ps[:1])
    with pytest.raises(NotImplementedError, match="host loop"):
        _pipe(drf, tgt, policy="typical").generate_batch(prompts, max_tokens=8, sampling_params=ps)
    with pytest.raises(NotImplementedError, match="host loop"):
        _pipe(drf, tgt, policy="rejection", policy_params={"temperature": 1.0}).generate_batch(prompts, max_tokens=8, sampling_params=ps)
    from src.specdec import HipLM, SpeculativePipeline

    adaptive = SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=HipLM(drf.to("cuda")), controller="adaptive", seed=1, policy="longest_prefix")
    with pytest.raises(NotImplementedError, match="fixed K"):
        adaptive.generate_batch(prompts, max_tokens=8, sampling_params=ps)
    eagle = SpeculativePipeline(base_lm=HipLM(tgt.to("cuda")), draft_lm=HipLM(drf.to("cuda")), controller="fixed", controller_params={"k": 4},
                                seed=1, policy="longest_prefix", draft_mode="eagle")
    with pytest.raises(NotImplementedError, match="medusa / eagle"):
        eagle.generate_batch(prompts, max_tokens=8, sampling_params=ps)
    # speculative sampling: the table under policy="rejection", backend="device"; the full-vocabulary nucleus stays refused there
    spec = _pipe(drf, tgt, policy="rejection", policy_params={"backend": "device", "temperature": T_HOT, "seed": 3})
    with pytest.raises(NotImplementedError, match="without top_k"):
        spec.generate_batch(prompts, max_tokens=8, sampling_params=[SamplingParams(1.0, None, 0.9), ps[1]])
    a = spec.generate_batch(prompts, max_tokens=12, sampling_params=[SamplingParams(T_HOT, 50, 0.9), SamplingParams(0.0)])
    b = spec.generate_batch(prompts, max_tokens=12, sampling_params=[SamplingParams(T_HOT, 50, 0.9), SamplingParams(0.0)])
    g = spec.generate_batch(prompts, max_tokens=12, sampling_params=[SamplingParams(0.0), SamplingParams(0.0)])
    assert [r["generated_tokens"] for r in a] == [r["generated_tokens"] for r in b]
    assert a[1]["generated_tokens"] == g[1]["generated_tokens"]       # the greedy request next to a sampled one
