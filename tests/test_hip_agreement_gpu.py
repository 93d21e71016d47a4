"""Draft-target agreement on the device: the op (sd_spec_agreement, csrc/spec_agree.hip) against its numpy float64 restatement
(tests/agreement_ref.py), the scoring head that keeps a chunk's logits (sd_model_score_logits) against sd_model_score, and
SpeculativePipeline.draft_agreement / run_specdec --eval-agreement over both.

Bounds. alpha and kl are compared within agreement_ref.bounds: a formula of the case's V, max |x/T|, max |a_v|, max |b_v| and
sum |exp(a_v)(a_v - b_v)| — float64 unit roundoff for the arguments, one ulp per exp / log, V u for a sum of V terms in any
order (derivation in tests/agreement_ref.py). For the cases here it must come out <= 1e-9 on alpha and <= 1e-9 (1 + kl) on kl,
which the test asserts of the bound itself. Argmax ids and `agree` are compared exactly.

score_logits against score: the stored rows are the logits score reduces, so greedy is equal exactly and logprob differs from a
float64 log_softmax of the stored rows only by score's fp32 evaluation of the log-sum-exp: _lse_eval of tests/test_hip_score_gpu.py
(a few fp32 ulp per fold of its fixed reduction tree, plus one rounding each of lse and of l_t - lse).
"""

import json
import math

import numpy as np
import pytest
import torch

import agreement_ref as A
from helpers import TINY_TARGET, synthetic_prompts, tiny_pair
from specdec_hip import _abi, ops
from specdec_hip.engine import HipModel
from test_hip_score_gpu import _lse_eval

pytestmark = pytest.mark.gpu


def _bf16(x):
    return torch.as_tensor(np.asarray(x, dtype=np.float32)).to(torch.bfloat16)


def _rows(V, n, seed):
    """target rows ~ N(0, 3), draft rows their 0.5-noise neighbours (the scale of _op_case, tests/test_hip_spec_shape_gpu.py)"""
    rng = np.random.default_rng(seed)
    p = _bf16(rng.normal(0, 3.0, (n, V)))
    q = _bf16(p.float().numpy() + rng.normal(0, 0.5, (n, V)))
    return p, q


def _check(p, q, T, got, label):
    """device outputs of target rows p / draft rows q (bf16 [n][V], on the host) against the restatement"""
    alpha, kl, agree, p_arg, q_arg = [t.cpu().numpy() for t in got]
    pn, qn = p.float().numpy(), q.float().numpy()
    worst_a = worst_k = worst_ba = worst_bk = 0.0
    for t, r in enumerate(A.agreement_ref(pn, qn, T)):
        assert (int(p_arg[t]), int(q_arg[t]), bool(agree[t])) == (r.p_arg, r.q_arg, r.agree), (label, t)
        if math.isnan(r.alpha):
            assert math.isnan(alpha[t]) and math.isnan(kl[t]), (label, t)
            continue
        b_alpha, b_kl = A.bounds(pn[t], qn[t], T)
        assert b_alpha <= 1e-9, (label, t, b_alpha)
        worst_a, worst_ba = max(worst_a, abs(alpha[t] - r.alpha)), max(worst_ba, b_alpha)
        assert abs(alpha[t] - r.alpha) <= b_alpha, (label, t, alpha[t], r.alpha, b_alpha)
        if math.isinf(r.kl):
            assert kl[t] == r.kl, (label, t)
            continue
        assert b_kl <= 1e-9 * (1 + r.kl), (label, t, b_kl)
        worst_k, worst_bk = max(worst_k, abs(kl[t] - r.kl) / (1 + r.kl)), max(worst_bk, b_kl / (1 + r.kl))
        assert abs(kl[t] - r.kl) <= b_kl, (label, t, kl[t], r.kl, b_kl)
    print(f"{label}: worst |alpha - ref| {worst_a:.3e} (bound {worst_ba:.3e}), worst |kl - ref| / (1 + kl) {worst_k:.3e} (bound {worst_bk:.3e})")


@pytest.mark.parametrize("V,n,T", [(100, 1, 1.0), (100, 5, 0.7), (4099, 5, 2.5), (4099, 130, 1.0), (50257, 1, 2.5), (50257, 5, 0.7),
                                   (128256, 5, 2.5), (128256, 130, 1.0)])
def test_op_matches_the_restatement(V, n, T):
    p, q = _rows(V, n, seed=V + n)
    got = ops.spec_agreement(q.cuda(), p.cuda(), T)
    _check(p, q, T, got, f"V={V} n={n} T={T}")
    again = ops.spec_agreement(q.cuda(), p.cuda(), T)
    for a, b in zip(got, again):                       # run-to-run bit identity (NaN-free cases: torch.equal compares values)
        assert torch.equal(a, b)


def test_strided_rows_three_dimensional_blocks_and_alignment_independence():
    V, n, T = 4099, 6, 0.7
    p, q = _rows(V, n, seed=1)
    wide_p = torch.zeros((n, V + 5), dtype=torch.bfloat16, device="cuda")
    wide_q = torch.zeros((n, V + 3), dtype=torch.bfloat16, device="cuda")
    wide_p[:, 3:3 + V] = p.cuda()                      # rows start 6 bytes into rows that are themselves an odd number of bytes apart
    wide_q[:, 1:1 + V] = q.cuda()
    got = ops.spec_agreement(wide_q[:, 1:1 + V], wide_p[:, 3:3 + V], T)
    _check(p, q, T, got, "strided V=4099")
    dense = ops.spec_agreement(q.cuda(), p.cuda(), T)
    for a, b in zip(got, dense):                       # a thread owns the same elements in the same order on either load path
        assert torch.equal(a, b)
    blk = ops.spec_agreement(q.cuda().view(2, 3, V), p.cuda().view(2, 3, V), T)
    for a, b in zip(blk, dense):
        assert a.shape == (2, 3) and torch.equal(a.reshape(-1), b)


def test_row_independence_and_equal_blocks():
    V, n = 50257, 130
    p, q = _rows(V, n, seed=2)
    pc, qc = p.cuda(), q.cuda()
    full = ops.spec_agreement(qc, pc, 0.7)
    alone = ops.spec_agreement(qc[3:4].clone(), pc[3:4].clone(), 0.7)
    for a, b in zip(full, alone):
        assert torch.equal(a[3:4], b)
    alpha, kl, agree, p_arg, q_arg = ops.spec_agreement(pc, pc.clone(), 0.7)
    assert bool((kl == 0.0).all()) and bool(agree.all()) and torch.equal(p_arg, q_arg)
    b_alpha = max(A.bounds(p[t].float().numpy(), p[t].float().numpy(), 0.7)[0] for t in (0, 64, 129))
    assert float((alpha - 1.0).abs().max()) <= b_alpha


def test_tied_maxima_and_special_rows():
    inf, nan = float("inf"), float("nan")
    V = 5000                                           # two slices: the special entries sit in either
    grid = np.round(np.random.default_rng(4).normal(0, 2.0, (8, V)) * 2) / 2      # a coarse grid: many exact ties
    p, q = _bf16(grid), _bf16(grid)
    top = float(grid.max()) + 1.0
    p[0, 17], p[0, 4500] = top, top                    # row 0: the target's maximum twice, the draft's once at the later index
    q[0, 4500] = top
    q[1] = _bf16(np.roll(grid[1], 7))                  # row 1: the same values elsewhere
    p[2, 4200] = nan                                   # row 2: a NaN on the target's side
    q[3, 9], q[3, 4100] = nan, nan                     # row 3: NaNs on the draft's side, the first one is its argmax
    p[4, 4097] = inf                                   # row 4: +inf on top
    q[5, :] = -inf                                     # row 5: a row of -inf
    q[6, 100:300] = -inf                               # row 6: -inf entries in q only: kl = +inf, alpha finite
    p[7, 100:300] = -inf                               # row 7: -inf entries in p only: both finite
    got = ops.spec_agreement(q.cuda(), p.cuda(), 1.0)
    _check(p, q, 1.0, got, "special rows")
    alpha, kl, agree, p_arg, q_arg = [t.cpu() for t in got]
    assert (int(p_arg[0]), int(q_arg[0]), bool(agree[0])) == (17, 4500, False)
    assert int(p_arg[2]) == 4200 and int(q_arg[3]) == 9 and int(p_arg[4]) == 4097 and int(q_arg[5]) == 0
    assert all(math.isnan(float(alpha[t])) and math.isnan(float(kl[t])) for t in (2, 3, 4, 5))
    assert float(kl[6]) == inf and 0.0 < float(alpha[6]) < 1.0 and math.isfinite(float(kl[7])) and float(kl[7]) > 0.0


def test_capture_replays_to_the_same_bits():
    V, n, T = 50257, 5, 0.7
    p, q = _rows(V, n, seed=6)
    pc, qc = p.cuda(), q.cuda()
    eager = ops.spec_agreement(qc, pc, T)
    lib = _abi.load()
    alpha = torch.zeros(n, dtype=torch.float64, device="cuda")
    kl = torch.zeros(n, dtype=torch.float64, device="cuda")
    ints = torch.zeros((3, n), dtype=torch.int32, device="cuda")
    ws = torch.empty(lib.sd_spec_agreement_workspace(n, V), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = lib.sd_spec_agreement(qc.data_ptr(), V, pc.data_ptr(), V, n, V, T, alpha.data_ptr(), kl.data_ptr(), ints[0].data_ptr(),
                                   ints[1].data_ptr(), ints[2].data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, _abi.last_error()
    for _ in range(2):
        alpha.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(alpha, eager[0]) and torch.equal(kl, eager[1]) and torch.equal(ints[0] != 0, eager[2])
        assert torch.equal(ints[1], eager[3]) and torch.equal(ints[2], eager[4])


def test_op_refusals():
    z = torch.zeros((2, 8), dtype=torch.bfloat16, device="cuda")
    with pytest.raises(TypeError, match="bfloat16"):
        ops.spec_agreement(z.float(), z)
    with pytest.raises(ValueError, match="shape"):
        ops.spec_agreement(z, z[:, :4])
    with pytest.raises(_abi.HipLibraryError, match="temperature"):
        ops.spec_agreement(z, z, 0.0)


# ------------------------------------------------------------------------------------------------ the scoring head with logits
@pytest.fixture(scope="module")
def pair():
    drf, tgt = tiny_pair(flip_fraction=0.25)
    return drf.to("cuda"), tgt.to("cuda")


def _seq(n, seed=5):
    return synthetic_prompts(1, n, TINY_TARGET.vocab, seed=seed)[0].to(torch.int32)


@pytest.mark.parametrize("page_len", [None, 64], ids=["dense", "paged64"])
@pytest.mark.parametrize("wd", ["bf16", "fp8"])
@pytest.mark.parametrize("n", [5, 150])
def test_score_logits_is_score_with_the_logits_kept(pair, n, wd, page_len):
    _, tgt = pair
    seq = _seq(n, seed=n)
    a = HipModel(tgt, batch=1, l_max=256, weight_dtype=wd, prefill_backend="native", page_len=page_len)
    b = HipModel(tgt, batch=1, l_max=256, weight_dtype=wd, prefill_backend="native", page_len=page_len)
    lp, greedy = a.score(seq)
    logits, greedy_l = b.score_logits(seq)
    torch.cuda.synchronize()
    assert logits.shape == (n, TINY_TARGET.vocab) and logits.dtype == torch.bfloat16
    assert torch.equal(greedy_l, greedy) and torch.equal(logits.float().argmax(dim=1).to(torch.int32), greedy)
    ls = torch.log_softmax(logits.double(), dim=-1)
    ref = ls[:-1].gather(1, seq[1:].long().cuda().view(-1, 1)).view(-1)
    lse = torch.logsumexp(logits.double(), dim=-1)[:-1]
    err = (lp.double() - ref).abs()
    bound = _lse_eval(lse, ref, TINY_TARGET.vocab // 64 + 1)
    print(f"n={n} {wd}: worst |logprob - log_softmax(stored rows)| {float(err.max()):.3e}, {float((err / bound).max()):.2f} x the bound")
    assert bool((err <= bound).all())
    assert torch.equal(a.k_cache, b.k_cache) and torch.equal(a.v_cache, b.v_cache)
    assert a.prefill_counts() == b.prefill_counts() == {"passes": 0, "rocblas": 0, "native": 1 if n >= 96 else 0}


def test_score_logits_continues_a_row_and_fills_a_buffer(pair):
    _, tgt = pair
    seq = _seq(12, seed=8)
    eng = HipModel(tgt, batch=2, l_max=64)
    whole, g = eng.score_logits(seq, row=0)
    buf = torch.zeros((16, TINY_TARGET.vocab), dtype=torch.bfloat16, device="cuda")
    eng.score_logits(seq[:8], row=1)
    tail, g_t = eng.score_logits(seq[8:], row=1, pos0=8, out=buf)
    assert tail.data_ptr() == buf.data_ptr() and tail.shape == (4, TINY_TARGET.vocab) and bool((buf[4:] == 0).all())
    assert torch.equal(g_t, g[8:])
    one, g1 = eng.score_logits(seq[:1], row=1)          # a single token is enough for logits
    assert one.shape == (1, TINY_TARGET.vocab) and int(g1[0]) == int(g[0])
    with pytest.raises(_abi.HipLibraryError, match="row"):
        eng.score_logits(seq, row=2)
    with pytest.raises(ValueError, match="out must be"):
        eng.score_logits(seq, out=buf[:4])


# --------------------------------------------------------------------------------------------------------------- the pipeline
def _pipe(pair, **kw):
    from src.specdec import HipLM, SpeculativePipeline

    drf, tgt = pair
    return SpeculativePipeline(base_lm=HipLM(tgt), draft_lm=HipLM(drf), controller="fixed", controller_params={"k": 2}, seed=1234, **kw)


def test_draft_agreement_of_the_target_with_itself(pair):
    from src.specdec import HipLM, SpeculativePipeline

    _, tgt = pair
    pipe = SpeculativePipeline(base_lm=HipLM(tgt), draft_lm=HipLM(tgt), controller="fixed", controller_params={"k": 2}, seed=1234)
    seq = _seq(20, seed=3).tolist()
    r = pipe.draft_agreement(seq, temperature=0.7)
    logits, _ = pipe.base_lm.score_logits(seq[:-1])
    b_alpha = max(A.bounds(row, row, 0.7)[0] for row in logits.float().cpu().numpy())
    assert len(r["alpha"]) == len(r["kl"]) == len(r["agree"]) == r["positions"] == 19
    assert all(k == 0.0 for k in r["kl"]) and all(r["agree"]) and max(abs(a - 1.0) for a in r["alpha"]) <= b_alpha
    assert r["greedy_agreement"] == 1.0 and r["mean_kl"] == 0.0
    assert r["expected_tokens_per_step"]["greedy"] == {K: float(K + 1) for K in range(1, 9)}
    assert all(abs(r["expected_tokens_per_step"]["sampling"][K] - (K + 1)) <= (K + 1) * K * b_alpha for K in range(1, 9))


def test_draft_agreement_is_the_op_over_the_two_score_logits(pair):
    pipe = _pipe(pair)
    seq = _seq(40, seed=4).tolist()
    r = pipe.draft_agreement(seq, temperature=1.0)
    q, _ = pipe.draft_lm.score_logits(seq[:-1])
    p, _ = pipe.base_lm.score_logits(seq[:-1])
    alpha, kl, agree, _, _ = ops.spec_agreement(q, p, 1.0)
    assert r["alpha"] == alpha.cpu().tolist() and r["kl"] == kl.cpu().tolist() and r["agree"] == agree.cpu().tolist()
    assert 0.0 < r["mean_alpha"] < 1.0 and r["mean_kl"] > 0.0
    assert r["mean_alpha"] == pytest.approx(sum(r["alpha"]) / 39) and r["greedy_agreement"] == sum(r["agree"]) / 39
    for kind, xs in (("sampling", r["alpha"]), ("greedy", [1.0 if x else 0.0 for x in r["agree"]])):
        for K in range(1, 9):
            assert r["expected_tokens_per_step"][kind][K] == pytest.approx(A.expected_tokens_loop(xs, K), rel=1e-12)
    _check(p.cpu(), q.cpu(), 1.0, ops.spec_agreement(q, p, 1.0), "tiny pair, 39 positions")


def test_draft_agreement_chunks_and_refusals(pair):
    pipe = _pipe(pair)
    seq = _seq(9, seed=6).tolist()
    small, large = pipe.draft_agreement(seq, chunk=4), pipe.draft_agreement(seq, chunk=256)
    assert small == large and small["positions"] == 8
    assert pipe.draft_agreement(" ".join(str(t) for t in seq), chunk=256) == large       # text of a synthetic model: its ids
    with pytest.raises(ValueError, match="at least 2"):
        pipe.draft_agreement(seq[:1])
    with pytest.raises(ValueError, match="temperature"):
        pipe.draft_agreement(seq, temperature=0.0)
    from src.specdec import HipLM, SpeculativePipeline

    with pytest.raises(NotImplementedError, match="fake"):
        SpeculativePipeline(implementation="fake").draft_agreement(seq)
    _, tgt = pair
    for mode in ("medusa", "eagle"):
        self_draft = SpeculativePipeline(base_lm=HipLM(tgt), draft_model="none", draft_mode=mode, seed=1234)
        with pytest.raises(NotImplementedError, match=mode):
            self_draft.draft_agreement(seq)


def test_run_specdec_eval_agreement_prints_json(pair, capsys, monkeypatch):
    from src.specdec import run_specdec
    from src.specdec.models import hip_lm

    drf, tgt = pair
    made = {"synthetic:tiny-target": tgt, "synthetic:tiny-draft": drf}
    real = hip_lm.create_hip_lm
    monkeypatch.setattr("src.specdec.core.pipeline.create_hip_lm", lambda spec, **kw: real(made[spec], **kw))
    rc = run_specdec.main(["--prompt", "5 6 7 8", "--max-tokens", "12", "--K", "2", "--base-model", "synthetic:tiny-target",
                           "--draft-model", "synthetic:tiny-draft", "--eval-agreement", "--temperature", "0.7"])
    assert rc == 0
    out = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert {"agreement_alpha", "agreement_kl", "agreement_greedy", "expected_tokens_per_step", "acceptance_rate"} <= set(out)
    assert 0.0 < out["agreement_alpha"] <= 1.0 and out["agreement_kl"] >= 0.0 and 0.0 <= out["agreement_greedy"] <= 1.0
    assert sorted(out["expected_tokens_per_step"]["sampling"]) == sorted(str(K) for K in range(1, 9))
    assert 1.0 <= out["expected_tokens_per_step"]["greedy"]["4"] <= 5.0
