"""sd_model_score (csrc/score_head.hip): per-token log-probs and greedy ids of a sequence, against the logits path, against fp64,
across the prefill routes, and its cache / determinism contract. One-layer and toy models only.

Bounds (derived, not fitted):
  * Logits path. Both paths round the same fp32 product to bf16; they differ in the fp32 summation order of the product and of the
    final norm's statistic, which moves a logit by at most one bf16 spacing (at the row's largest |l|, sp). log-sum-exp is
    1-Lipschitz in the max-norm, so logprob = l_t - lse moves by at most 2 sp, plus the fp32 evaluation of the reduction (lse_eval).
  * fp64. head_stage gives each logit's bound B_i around the fp64 value; the same argument gives B_t + max_i B_i + lse_eval.
  * lse_eval: the kernel folds (max, sum) pairs in fp32; each fold is two expf (2^-22 relative each), a multiply and an add, so
    4 * 2^-23 relative on the sum per fold, over RF (<= 4) rows per lane + 4 lane folds + 1 wave fold + ceil(blocks / 256) + 8
    tree folds + 1 for log; then lse = M + log S and l_t - lse round once each (2^-24 of |lse| and |logprob|).
"""

import dataclasses
import math

import pytest
import torch

import stage_ref as R
from helpers import synthetic_prompts
from specdec_hip import _abi
from specdec_hip import weights as W
from specdec_hip.engine import HipModel
from test_hip_stage_fp64_gpu import GPT2, S1B_V, S3B, TOY, TOY128, _matrices, _weights

pytestmark = pytest.mark.gpu

GPT2_ODD = dataclasses.replace(GPT2, vocab=513, name="gpt2-layer-odd-vocab")   # n_pairs = 257: the pad row of the head is skipped
TOY1 = dataclasses.replace(TOY, n_layers=1, name="toy-d64-1l")


def _lse_eval(lse, logprob, n_blocks):
    folds = 4 + 4 + 1 + math.ceil(n_blocks / 256) + 8 + 1
    return folds * 4 * 2.0 ** -23 + 2.0 ** -24 * (lse.abs() + logprob.abs())


def _ref_logprob(logits, targets):
    """fp64 log-softmax of [n][V] logits at the targets -> (logprob [n], lse [n])"""
    l = logits.to(torch.float64)
    lse = torch.logsumexp(l, dim=-1)
    return l.gather(1, targets.view(-1, 1)).view(-1) - lse, lse


def _engine(cfg, wd="bf16", batch=2, l_max=1280, backend="passes", page_len=None):
    return HipModel(_weights(cfg), batch=batch, l_max=l_max, weight_dtype=wd, prefill_backend=backend, page_len=page_len)


def _seq(cfg, n, seed=5):
    return synthetic_prompts(1, n, cfg.vocab, seed=seed)[0].to(torch.int32)


@pytest.mark.parametrize("cfg,wd", [(TOY1, "bf16"), (TOY1, "fp8"), (TOY128, "bf16"), (GPT2_ODD, "bf16")],
                         ids=["llama-bf16", "llama-fp8", "toy128", "gpt2-odd-vocab"])
def test_score_matches_the_logits_path(cfg, wd):
    n = 40
    eng = _engine(cfg, wd)
    seq = _seq(cfg, n)
    dev = seq.to("cuda").view(1, -1)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    ids, logits = eng.forward(dev, zero, 0, want_logits=True, row0=0)
    lp, greedy = eng.score(seq, row=1)
    torch.cuda.synchronize()
    l = logits[0].double()
    ref, lse = _ref_logprob(l[:-1], seq[1:].long().cuda())
    sp = R.bf16_spacing(l.abs().amax(dim=1))
    bound = 2 * sp[:-1] + _lse_eval(lse, ref, cfg.vocab // 64 + 1)
    err = (lp.double() - ref).abs()
    assert bool((err <= bound).all()), f"worst {float((err / bound).max()):.2f} x the bound"
    top2 = l.topk(2, dim=1).values
    clear = (top2[:, 0] - top2[:, 1]) > sp
    assert bool((greedy.long()[clear] == l.argmax(dim=1)[clear]).all())
    assert bool((greedy < cfg.vocab).all())


@pytest.mark.parametrize("wd", ["bf16", "fp8"])
def test_score_against_fp64(wd):
    cfg, n = TOY1, 100
    mw = _weights(cfg)
    eng = _engine(cfg, wd)
    seq = _seq(cfg, n, seed=9)
    lp, greedy = eng.score(seq)
    x = eng.hidden_rows(n).double()
    ref_l, bnd = R.head_stage(cfg, mw, _matrices(mw, wd)["head"], x, R.chain_hip)
    tgt = seq[1:].long().cuda()
    ref, lse = _ref_logprob(ref_l[:-1], tgt)
    bound = bnd[:-1].gather(1, tgt.view(-1, 1)).view(-1) + bnd[:-1].amax(dim=1) + _lse_eval(lse, ref, cfg.vocab // 64 + 1)
    err = (lp.double() - ref).abs()
    assert bool((err <= bound).all()), f"worst {float((err / bound).max()):.2f} x the bound"


@pytest.mark.parametrize("wd", ["bf16", "fp8"])
@pytest.mark.parametrize("n", [95, 96, 128, 129, 511, 512, 513, 1100])
def test_native_route(n, wd):
    """The native route: the expected backend ran, the last chunk's positions match the fp64 head over the hidden rows it leaves,
    and the whole sequence stays close to the passes' scores (their residual rows differ in summation order only)."""
    cfg = TOY1
    mw = _weights(cfg)
    seq = _seq(cfg, n, seed=n)
    nat = _engine(cfg, wd, batch=1, backend="native")
    lp_n, g_n = nat.score(seq)
    assert nat.prefill_counts() == {"passes": 0, "rocblas": 0, "native": 1 if n >= 96 else 0}
    pas = _engine(cfg, wd, batch=1, backend="passes")
    lp_p, g_p = pas.score(seq)
    assert pas.prefill_counts()["passes"] == (1 if n >= 96 else 0)
    # the rows the route leaves: the last chunk's last <= 128 (native), the last pass (n < 96)
    k = min((n - 1) % 512 + 1, 128) if n >= 96 else (n - 1) % nat.pass_tokens + 1
    x = nat.hidden_rows(k).double()
    ref_l, bnd = R.head_stage(cfg, mw, _matrices(mw, wd)["head"], x, R.chain_hip)
    tail = torch.arange(n - k, n - 1, device="cuda")
    tgt = seq.cuda().long()[tail + 1]
    ref, lse = _ref_logprob(ref_l[:-1], tgt)
    bound = bnd[:-1].gather(1, tgt.view(-1, 1)).view(-1) + bnd[:-1].amax(dim=1) + _lse_eval(lse, ref, cfg.vocab // 64 + 1)
    err = (lp_n.double()[tail] - ref).abs()
    assert bool((err <= bound).all()), f"worst {float((err / bound).max()):.2f} x the bound"
    assert float((lp_n - lp_p).abs().mean()) < 0.05 and float((g_n == g_p).float().mean()) > 0.9


def test_cache_contract_and_determinism():
    cfg, n = TOY1, 300
    seq = _seq(cfg, n, seed=3)
    dense = _engine(cfg, "bf16", backend="native")
    paged = _engine(cfg, "bf16", backend="native", page_len=64)
    a = dense.score(seq)
    b = dense.score(seq)
    c = paged.score(seq)
    for u, v in ((a, b), (a, c)):
        assert torch.equal(u[0], v[0]) and torch.equal(u[1], v[1])
    # continuation: the tail scored after the head of the sequence is cached
    cut = 200
    dense.score(seq[:cut], row=1)
    lp_t, g_t = dense.score(seq[cut:], row=1, pos0=cut)
    assert torch.equal(g_t, a[1][cut:])
    err = (lp_t.double() - a[0][cut:].double()).abs()
    assert float(err.max()) < 0.05
    # a greedy step after score gives the token a forward of the same prompt gives
    eng = _engine(cfg, "bf16")
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    ids_f, _ = eng.forward(seq[:64].cuda().view(1, -1), zero, 0, row0=0)
    _, g = eng.score(seq[:64], row=1)
    assert int(g[-1]) == int(ids_f[0, -1])
    pos = torch.tensor([64], dtype=torch.int32, device="cuda")
    nxt0, _ = eng.forward(ids_f[:, -1:].contiguous(), pos, 0, row0=0)
    nxt1, _ = eng.forward(g[-1:].view(1, 1).contiguous(), pos, 0, row0=1)
    assert int(nxt0[0, 0]) == int(nxt1[0, 0])


@pytest.mark.parametrize("wd", ["bf16", "fp8"])
@pytest.mark.parametrize("cfg", [S1B_V, dataclasses.replace(S3B, vocab=128256, name="3b-layer-fullvocab")], ids=["1b", "3b"])
def test_full_lm_head_shape(cfg, wd):
    n = 512
    eng = _engine(cfg, wd, batch=1, l_max=n + 64, backend="native")
    seq = _seq(cfg, n, seed=2)
    lp, greedy = eng.score(seq)
    mw = _weights(cfg)
    k = 128
    x = eng.hidden_rows(k).double()
    ref_l, bnd = R.head_stage(cfg, mw, _matrices(mw, wd)["head"], x, R.chain_hip)
    tgt = seq.cuda().long()[n - k + 1:]
    ref, lse = _ref_logprob(ref_l[:-1], tgt)
    bound = bnd[:-1].gather(1, tgt.view(-1, 1)).view(-1) + bnd[:-1].amax(dim=1) + _lse_eval(lse, ref, cfg.vocab // 64 + 1)
    err = (lp.double()[n - k:] - ref).abs()
    assert bool((err <= bound).all()), f"worst {float((err / bound).max()):.2f} x the bound"
    assert bool((greedy >= 0).all()) and bool((greedy < cfg.vocab).all())
    del eng
    torch.cuda.empty_cache()


def test_refusals_on_the_device(monkeypatch):
    cfg = TOY1
    mw = _weights(cfg)
    monkeypatch.setenv("SPECDEC_NO_PACK", "1")
    rm = HipModel(dataclasses.replace(mw, meta={}), batch=1, l_max=256)
    monkeypatch.delenv("SPECDEC_NO_PACK")
    with pytest.raises(_abi.HipLibraryError, match="packed"):
        rm.score(_seq(cfg, 8))
    eng = _engine(cfg)
    with pytest.raises(_abi.HipLibraryError, match="row"):
        eng.score(_seq(cfg, 8), row=2)
    with pytest.raises(_abi.HipLibraryError, match="positions"):
        eng.score(_seq(cfg, 8), pos0=1275)
    seq = _seq(cfg, 8).cuda()
    s = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    lp = torch.empty(7, device="cuda")
    gr = torch.empty(8, dtype=torch.int32, device="cuda")
    rc = None
    with torch.cuda.stream(s):
        g.capture_begin()
        try:
            rc = eng.lib.sd_model_score(eng.handle, seq.data_ptr(), 8, 0, 0, lp.data_ptr(), gr.data_ptr(), s.cuda_stream)
        finally:
            try:
                g.capture_end()
            except RuntimeError:   # an empty capture may be refused by the runtime; the refusal above is what is tested
                pass
    assert rc != 0 and "capturing" in _abi.last_error()
