"""sd_model_score's refusals through the C-ABI (no device work: a model is created over placeholder pointers and never bound), and
the perplexity arithmetic of src.benchmarks.quality_eval over a stub scorer."""

import ctypes
import math

import pytest
import torch

from specdec_hip import _abi
from specdec_hip.engine import _LayerWeights, _ModelConfig


def _model(d_model=128, packed=True):
    """an unbound sd_model over placeholder addresses (sd_model_create only records them)"""
    lib = _abi.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    layers = (_LayerWeights * 1)()
    for f, _ in _LayerWeights._fields_:
        setattr(layers[0], f, p)
    mc = _ModelConfig(arch=0, n_layers=1, d_model=d_model, n_heads=2, n_kv_heads=1, head_dim=64, d_ff=256, vocab=1000, max_pos=512,
                      norm_eps=1e-5, weight_dtype=_abi.SD_BF16, tok_emb=p, pos_emb=None, final_norm_w=p, final_norm_b=None, lm_head=p,
                      rope_cos=p, rope_sin=p, layers=layers, packed=p if packed else None)
    h = ctypes.c_void_p()
    _abi.check(lib.sd_model_create(ctypes.byref(mc), ctypes.byref(h)), "sd_model_create")
    return lib, h, (buf, layers)


def _score(lib, h, n=8, tokens=16, row=0, pos0=0):
    return lib.sd_model_score(h, tokens, n, row, pos0, None, None, None)


def test_score_is_exported():
    assert "sd_model_score" in _abi.SIGNATURES and hasattr(_abi.load(), "sd_model_score")


@pytest.mark.parametrize("case,msg", [
    ("null_model", "NULL model"),
    ("null_tokens", "NULL tokens"),
    ("n_one", "n=1"),
    ("n_zero", "n=0"),
    ("no_pack", "packed"),
    ("d_model", "multiple of 64"),
    ("unbound", "not bound"),
])
def test_score_refusals(case, msg):
    lib, h, keep = _model(d_model=72 if case == "d_model" else 128, packed=case != "no_pack")
    try:
        if case == "null_model":
            rc = _score(lib, None)
        elif case == "null_tokens":
            rc = _score(lib, h, tokens=None)
        elif case == "n_one":
            rc = _score(lib, h, n=1)
        elif case == "n_zero":
            rc = _score(lib, h, n=0)
        else:
            rc = _score(lib, h)
        assert rc != 0
        assert msg in _abi.last_error(), _abi.last_error()
        assert _abi.last_error().startswith("score:")
    finally:
        lib.sd_model_destroy(h)


class _Stub:
    """encode: one id per character; score: the log-probs it is given"""

    def __init__(self, logprob=None, fail=None):
        self.logprob, self.fail, self.seen = logprob, fail, []

    def encode(self, text):
        return torch.tensor([ord(c) % 100 for c in text])

    def score(self, ids):
        self.seen.append(list(ids))
        if self.fail:
            raise RuntimeError(self.fail)
        n = len(ids)
        lp = self.logprob if self.logprob is not None else [-math.log(2.0 + i) for i in range(n - 1)]
        return torch.tensor(lp[: n - 1], dtype=torch.float32), torch.zeros(n, dtype=torch.int32)


def _evaluator(stub, **kw):
    from src.benchmarks.quality_eval import PerplexityEvaluator

    return PerplexityEvaluator("synthetic:test", device="cuda", model=stub, **kw)


def test_perplexity_is_exp_of_the_mean_nll():
    stub = _Stub()
    r = _evaluator(stub).calculate_perplexity("abcde")
    lp = torch.tensor([-math.log(2.0 + i) for i in range(4)], dtype=torch.float32).double()
    loss = -float(lp.mean())
    assert r["loss"] == pytest.approx(loss, rel=1e-12) and r["perplexity"] == pytest.approx(math.exp(loss), rel=1e-12)
    assert r["token_count"] == 5 and r["text_length"] == 5 and r["model"] == "synthetic:test" and r["device"] == "cuda"
    assert set(r) == {"perplexity", "loss", "text_length", "token_count", "model", "device"}


def test_truncation_to_max_length():
    stub = _Stub()
    r = _evaluator(stub, max_length=7).calculate_perplexity("x" * 20)
    assert r["token_count"] == 7 and len(stub.seen[0]) == 7


def test_error_path():
    r = _evaluator(_Stub(fail="device lost")).calculate_perplexity("abc")
    assert r["perplexity"] == float("inf") and r["loss"] == float("inf") and r["token_count"] == 0 and "device lost" in r["error"]
    r = _evaluator(_Stub()).calculate_perplexity("a")   # one token: nothing to predict
    assert r["perplexity"] == float("inf") and "error" in r


def test_compare_texts_statistics():
    ev = _evaluator(_Stub(logprob=[-1.0] * 50))
    out = ev.compare_texts(["ab", "abc", "z"], labels=["two", "three", "bad"])
    assert [r["label"] for r in out["results"]] == ["two", "three", "bad"]
    st = out["statistics"]
    assert st["count"] == 2 and st["avg_perplexity"] == pytest.approx(math.e) and st["min_perplexity"] == pytest.approx(math.e)
    assert st["max_perplexity"] == pytest.approx(math.e)
    assert out["results"][2]["perplexity"] == float("inf")
    assert _evaluator(_Stub(fail="x")).compare_texts(["ab"])["statistics"] == {
        "avg_perplexity": float("inf"), "min_perplexity": float("inf"), "max_perplexity": float("inf"), "count": 0}
    assert [r["label"] for r in ev.compare_texts(["ab", "cd"])["results"]] == ["text_0", "text_1"]


def test_run_specdec_perplexity_of_generated_tokens():
    from src.specdec.run_specdec import generated_perplexity, parse_args

    assert parse_args(["--prompt", "1 2", "--eval-perplexity"]).eval_perplexity
    assert not parse_args(["--prompt", "1 2"]).eval_perplexity
    stub = _Stub(logprob=[-0.5, -1.5, -1.0])
    ppl, loss = generated_perplexity(stub, [5, 6, 7, 8])
    assert loss == pytest.approx(1.0) and ppl == pytest.approx(math.e) and stub.seen == [[5, 6, 7, 8]]
    assert generated_perplexity(stub, [5]) == (float("inf"), float("inf"))
