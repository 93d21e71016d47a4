"""The fixed-geometry instances of csrc/gemv.hip against the generic kernel, bit for bit.

A fixed instance has the work split of its matrix class compiled in; sums, rounding points and the thread -> item map are the
generic kernel's, so every output must be EQUAL, not close: no tolerance appears in this file. SPECDEC_GEMV_GENERIC=1 (read
at every launch) forces the generic kernel, which gives both paths in one process. That both are RIGHT is what the existing
suites check against independent references (test_hip_fullshape_parity_gpu.py, test_full_size_gpu.py, the fp64 stage checks).

Models: one layer, vocabulary 1024 (a small head), the real layer dimensions of Llama-3.2-1B and 3B — the geometry is a function
of (row pairs, K), so a narrower matrix would run another instance — dense KV and one paged case, plain random weights. The
"short-last" model has dimensions at which the LAST workgroup of the QKV, out and gate / up launches owns fewer pairs than
the others (2688 = 244 x 11 + 4, 1408 = 234 x 6 + 4, 8184 = 255 x 32 + 24 pairs) while the class is still a fixed one.
The "8b" model runs the three 8B classes; its down-projection (K = 14336) is the generic MASK kernel up to 5 tokens and a
csrc/gemm_skinny.hip body above (the 7-token context pass and the 9-token pass), on both sides of the switch."""

import dataclasses

import pytest
import torch

from specdec_hip import weights as W
from specdec_hip.ops import gemv_instance, gemv_variant

pytestmark = pytest.mark.gpu

TOKENS = (1, 2, 3, 5, 9)
CTX = 7                     # positions in the cache before the compared passes: they start at a non-zero position


def _one_layer(base, **kw):
    return dataclasses.replace(base, n_layers=1, vocab=1024, max_pos=256, tie_embeddings=True, **kw)


MODELS = {
    # name: (config, page_len)
    "1b": (_one_layer(W.LLAMA_3_2_1B), None),
    "3b": (_one_layer(W.LLAMA_3_2_3B), None),
    "3b-paged": (_one_layer(W.LLAMA_3_2_3B), 32),
    "8b": (_one_layer(W.LLAMA_3_8B), None),
    "short-last": (_one_layer(W.LLAMA_3_2_3B, d_model=2816, n_heads=28, n_kv_heads=7, head_dim=128, d_ff=8184, rope_scaling=None), None),
}
_weights = {}


def _model_weights(name):
    cfg = MODELS[name][0]
    key = (cfg.d_model, cfg.d_ff)
    if key not in _weights:
        _weights[key] = W.random_init(cfg, seed=cfg.d_model, device="cuda")
    return _weights[key]


def _variants(hm, T):
    out = []
    for which in range(4):
        _, K, n_pairs, epi, pro = hm.matrix_shape(which)
        out.append(gemv_variant(T, n_pairs, K, False, pro, epi))
    return out


def _down_instance(hm, T):
    """the kernel the down-projection really runs (sd_gemv_instance; sd_gemv_variant names the launcher's family)"""
    _, K, n_pairs, epi, pro = hm.matrix_shape(3)
    return gemv_instance(T, n_pairs, K, False, pro, epi)


def _run(name, generic, monkeypatch):
    """every observable of the passes: stage rows, ids, then the whole K and V caches"""
    from specdec_hip.engine import HipModel

    monkeypatch.setenv("SPECDEC_NO_PERSIST", "1")       # the launch path at 1 and 2 tokens too
    if generic:
        monkeypatch.setenv("SPECDEC_GEMV_GENERIC", "1")
    else:
        monkeypatch.delenv("SPECDEC_GEMV_GENERIC", raising=False)
    cfg, page_len = MODELS[name]
    hm = HipModel(_model_weights(name), batch=1, l_max=64, page_len=page_len)
    g = torch.Generator().manual_seed(11)
    toks = torch.randint(0, cfg.vocab, (1, CTX + sum(TOKENS)), generator=g).to(torch.int32).cuda()
    seen, names, down = [], {}, {}
    pos = 0
    for T in (CTX,) + TOKENS:
        names[T] = _variants(hm, T)
        down[T] = _down_instance(hm, T)
        ids, _ = hm.forward(toks[:, pos:pos + T].contiguous(), torch.tensor([pos], dtype=torch.int32, device="cuda"), 0,
                            skip_head=(pos == 0))
        for which in (hm.DEBUG_X, hm.DEBUG_Q, hm.DEBUG_ATTN, hm.DEBUG_ACT):
            seen.append((f"T={T} stage {which}", hm.debug_rows(which, T).cpu()))
        if ids is not None:
            seen.append((f"T={T} ids", ids.cpu()))
        pos += T
    torch.cuda.synchronize()
    seen.append(("k cache", hm.k_cache.cpu()))
    seen.append(("v cache", hm.v_cache.cpu()))
    return seen, names, down


@pytest.mark.parametrize("name", list(MODELS))
def test_fixed_instances_equal_the_generic_kernel_bit_for_bit(name, monkeypatch):
    want, names_generic, down_generic = _run(name, True, monkeypatch)
    got, names_fixed, down_fixed = _run(name, False, monkeypatch)
    # the fixed path is what ran: every layer launch of every pass names a fixed instance (the down-projection of the
    # short-last model has K = 8184, no whole 32-k slices: a MASK shape, generic on both sides)
    for T, names in names_fixed.items():
        assert all(n.startswith("fixed<") for n in names[:3]), (name, T, names)
        assert names[3].startswith("fixed<") or name in ("short-last", "8b"), (name, T, names)
    if name == "8b":    # the down-projection: the generic MASK kernel while T rows of 14336 fit the LDS, the hand-over above
        for down in (down_fixed, down_generic):
            assert down == {T: "generic<resid,mask,tt9,bf16,kb12>" if T <= 5 else "skinny:direct<tg1>" for T in (CTX,) + TOKENS}, down
    assert all(n == "generic" for names in names_generic.values() for n in names)
    assert len(got) == len(want)
    for (what, a), (_, b) in zip(got, want):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a, b.view(torch.int16) if b.dtype == torch.bfloat16 else b), (name, what)
    # and the passes did something: the cache holds the appended rows, the stages are not all zero
    assert all(t.float().abs().sum() > 0 for what, t in got if "stage" in what or "cache" in what)


def test_the_flagship_verify_pass_runs_fixed_instances(monkeypatch):
    """the 5-token pass of the 3B target: the four instances by name, and 'generic' under the switch"""
    from specdec_hip.engine import HipModel

    monkeypatch.delenv("SPECDEC_GEMV_GENERIC", raising=False)
    hm = HipModel(_model_weights("3b"), batch=1, l_max=64)
    assert _variants(hm, 5) == ["fixed<qkv,ks8,tp5,rmsnorm,tt5,kb6>", "fixed<resid,ks16,tp6,none,tt5,kb6>",
                                "fixed<swiglu,ks4,tp8,rmsnorm,tt5,kb12>", "fixed<resid,ks16,tp6,none,tt5,kb12>"]
    monkeypatch.setenv("SPECDEC_GEMV_GENERIC", "1")
    assert _variants(hm, 5) == ["generic"] * 4


def test_adaptive_k_skipping_draft_launches(monkeypatch):
    """Per-row adaptive K inside the captured step: draft forwards the row does not need leave at kernel entry (skip_k), in the
    fixed instances as in the generic kernel. An untrained draft is almost never accepted, so k falls to 1 and forwards 1..3
    are skipped; tokens, counters and the k trace of the two paths are equal."""
    from helpers import synthetic_prompts
    from src.specdec import HipLM, SpeculativePipeline

    monkeypatch.setenv("SPECDEC_NO_PERSIST", "1")       # the draft's 1- and 2-token passes on the launch path
    drf, tgt = _model_weights("1b"), _model_weights("3b")
    params = {"initial_k": 3, "min_k": 1, "max_k": 4, "step_size": 1, "target_acceptance_rate": 0.6, "per_row": True}
    prompts = synthetic_prompts(1, 9, 1024, seed=3).tolist()
    runs = []
    for generic in (True, False):
        if generic:
            monkeypatch.setenv("SPECDEC_GEMV_GENERIC", "1")
        else:
            monkeypatch.delenv("SPECDEC_GEMV_GENERIC")
        pipe = SpeculativePipeline(base_lm=HipLM(tgt), draft_lm=HipLM(drf), controller="adaptive", controller_params=dict(params), seed=1234)
        r = pipe.generate_batch(prompts, max_tokens=20, do_sample=False)[0]
        runs.append((r["generated_tokens"], r["proposed"], r["accepted"], r["k_trace"]))
    assert runs[0] == runs[1]
    assert min(runs[1][3]) < 4, "no step ran with k below the loop's K: no launch was skipped"
