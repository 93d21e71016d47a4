"""The native prompt-prefill backend (SD_PREFILL_NATIVE: csrc/prefill_mfma.hip, an MFMA GEMM over the packed tile streams of
csrc/pack.hip, inside the chunked prefill driver of csrc/prefill_gemm.hip) against (a) the CPU oracle — over the dequantised
weights for fp8 storage —, (b) the 128-token passes at production layer shapes, (c) itself on a dense and a paged cache, and the
backend selection / reporting surface (HipModel.set_prefill_backend, prefill_counts).

Tolerances are those of tests/test_hip_prefill_gemm_gpu.py: the native GEMM only changes the fp32 summation order of the matrix
products; the bf16 rounding points are the fused epilogues' (the same kernels as every other path)."""

import dataclasses

import pytest
import torch

from helpers import synthetic_prompts
from oracle import fp8_ref
from oracle.model_ref import OracleLM
from specdec_hip import _abi
from specdec_hip import weights as W
from test_hip_persist_gpu import TOY, TOY128, _close, _dev, _shape_1b, _shape_3b

pytestmark = pytest.mark.gpu

# fp8 storage needs every K slice of the decode kernels' work split to be whole 64-k steps: TOY128's d_model of 384 is not
# (model_create refuses it), so its fp8 twin has d_model 512 (4 heads of 128)
TOY128_FP8 = dataclasses.replace(TOY128, d_model=512, n_heads=4, name="persist-toy128-fp8")


def _model(mw, l_max, backend="native", batch=1, **kw):
    from specdec_hip.engine import HipModel

    return HipModel(mw.to("cuda") if mw.tok_emb.device.type != "cuda" else mw, batch=batch, l_max=l_max, prefill_backend=backend, **kw)


def _toy(cfg, seed=3):
    return W.synthetic_llama(cfg, seed=seed, device="cpu", layer_gain=0.05)


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("cfg,L", [(TOY, 200), (TOY128, 333), (TOY, 700)], ids=["toy-200", "toy128-333", "toy-700-two-chunks"])
def test_native_prefill_matches_the_oracle(cfg, L, dtype):
    """Logits of the position after an L-token prompt absorbed by the native GEMM, against the bf16 oracle's full-prefix forward
    (over the dequantised weights for fp8 storage)."""
    if dtype == "fp8" and cfg is TOY128:
        cfg = TOY128_FP8
    mw = _toy(cfg)
    seq = synthetic_prompts(1, L + 1, cfg.vocab, seed=7)
    want, _ = OracleLM(fp8_ref.dequantized(mw) if dtype == "fp8" else mw, "bf16").forward(seq)
    hm = _model(mw, L + 64, weight_dtype=dtype)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    hm.forward(_dev(seq[:, :L]), zero, 0, skip_head=True)
    assert hm.prefill_counts() == {"passes": 0, "rocblas": 0, "native": 1}
    pos = torch.tensor([L], dtype=torch.int32, device="cuda")
    ids, got = hm.forward(_dev(seq[:, L:]), pos, 0, want_logits=True)
    w = want[0, L].float()
    g = got[0, 0].float().cpu()
    rng = (w.max() - w.min()).item()
    err = (g - w).abs()
    assert err.max().item() < 0.03 * rng and err.pow(2).mean().sqrt().item() < 0.015 * rng, (err.max().item() / rng, rng)
    top2 = w.topk(2).values
    if (top2[0] - top2[1]).item() > 2 * err.max().item():
        assert int(ids[0, 0]) == int(w.argmax())


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
@pytest.mark.parametrize("shape,L", [(_shape_1b(2), 300), (_shape_3b(2), 640)], ids=["1b-2l-300", "3b-2l-640-two-chunks"])
def test_native_prefill_matches_the_passes_at_production_shapes(shape, L, dtype):
    """The same prompt through the native GEMM and through the 128-token passes at the real layer dimensions: the caches they
    leave, the residual rows of the last positions, the ids of the prompt positions and the next position's logits."""
    mw = W.random_init(dataclasses.replace(shape, vocab=32000), seed=11, device="cuda")
    seq = synthetic_prompts(1, L + 1, 32000, seed=9)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    pos = torch.tensor([L], dtype=torch.int32, device="cuda")
    res = {}
    for backend in ("native", "passes"):
        hm = _model(mw, L + 64, backend, weight_dtype=dtype)
        ids_p, _ = hm.forward(_dev(seq[:, :L]), zero, 0)
        assert hm.prefill_counts()[backend] == 1
        # rows of the last pass: the native path leaves the last chunk's last <= 128, the passes their last pass (fp8: 64 tokens)
        cap = hm.pass_tokens
        hid = hm.hidden_rows(min(L, 128) if backend == "native" else (L - 1) % cap + 1)
        k, v = hm.kv_view()
        ids_n, lg = hm.forward(_dev(seq[:, L:]), pos, 0, want_logits=True)
        res[backend] = (ids_p.cpu(), hid.float().cpu(), k[:, :, :, :L].float().cpu(), v[:, :, :, :, :L].float().cpu(), ids_n.cpu(),
                        lg.float().cpu())
        del hm
    a, b = res["native"], res["passes"]
    n = min(a[1].shape[0], b[1].shape[0])
    _close(a[1][-n:], b[1][-n:], "residual rows of the last positions")
    _close(a[2], b[2], "K rows of the prompt")
    _close(a[3], b[3], "V rows of the prompt")
    _close(a[5], b[5], "logits of the next position", floor=b[5].abs().max().item() / 8)
    band = (a[5] - b[5]).abs().max().item()
    top2 = b[5][0, 0].topk(2).values
    if (top2[0] - top2[1]).item() > 2 * band:
        assert torch.equal(a[4], b[4])
    agree = (a[0] == b[0]).float().mean().item()
    assert agree > 0.97, f"only {agree:.3f} of the prompt positions' ids agree between the native GEMM and the passes"


@pytest.mark.parametrize("dtype", ["bf16", "fp8"])
def test_native_prefill_into_paged_kv_is_bit_identical_to_dense(dtype):
    """Native prefill into a paged cache (page_len 64, pages handed out in scrambled pool order) leaves exactly the K / V rows,
    residual rows and next logits of native prefill into a dense cache."""
    mw = _toy(TOY).to("cuda")
    L, P = 300, 64
    seq = synthetic_prompts(1, L + 1, TOY.vocab, seed=17)
    dense = _model(mw, 448, weight_dtype=dtype)
    dense.set_persist_tokens(0)           # the next-position pass of both models on the launch path (paged KV never takes the persistent one)
    paged = _model(mw, 448, weight_dtype=dtype, page_len=P, batch=2)
    assert paged.prefill_backend == "native"
    for n in range(1, 6):                 # rows 1 and 0 take pages in turn: row 0's pages are scattered over the pool
        for b in (1, 0):
            paged.reserve(b, n * P)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    pos = torch.tensor([L], dtype=torch.int32, device="cuda")
    out = {}
    for name, m in (("dense", dense), ("paged", paged)):
        m.forward(_dev(seq[:, :L]), zero, 0, skip_head=True)
        assert m.prefill_counts()["native"] == 1
        hid = m.hidden_rows(128).cpu()
        k, v = m.kv_view()
        if name == "paged":
            pages = paged.block_table[0, : (L + P - 1) // P].long()
            nl, _, hkv, _, d = k.shape
            kk = k[:, pages].permute(0, 2, 1, 3, 4).reshape(nl, hkv, -1, d)[:, :, :L]
            vv = v[:, pages].permute(0, 2, 3, 1, 4).reshape(nl, hkv, d, -1)[..., :L]
        else:
            kk, vv = k[:, 0, :, :L], v[:, 0, :, :, :L]
        _, lg = m.forward(_dev(seq[:, L:]), pos, 0, want_logits=True)
        out[name] = (kk.cpu(), vv.cpu(), hid, lg.cpu())
    assert paged.block_table[0, :5].tolist() != list(range(5))
    for a, b, what in zip(out["paged"], out["dense"], ("K rows", "V rows", "residual rows", "next logits")):
        assert torch.equal(a, b), what


def test_backend_selection_and_counts():
    """The selected backend absorbs a 300-token prompt and only its count moves; AUTO on fp8 storage takes the passes; a 64-token
    prompt is no prompt (nothing counts); backends that cannot serve a model are refused with the library's reason."""
    from specdec_hip.engine import HipModel, prefill_backends_available

    mw = _toy(TOY).to("cuda")
    seq = _dev(synthetic_prompts(1, 300, TOY.vocab, seed=5))
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    names = [b for b in ("passes", "rocblas", "native") if b in prefill_backends_available()]
    assert "native" in names and "passes" in names
    for backend in names:
        hm = _model(mw, 384, backend)
        assert hm.prefill_backend == backend
        hm.forward(seq[:, :64], zero, 0, skip_head=True)
        assert hm.prefill_counts() == {"passes": 0, "rocblas": 0, "native": 0}
        hm.forward(seq, zero, 0, skip_head=True)
        assert hm.prefill_counts() == {n: int(n == backend) for n in ("passes", "rocblas", "native")}, backend
    hm = _model(mw, 384, "auto", weight_dtype="fp8")
    assert hm.prefill_backend == "auto"
    hm.forward(seq, zero, 0, skip_head=True)
    assert hm.prefill_counts() == {"passes": 1, "rocblas": 0, "native": 0}
    hm.set_prefill_backend("native")
    assert hm.prefill_backend == "native"
    with pytest.raises(_abi.HipLibraryError, match="fp8"):
        hm.set_prefill_backend("rocblas")
    assert hm.prefill_backend == "native"                 # a refused choice changes nothing
    with pytest.raises(ValueError, match="prefill_backend"):
        hm.set_prefill_backend("cublas")
    g2 = W.ModelConfig(arch=W.ARCH_GPT2, n_layers=1, d_model=128, n_heads=2, n_kv_heads=2, head_dim=64, d_ff=512, vocab=512,
                       max_pos=256, tie_embeddings=True, name="gpt2-toy")
    gm = HipModel(W.synthetic_gpt2(g2, seed=1).to("cuda"), batch=1, l_max=128)
    with pytest.raises(_abi.HipLibraryError, match="GPT-2"):
        gm.set_prefill_backend("native")
    with pytest.raises(_abi.HipLibraryError, match="GPT-2"):
        HipModel(W.synthetic_gpt2(g2, seed=1).to("cuda"), batch=1, l_max=128, prefill_backend="native")


@pytest.mark.parametrize("paged", [False, True], ids=["dense", "paged"])
def test_native_prefill_feeds_the_step_loop_fp8(paged):
    """A 400-token prompt through the pipeline with fp8 storage and the native backend: both models absorb it with the native
    GEMM and the decoded tokens / counters are the oracle's over the dequantised weights (greedy, K = 4)."""
    from oracle.pipeline_ref import OraclePipeline
    from src.specdec import HipLM, SpeculativePipeline

    tcfg = dataclasses.replace(TOY, max_pos=1024)
    dcfg = dataclasses.replace(TOY, n_layers=1, d_model=128, n_heads=2, n_kv_heads=1, d_ff=256, max_pos=1024, name="persist-toy-draft")
    tgt = _toy(tcfg)
    drf = W.synthetic_llama(dcfg, seed=4, device="cpu", layer_gain=0.05, embed_from=tgt, flip_fraction=0.25)
    prompt = synthetic_prompts(1, 400, tcfg.vocab, seed=21)[0].tolist()
    want = OraclePipeline(OracleLM(fp8_ref.dequantized(tgt), "bf16"), OracleLM(fp8_ref.dequantized(drf), "bf16"), k=4).generate_batch([prompt], 24)[0]
    kw = dict(weight_dtype="fp8", prefill_backend="native", kv_page_len=64 if paged else None)
    pipe = SpeculativePipeline(base_lm=HipLM(tgt.to("cuda"), **kw), draft_lm=HipLM(drf.to("cuda"), **kw), controller="fixed",
                               controller_params={"k": 4}, seed=1234)
    got = pipe.generate_batch([prompt], max_tokens=24, do_sample=False)[0]
    assert got["generated_tokens"] == want["generated_tokens"]
    assert (got["proposed"], got["accepted"]) == (want["proposed"], want["accepted"])
    rt = next(iter(pipe._runtimes.values()))
    for role in ("target", "draft"):
        assert rt[role].prefill_counts()["native"] >= 1, role
        assert (rt[role].page_len is not None) == paged
