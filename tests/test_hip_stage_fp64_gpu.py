"""Every stage of the HIP forward against a plain fp64 computation of the same operation, within bounds derived from the
arithmetic (tests/stage_ref.py), on one-layer `random_init` models (no damped layers).

Each case runs one pass and checks, from the bf16 values the kernels read: norm + QKV + RoPE (q tap, new K / V rows of the
cache), attention (q tap + cache), out-projection + residual, norm + gate / up + SwiGLU or gelu_new (activation tap),
down-projection + residual (hidden rows) and final norm + lm_head (logits). The reference does not share code or
summation order with any HIP path, so it sees faults the path-against-path tests cannot. The worst error of every stage
as a fraction of its bound is printed (run with -s)."""

import dataclasses
import random

import pytest
import torch

import stage_ref as R
from specdec_hip import weights as W
from specdec_hip.engine import HipModel, prefill_backends_available
from stage_check import cache_rows as _cache_rows, check_pass as _check_pass, matrices as _matrices  # noqa: F401  (other files take them from here)

pytestmark = pytest.mark.gpu

LL = W.ARCH_LLAMA


def _llama(name, d, hq, hkv, D, ff, vocab=512, max_pos=4096, scaling=None):
    return W.ModelConfig(arch=LL, n_layers=1, d_model=d, n_heads=hq, n_kv_heads=hkv, head_dim=D, d_ff=ff, vocab=vocab,
                         max_pos=max_pos, rope_theta=500000.0, rope_scaling=scaling, tie_embeddings=False, name=name)


L3 = {"factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192, "rope_type": "llama3"}
TINY = _llama("tiny-d32", 128, 4, 2, 32, 256, scaling={"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                                         "original_max_position_embeddings": 64, "rope_type": "llama3"})
TOY = _llama("toy-d64", 256, 4, 2, 64, 512)
TOY128 = _llama("toy-d128", 384, 3, 1, 128, 1024)
S1B = _llama("1b-layer", 2048, 32, 8, 64, 8192, scaling=L3)
S1B_V = _llama("1b-layer-fullvocab", 2048, 32, 8, 64, 8192, vocab=128256, scaling=L3)
S3B = _llama("3b-layer", 3072, 24, 8, 128, 8192, scaling=L3)
S8B = _llama("8b-layer", 4096, 32, 8, 128, 14336)
GPT2 = W.ModelConfig(arch=W.ARCH_GPT2, n_layers=1, d_model=768, n_heads=12, n_kv_heads=12, head_dim=64, d_ff=3072, vocab=512,
                     max_pos=1024, tie_embeddings=False, name="gpt2-small-layer")

_MODELS = {}


def _weights(cfg):
    if cfg.name not in _MODELS:
        if cfg.d_model >= 2048 or any(m.config.d_model >= 2048 for m in _MODELS.values()):
            _MODELS.clear()           # one large model at a time
            torch.cuda.empty_cache()
        _MODELS[cfg.name] = W.random_init(cfg, seed=7, device="cuda")
    return _MODELS[cfg.name]


def _write_prefix(eng, row, n, gen, peaked=False, spikes=()):
    """random K / V at positions [0, n) of `row`, through kv_view (K x 32 for a peaked softmax; V x 256 in one channel at each
    of `spikes`)"""
    if n <= 0:
        return
    c = eng.cfg
    eng.reserve(row, n)
    pos = torch.arange(n, device=eng.device)
    kk = torch.randn(c.n_kv_heads, n, c.head_dim, generator=gen, device=eng.device).bfloat16()
    vv = torch.randn(c.n_kv_heads, n, c.head_dim, generator=gen, device=eng.device).bfloat16()
    if peaked:
        kk = kk * 32
    for j, s in enumerate(spikes):
        if 0 <= s < n:
            vv[:, s, (5 * j) % c.head_dim] *= 256
    k, v = eng.kv_view()
    if eng.page_len is None:
        k[0, row, :, :n] = kk
        v[0, row, :, :, :n] = vv.transpose(1, 2)
    else:
        P = eng.page_len
        pages = eng.block_table[row].long()[pos // P]
        k[0][pages, :, pos % P] = kk.transpose(0, 1)
        v[0][pages, :, :, pos % P] = vv.permute(1, 0, 2)


def _engine(mw, batch, l_max, weight_dtype="bf16", packed=True, page_len=None, backend="auto", monkeypatch=None):
    if not packed:   # row-major weights: a view of the weights without the packed copy another engine made
        monkeypatch.setenv("SPECDEC_NO_PACK", "1")
        mw = dataclasses.replace(mw, meta={})
    eng = HipModel(mw, batch=batch, l_max=l_max, weight_dtype=weight_dtype, page_len=page_len, prefill_backend=backend)
    if not packed:
        monkeypatch.delenv("SPECDEC_NO_PACK")
    assert (eng._packed is not None) == packed
    return eng


# (config, weight storage, packed, tokens per pass, first position, path): "persist" = the persistent launch,
# "launch" = the launch-per-operator path. Tokens per pass within what each model's kernels take (pass_tokens: 9 where
# gemm_skinny does not cover a matrix); fp8 storage where every K is a multiple of 64 (not the 384-wide toy, not GPT-2)
DECODE = [
    (TINY, "bf16", True, 1, 37, "launch"), (TINY, "bf16", True, 5, 40, "launch"), (TINY, "bf16", True, 17, 3, "launch"),
    (TINY, "fp8", True, 9, 70, "launch"), (TINY, "bf16", False, 16, 20, "launch"),
    (TOY, "bf16", True, 1, 100, "persist"), (TOY, "bf16", True, 2, 31, "persist"), (TOY, "bf16", True, 2, 31, "launch"),
    (TOY, "bf16", True, 9, 0, "launch"), (TOY, "bf16", True, 16, 64, "launch"), (TOY, "bf16", True, 40, 500, "launch"),
    (TOY, "bf16", True, 64, 1, "launch"), (TOY, "bf16", True, 128, 30, "launch"), (TOY, "fp8", True, 1, 200, "launch"),
    (TOY, "fp8", True, 17, 33, "launch"), (TOY, "fp8", True, 64, 300, "launch"), (TOY, "bf16", False, 5, 9, "launch"),
    (TOY, "bf16", False, 40, 47, "launch"),
    (TOY128, "bf16", True, 1, 513, "persist"), (TOY128, "bf16", True, 2, 90, "persist"), (TOY128, "bf16", True, 9, 0, "launch"),
    (S1B, "bf16", True, 1, 60, "persist"), (S1B, "bf16", True, 9, 60, "launch"), (S1B, "fp8", True, 64, 10, "launch"),
    (S1B_V, "bf16", True, 2, 5, "launch"),
    (S3B, "bf16", True, 5, 33, "launch"), (S3B, "fp8", True, 64, 0, "launch"), (S3B, "bf16", False, 9, 4, "launch"),
    (S8B, "bf16", True, 5, 17, "launch"), (S8B, "fp8", True, 2, 40, "launch"),
    (GPT2, "bf16", True, 1, 7, "launch"), (GPT2, "bf16", True, 5, 100, "launch"), (GPT2, "bf16", False, 9, 64, "launch"),
]


@pytest.mark.parametrize("cfg,wd,packed,M,pos0,path", DECODE,
                         ids=[f"{c.name}-{wd}-{'packed' if p else 'rowmajor'}-M{M}-p{p0}-{path}" for c, wd, p, M, p0, path in DECODE])
def test_decode_pass_stages(cfg, wd, packed, M, pos0, path, monkeypatch):
    mw = _weights(cfg)
    eng = _engine(mw, 1, pos0 + M + 64, wd, packed, monkeypatch=monkeypatch)
    if path == "launch":
        eng.set_persist_tokens(0)
    assert eng.persist_active(M) == (path == "persist")
    assert M <= eng.pass_tokens
    gen = torch.Generator(device="cuda").manual_seed(pos0 + M)
    _write_prefix(eng, 0, pos0, gen, spikes=(pos0 - 1, 31, 32))
    tok = torch.randint(4, cfg.vocab, (1, M), generator=gen, device="cuda", dtype=torch.int32)
    _, logits = eng.forward(tok, torch.tensor([pos0], dtype=torch.int32, device="cuda"), want_logits=True)
    positions = torch.arange(pos0, pos0 + M, device="cuda")
    _check_pass(eng, mw, _matrices(mw, wd), tok[0].long(), positions, torch.zeros(M, dtype=torch.long), logits[0],
                R.chain_hip, f"{cfg.name} {wd} M={M}")


def test_batched_ragged_rows(monkeypatch):
    """B = 8 rows x 5 tokens at ragged lengths, rows 2..9 of the bound batch: one 40-token pass"""
    mw = _weights(TOY)
    eng = _engine(mw, 10, 1200)
    gen = torch.Generator(device="cuda").manual_seed(3)
    pb = [0, 1, 31, 32, 63, 511, 512, 1000]
    for i, p in enumerate(pb):
        _write_prefix(eng, 2 + i, p, gen, spikes=(p - 1, 31, 511))
    tok = torch.randint(4, TOY.vocab, (8, 5), generator=gen, device="cuda", dtype=torch.int32)
    _, logits = eng.forward(tok, torch.tensor(pb, dtype=torch.int32, device="cuda"), want_logits=True, row0=2)
    positions = torch.tensor([p + m for p in pb for m in range(5)], device="cuda")
    rows = torch.tensor([2 + i for i in range(8) for _ in range(5)])
    _check_pass(eng, mw, _matrices(mw, "bf16"), tok.reshape(-1).long(), positions, rows, logits.reshape(40, -1), R.chain_hip,
                "toy B=8x5 ragged, row0=2")


# ---- attention at the edges: block (32 keys), split (512 keys: a workgroup per 512), pages, past 2048 -------------------------
ATTN = [(p, M, split, page, adv) for (p, M) in [(0, 5), (1, 5), (31, 1), (32, 1), (33, 5), (507, 5), (511, 1), (512, 2), (1023, 2), (2100, 5)]
        for (split, page, adv) in [(True, None, "spikes"), (False, None, "peaked"), (True, 32, "spikes"), (True, 64, "peaked")]]


@pytest.mark.parametrize("pos0,M,split,page,adv", ATTN,
                         ids=[f"p{p}-M{M}-{'split' if s else 'nosplit'}-{'dense' if pg is None else f'page{pg}'}-{a}" for p, M, s, pg, a in ATTN])
def test_attention_edges(pos0, M, split, page, adv, monkeypatch):
    cfg = TOY128 if pos0 in (33, 1023) else TOY
    mw = _weights(cfg)
    if not split:
        monkeypatch.setenv("SPECDEC_NO_ATTN_SPLIT", "1")
    eng = _engine(mw, 2, 2304 if pos0 > 1500 else 1280, page_len=page)
    eng.set_persist_tokens(0)
    if page is not None:            # pages handed out in a scrambled order
        random.Random(pos0).shuffle(eng._free)
    gen = torch.Generator(device="cuda").manual_seed(pos0 * 7 + M)
    spikes = (pos0 - 1, 31, 32, 63, 64, 511, 512, 1023, 1024) if adv == "spikes" else ()
    _write_prefix(eng, 1, pos0, gen, peaked=adv == "peaked", spikes=spikes)
    tok = torch.randint(4, cfg.vocab, (1, M), generator=gen, device="cuda", dtype=torch.int32)
    _, logits = eng.forward(tok, torch.tensor([pos0], dtype=torch.int32, device="cuda"), want_logits=True, row0=1)
    positions = torch.arange(pos0, pos0 + M, device="cuda")
    _check_pass(eng, mw, _matrices(mw, "bf16"), tok[0].long(), positions, torch.ones(M, dtype=torch.long), logits[0], R.chain_hip,
                f"{cfg.name} attention p{pos0} M={M} split={split} page={page} {adv}")


@pytest.mark.parametrize("M,pos0", [(5, 0), (5, 27), (128, 0)])
def test_in_pass_causality(M, pos0, monkeypatch):
    """query m sees the new keys <= m only: new V rows are not spikable, so the stale keys after the pass are (x 256 V at
    every position of the next 64) — a query that saw one would move by O(1)"""
    mw = _weights(TOY)
    eng = _engine(mw, 1, 256)
    eng.set_persist_tokens(0)
    gen = torch.Generator(device="cuda").manual_seed(M)
    _write_prefix(eng, 0, pos0 + M + 64, gen, spikes=tuple(range(pos0, pos0 + M + 64)))
    tok = torch.randint(4, TOY.vocab, (1, M), generator=gen, device="cuda", dtype=torch.int32)
    _, logits = eng.forward(tok, torch.tensor([pos0], dtype=torch.int32, device="cuda"), want_logits=True)
    positions = torch.arange(pos0, pos0 + M, device="cuda")
    _check_pass(eng, mw, _matrices(mw, "bf16"), tok[0].long(), positions, torch.zeros(M, dtype=torch.long), logits[0], R.chain_hip,
                f"toy in-pass causality M={M} p{pos0}")


# ---- prompt GEMMs ----------------------------------------------------------------------------------------------------------------
def _backend(name):
    if name not in prefill_backends_available():
        pytest.skip(f"prefill backend {name!r} is not available in this process ({prefill_backends_available()})")


def _prompt(eng, mw, backend, wd, L, pos0=0, row=0, B=1, gen=None, what=""):
    """a prompt of L positions (per row) at pos0 into rows [row, row + B): check the GEMM path ran, then the stages of the last
    chunk's last <= 128 positions of the last row"""
    cfg = mw.config
    before = eng.prefill_counts()[backend]
    tok = torch.randint(4, cfg.vocab, (B, L), generator=gen, device="cuda", dtype=torch.int32)
    eng.forward(tok, torch.full((B,), pos0, dtype=torch.int32, device="cuda"), row0=row)
    assert eng.prefill_counts()[backend] == before + B
    n = min(128, L - (L - 1) // 512 * 512)
    positions = torch.arange(pos0 + L - n, pos0 + L, device="cuda")
    chain = R.chain_rocblas if backend == "rocblas" else R.chain_hip
    return _check_pass(eng, mw, _matrices(mw, wd), tok[-1, L - n:].long(), positions, torch.full((n,), row + B - 1, dtype=torch.long),
                       None, chain, what)


PREFILL = [(b, cfg, wd, L) for b in ("native", "rocblas") for (cfg, wd, Ls) in
           [(TOY, "bf16", (96, 127, 128, 129, 300, 512, 513, 700)), (TOY, "fp8", (129, 513)), (S1B, "bf16", (300,)), (S1B, "fp8", (127,))]
           for L in Ls if not (b == "rocblas" and wd == "fp8")]


@pytest.mark.parametrize("backend,cfg,wd,L", PREFILL, ids=[f"{b}-{c.name}-{wd}-L{L}" for b, c, wd, L in PREFILL])
def test_prompt_gemm_stages(backend, cfg, wd, L):
    """1B dimensions at 300 positions take both row-block widths of the native GEMM (RB = 128 for gate / up, 64 for QKV)"""
    _backend(backend)
    mw = _weights(cfg)
    eng = HipModel(mw, batch=1, l_max=L + 32, weight_dtype=wd, prefill_backend=backend)
    _prompt(eng, mw, backend, wd, L, gen=torch.Generator(device="cuda").manual_seed(L), what=f"{backend} {cfg.name} {wd} L={L}")


@pytest.mark.parametrize("backend", ["native", "rocblas"])
def test_prompt_continues_after_prefix(backend):
    """a prompt at pos_base > 0 after a cached prefix, into row 1 (HipLM.generate_tokens), then a B = 2 prompt in one call
    (SpeculativePipeline._prefill)"""
    _backend(backend)
    mw = _weights(TOY)
    eng = HipModel(mw, batch=3, l_max=800, prefill_backend=backend)
    gen = torch.Generator(device="cuda").manual_seed(11)
    tok = torch.randint(4, TOY.vocab, (1, 200), generator=gen, device="cuda", dtype=torch.int32)
    eng.forward(tok, torch.zeros(1, dtype=torch.int32, device="cuda"), row0=1)
    _prompt(eng, mw, backend, "bf16", 150, pos0=200, row=1, gen=gen, what=f"{backend} continuation p200 L=150 row 1")
    _prompt(eng, mw, backend, "bf16", 97, pos0=0, row=1, B=2, gen=gen, what=f"{backend} B=2 L=97")


@pytest.mark.parametrize("backend", ["native", "rocblas"])
def test_debug_rows_after_prompt(backend):
    """q / attention / activation rows after a prompt are that prompt's (not those of an earlier decode-shaped pass): the
    same positions as hidden_rows"""
    _backend(backend)
    mw = _weights(TOY)
    eng = HipModel(mw, batch=1, l_max=512, prefill_backend=backend)
    gen = torch.Generator(device="cuda").manual_seed(5)
    eng.forward(torch.randint(4, TOY.vocab, (1, 40), generator=gen, device="cuda", dtype=torch.int32), torch.zeros(1, dtype=torch.int32, device="cuda"))
    tok = torch.randint(4, TOY.vocab, (1, 200), generator=gen, device="cuda", dtype=torch.int32)
    eng.forward(tok, torch.zeros(1, dtype=torch.int32, device="cuda"))
    got = [eng.debug_rows(w, 128) for w in (HipModel.DEBUG_Q, HipModel.DEBUG_ATTN, HipModel.DEBUG_ACT)]
    ref = HipModel(mw, batch=1, l_max=512, prefill_backend="passes")
    ref.set_persist_tokens(0)
    ref.forward(tok[:, :72], torch.zeros(1, dtype=torch.int32, device="cuda"))
    ref.forward(tok[:, 72:], torch.full((1,), 72, dtype=torch.int32, device="cuda"))       # the same last 128 positions, one pass
    for w, g in zip((HipModel.DEBUG_Q, HipModel.DEBUG_ATTN, HipModel.DEBUG_ACT), got):
        want = ref.debug_rows(w, 128).float()
        err = (g.float() - want).abs().max().item()
        assert err <= 2.0 ** -4 * want.abs().max().item(), (w, err)   # one model's rows, two summation orders (a wrong row is O(1) off)
