"""Every position of a GEMM-prefilled prompt against the fp64 stage references of tests/stage_ref.py, bounds unchanged.

A prompt chunk computes up to 512 positions, but the taps every other test reads (debug_rows, hidden_rows) hold the chunk's
last <= 128: one token block of the GEMM, the attention sub-pass with no future keys in the cache. sd_model_prefill_rows
serves any row of the last chunk out of the prefill workspace, so here every token block of all four products, every
attention sub-pass (with up to 384 keys of the queries' own future already appended) and, through the cache, the K / V
rows of every position of every chunk are held against an independent computation. Every native case first asserts the
plan it was chosen for (tests/prefill_cases.py; closure: tests/test_prefill_plan_cpu.py).

The worst error of every stage as a fraction of its bound and the wall time are printed (run with -s)."""

import dataclasses
import random
import time

import pytest
import torch

import prefill_cases as P
import stage_ref as R
from specdec_hip import _abi
from specdec_hip import weights as W
from specdec_hip.engine import HipModel
from test_hip_stage_fp64_gpu import _backend, _cache_rows, _check_pass, _matrices, _weights

pytestmark = pytest.mark.gpu

WHICH = (HipModel.DEBUG_X, HipModel.DEBUG_Q, HipModel.DEBUG_ATTN, HipModel.DEBUG_ACT)


def _chain(backend):
    return R.chain_rocblas if backend == "rocblas" else R.chain_hip


def _assert_plan(eng, model, wd, L):
    """the engine's own plan for every chunk size of the prompt is the pinned one"""
    for mc in sorted({min(P.CHUNK, L - m0) for m0 in range(0, L, P.CHUNK)}):
        plans = [eng.prefill_plan(w, mc) for w in range(4)]
        assert tuple(P.summary(p) for p in plans) == P.PINS[(model, mc)], (model, mc, plans)
        assert all(p.name == f"mfma<rf{p.rb // 32},{wd}>" for p in plans), plans


def _forward(eng, backend, tok, pos0, row):
    before = eng.prefill_counts()[backend]
    B = tok.shape[0]
    eng.forward(tok, torch.full((B,), pos0, dtype=torch.int32, device="cuda"), row0=row, skip_head=True)   # no prompt takes the lm_head
    assert eng.prefill_counts()[backend] == before + B


def _check_kv(eng, mw, mats, tok_row, pos0, n, row, chain, what, layer=0):
    """the K / V rows the cache holds for the first n positions of the prompt against qkv_stage from the embeddings"""
    c, lw = mw.config, mw.layers[layer]
    Hq, Hkv, D = c.n_heads, c.n_kv_heads, c.head_dim
    worst = {"k": 0.0, "v": 0.0}
    for g0 in range(0, n, 128):
        m = min(128, n - g0)
        positions = torch.arange(pos0 + g0, pos0 + g0 + m, device="cuda")
        x0, x0d = R.embed(c, mw, tok_row[g0:g0 + m].long(), positions)
        ref, bnd = R.qkv_stage(c, lw, mats["wqkv"], x0, x0d, positions, mw.rope_cos, mw.rope_sin, chain)
        k_r, v_r = _cache_rows(eng, row, positions, layer)
        kn = k_r.transpose(0, 1).reshape(m, Hkv * D)
        vn = v_r.transpose(0, 1).reshape(m, Hkv * D)
        worst["k"] = max(worst["k"], R.check(kn, (ref[:, Hq * D:(Hq + Hkv) * D], bnd[:, Hq * D:(Hq + Hkv) * D]), f"{what}: K rows {g0}.."))
        worst["v"] = max(worst["v"], R.check(vn, (ref[:, (Hq + Hkv) * D:], bnd[:, (Hq + Hkv) * D:]), f"{what}: V rows {g0}.."))
    return worst


def _check_prompt(eng, mw, mats, tok_row, pos0, L, row, chain, what, layer=0, x_in=None):
    """every stage of every position of the prompt's last chunk (in groups of 128 rows through prefill_rows), the K / V rows
    of every position of the chunks before it, and the last <= 128 rows bit for bit against debug_rows / hidden_rows.
    -> {stage: worst error / bound}"""
    m0 = (L - 1) // P.CHUNK * P.CHUNK
    Mc = L - m0
    worst = {}
    for r0 in range(0, Mc, 128):
        n = min(128, Mc - r0)
        positions = torch.arange(pos0 + m0 + r0, pos0 + m0 + r0 + n, device="cuda")
        res = _check_pass(eng, mw, mats, tok_row[m0 + r0:m0 + r0 + n].long(), positions, torch.full((n,), row, dtype=torch.long), None,
                          chain, f"{what} rows {r0}..{r0 + n - 1}", layer=layer, x_in=None if x_in is None else x_in[r0:r0 + n],
                          taps=lambda which, T, r0=r0: eng.prefill_rows(which, r0, T))
        for k, v in res.items():
            worst[k] = max(worst.get(k, 0.0), v)
    if m0 and x_in is None:
        for k, v in _check_kv(eng, mw, mats, tok_row, pos0, m0, row, chain, what, layer).items():
            worst[k] = max(worst[k], v)
    keep = min(128, Mc)
    for which in WHICH:
        tail = eng.prefill_rows(which, Mc - keep, keep)
        old = eng.hidden_rows(keep) if which == HipModel.DEBUG_X else eng.debug_rows(which, keep)
        assert torch.equal(tail, old), f"{what}: rows [{Mc - keep}, {Mc}) of stage {which} differ from the 128-row taps"
    assert torch.equal(eng.prefill_rows(HipModel.DEBUG_X, Mc - keep, keep), eng.debug_rows(HipModel.DEBUG_X, keep))
    with pytest.raises(RuntimeError, match="outside the"):
        eng.prefill_rows(HipModel.DEBUG_Q, Mc - 1, 2)
    assert eng.engine_status() == 0
    print(f"[prefill rows/bound] {what}: " + " ".join(f"{k} {v:.5f}" for k, v in worst.items()))
    assert all(v < 1.0 for v in worst.values()), worst       # strictly inside: a residual row's bound is mostly half a bf16 spacing
    return worst


def _tokens(cfg, B, L, gen):
    return torch.randint(4, cfg.vocab, (B, L), generator=gen, device="cuda", dtype=torch.int32)


def _run_case(case):
    t0 = time.perf_counter()
    _backend(case.backend)
    cfg = case.cfg
    mw = _weights(cfg)
    eng = HipModel(mw, batch=case.batch, l_max=case.pos0 + case.L + 32, weight_dtype=case.wd, page_len=case.page, prefill_backend=case.backend)
    if case.page is not None:
        random.Random(case.L).shuffle(eng._free)          # pages handed out in a scrambled order
    if case.backend == "native":
        _assert_plan(eng, case.model, case.wd, case.L)
    gen = torch.Generator(device="cuda").manual_seed(case.L + case.pos0)
    mats = _matrices(mw, case.wd)
    chain = _chain(case.backend)
    last = case.row + case.B - 1
    if case.pos0:                                            # the cached prefix: a prompt of its own into the same row
        pre = _tokens(cfg, 1, case.pos0, gen)
        _forward(eng, case.backend, pre, 0, last)
        _check_kv(eng, mw, mats, pre[0], 0, case.pos0, last, chain, f"{case.id} prefix")
    tok = _tokens(cfg, case.B, case.L, gen)
    _forward(eng, case.backend, tok, case.pos0, case.row)
    worst = _check_prompt(eng, mw, mats, tok[-1], case.pos0, case.L, last, chain, case.id)
    for b in range(case.B - 1):                              # the rows before the checked one: their K / V, every position
        _check_kv(eng, mw, mats, tok[b], case.pos0, case.L, case.row + b, chain, f"{case.id} row {case.row + b}")
    torch.cuda.synchronize()
    print(f"[prefill rows/time] {case.id}: {time.perf_counter() - t0:.2f} s")
    return eng, mw, tok, worst


@pytest.mark.parametrize("case", P.CASES, ids=[c.id for c in P.CASES])
def test_prompt_rows(case):
    _run_case(case)


@pytest.mark.parametrize("case", P.CONTINUATION + P.BATCHED, ids=[c.id for c in P.CONTINUATION + P.BATCHED])
def test_prompt_rows_continuation_and_batch(case):
    """a 512-position continuation at position 200 into row 1 of a 3-row cache (queries 200 .. 711: over the split-KV edge, every
    sub-pass with a prefix below it), and a B = 2 prompt whose record is the second row's"""
    _run_case(case)


def test_prompt_rows_paged_is_bit_identical_to_dense():
    """native prefill into scrambled 64-key pages: every row of all four stages equals the dense engine's bit for bit (and
    meets its bounds against the paged cache's own K / V)"""
    case = P.PAGED[0]
    paged, mw, tok, _ = _run_case(case)
    assert paged.block_table[0, :5].tolist() != sorted(paged.block_table[0, :5].tolist())
    dense = HipModel(mw, batch=1, l_max=case.L + 32, prefill_backend="native")
    _forward(dense, "native", tok, 0, 0)
    for which in WHICH:
        assert torch.equal(paged.prefill_rows(which, 0, case.L), dense.prefill_rows(which, 0, case.L)), which
    pos = torch.arange(case.L)
    for a, b in zip(_cache_rows(paged, 0, pos), _cache_rows(dense, 0, pos)):
        assert torch.equal(a, b)


def test_record_is_dropped_by_other_forwards_and_binds():
    """prefill_rows serves the last GEMM chunk only: refused before any prompt, after a decode-shaped pass, after a prompt the
    128-token passes absorbed, and for a range or a stage that does not exist"""
    mw = _weights(P.TOY)
    eng = HipModel(mw, batch=1, l_max=400, prefill_backend="native")
    gen = torch.Generator(device="cuda").manual_seed(1)
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="no GEMM-prefill chunk on record"):
        eng.prefill_rows(0, 0, 1)
    eng.forward(_tokens(P.TOY, 1, 200, gen), zero)
    assert eng.prefill_rows(0, 0, 200).shape == (200, 256) and eng.prefill_rows(3, 199, 1).shape == (1, 512)
    for bad in ((0, -1, 1), (0, 0, 201), (0, 200, 1), (1, 2 ** 31 - 1, 2)):
        with pytest.raises(RuntimeError, match="outside the 200 rows"):
            eng.prefill_rows(*bad)
    out = torch.empty(256, dtype=torch.bfloat16, device="cuda")
    assert eng.lib.sd_model_prefill_rows(eng.handle, 4, 0, 1, out.data_ptr(), None) != 0 and "which=4" in _abi.last_error()
    assert eng.lib.sd_model_prefill_rows(eng.handle, 0, 0, 0, out.data_ptr(), None) != 0 and "outside the 200 rows" in _abi.last_error()
    assert eng.lib.sd_model_prefill_rows(eng.handle, 2, 199, 2 ** 31 - 1, out.data_ptr(), None) != 0 and "outside the 200 rows" in _abi.last_error()
    assert eng.lib.sd_model_prefill_rows(eng.handle, 0, 0, 1, None, None) != 0 and "NULL" in _abi.last_error()
    eng.forward(_tokens(P.TOY, 1, 5, gen), torch.full((1,), 200, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="no GEMM-prefill chunk on record"):
        eng.prefill_rows(0, 0, 1)
    eng.forward(_tokens(P.TOY, 1, 100, gen), zero)
    assert eng.prefill_rows(0, 0, 100).shape == (100, 256)
    eng.set_prefill_backend("passes")
    eng.forward(_tokens(P.TOY, 1, 100, gen), zero)
    with pytest.raises(RuntimeError, match="no GEMM-prefill chunk on record"):
        eng.prefill_rows(0, 0, 1)
    assert eng.engine_status() == 0


@pytest.mark.parametrize("wd", ["bf16", "fp8"])
def test_stale_products_of_a_longer_prompt(wd):
    """a 512-position prompt, then shorter ones on the same engine: the product buffer, the workspace rows and the cache beyond
    the shorter prompt hold the longer one's values — a block the GEMM skipped would keep a plausible stale product, and a key
    past a query's position is a real K / V row of another prompt. Every row of every shorter prompt meets its bounds."""
    mw = _weights(P.TOY)
    eng = HipModel(mw, batch=1, l_max=544, weight_dtype=wd, prefill_backend="native")
    mats = _matrices(mw, wd)
    gen = torch.Generator(device="cuda").manual_seed(99)
    for L in (512, 300, 129, 96):
        _assert_plan(eng, "toy-d64", wd, L)
        tok = _tokens(P.TOY, 1, L, gen)
        _forward(eng, "native", tok, 0, 0)
        _check_prompt(eng, mw, mats, tok[0], 0, L, 0, R.chain_hip, f"stale {wd} L={L} after longer prompts")


_SPIKED = {}


def _spiked():
    if "mw" not in _SPIKED:
        _SPIKED["mw"] = P.spike_weights(_weights(P.TOY))
    return _SPIKED["mw"]


@pytest.mark.parametrize("L,s", P.FUTURE, ids=[f"L{L}-spike{s}" for L, s in P.FUTURE])
def test_future_keys_are_masked(L, s):
    """the QKV epilogue appends the whole chunk's K / V before any attention sub-pass runs, so queries of the first sub-passes
    have keys of their own future in the cache. From position s on every token is the spike token (V rows ~256 x any other): a
    query before s that saw ONE of them would move by ~256 / (its keys) of the V scale, far over the attention bound
    (tests/test_stage_bounds.py shows it at the largest position used). Every query meets its bound against the causal reference."""
    mw = _spiked()
    c = mw.config
    eng = HipModel(mw, batch=1, l_max=L + 32, prefill_backend="native")
    _assert_plan(eng, "toy-d64", "bf16", L)
    gen = torch.Generator(device="cuda").manual_seed(s)
    tok = _tokens(c, 1, L, gen)
    tok[0, s:] = P.SPIKE_TOKEN
    _forward(eng, "native", tok, 0, 0)
    # the construction's precondition, from the cache itself: the spike rows' V is two orders above the others'
    k, v = _cache_rows(eng, 0, torch.arange(L))
    v = v.float().abs().mean((0, 2))
    assert float(v[s:].min()) > 100 * float(v[:s].max()), (float(v[s:].min()), float(v[:s].max()))
    _check_prompt(eng, mw, _matrices(mw, "bf16"), tok[0], 0, L, 0, R.chain_hip, f"future keys L={L} spikes from {s}")


def test_two_layers_every_row():
    """layer 1 of a 2-layer toy at 512 positions, from the exact bf16 rows entering it: those a 1-layer engine over layer 0
    leaves (prefill_rows, residual stream), after the two engines' layer-0 K / V are shown bit-equal — so no input-uncertainty
    term. Holds the per-layer weight index and the KV layer stride for all 512 rows."""
    mw2 = W.random_init(P.TWO_LAYER, seed=7, device="cuda")
    mw1 = dataclasses.replace(mw2, config=dataclasses.replace(P.TWO_LAYER, n_layers=1, name="toy-d64-2l-first"), layers=mw2.layers[:1], meta={})
    L = 512
    tok = _tokens(P.TWO_LAYER, 1, L, torch.Generator(device="cuda").manual_seed(2))
    e1 = HipModel(mw1, batch=2, l_max=L + 32, prefill_backend="native")
    e2 = HipModel(mw2, batch=2, l_max=L + 32, prefill_backend="native")
    _assert_plan(e2, "toy-d64", "bf16", L)
    for e in (e1, e2):
        _forward(e, "native", tok, 0, 1)
    pos = torch.arange(L)
    for a, b in zip(_cache_rows(e1, 1, pos, 0), _cache_rows(e2, 1, pos, 0)):
        assert torch.equal(a, b)
    _check_prompt(e1, mw1, _matrices(mw1, "bf16"), tok[0], 0, L, 1, R.chain_hip, "two layers: layer 0 alone")
    x_in = e1.prefill_rows(HipModel.DEBUG_X, 0, L)
    _check_prompt(e2, mw2, _matrices(mw2, "bf16", layer=1), tok[0], 0, L, 1, R.chain_hip, "two layers: layer 1", layer=1, x_in=x_in)
