"""attention_mfma_kernel across its launch geometry against fp64, by plan (tests/attention_cases.py).

Every case is one forward of a one-layer `random_init` model over a cache whose prefix was WRITTEN (kv_view, dense or through
the block table with pages handed out in scrambled order), with the sentinel layout of the case: a lost, doubled or
misplaced partial, a wrong tile row, another row's cache, a key beyond n_keys or a wrong page moves some output element by
at least 4 x its bound (proved on the reference alone: tests/test_attention_cases_cpu.py). All stages of the pass are held to
the derived bounds of tests/stage_ref.py by stage_check.check_pass — every element, none excused, nothing fitted. Each case
first asserts from sd_attention_plan that the launch has the geometry it is listed for, runs with and without the split
(SPECDEC_NO_ATTN_SPLIT), and issues its forward twice: the second must repeat the first bit for bit (the merge workspace and
its arrival counters are left as found).

The worst error of every stage as a fraction of its bound and the wall time are printed (run with -s;
profiles/attention_geometry_fp64.md)."""

import random
import time

import pytest
import torch

import attention_cases as A
import stage_ref as R
from specdec_hip import weights as W
from specdec_hip.engine import HipModel
from specdec_hip.ops import attention_plan
from stage_check import check_pass, matrices
from test_hip_prefill_rows_fp64_gpu import _backend, _chain, _check_prompt, _forward

pytestmark = pytest.mark.gpu

_MODEL = {}


def _weights(md):
    """one model of the table at a time"""
    if md.name not in _MODEL:
        _MODEL.clear()
        torch.cuda.empty_cache()
        cfg = W.ModelConfig(arch=md.arch, n_layers=1, d_model=md.d_model, n_heads=md.hq, n_kv_heads=md.hkv, head_dim=md.D, d_ff=md.d_ff,
                            vocab=md.vocab, max_pos=md.max_pos, rope_theta=500000.0, tie_embeddings=False, name=md.name)
        _MODEL[md.name] = W.random_init(cfg, seed=7, device="cuda")
    return _MODEL[md.name]


def _engine(case, page, backend="auto"):
    mw = _weights(case.model)
    eng = HipModel(mw, batch=case.bound_batch, l_max=case.l_max, page_len=page, prefill_backend=backend)
    assert eng.l_max == case.l_max
    eng.set_persist_tokens(0)
    if page is not None:            # pages handed out in a scrambled order
        random.Random(case.l_max + page).shuffle(eng._free)
    return eng, mw


def _write_rows(eng, case):
    """the case's cache contents into rows [row0, row0 + B), straight through kv_view"""
    k, v = eng.kv_view()
    for i in range(case.B):
        kk, vv = (t.to(eng.device) for t in A.cache_row(case, i))          # [Hkv][n][D]
        n, row = kk.shape[1], case.row0 + i
        if eng.page_len is None:
            k[0, row, :, :n] = kk
            v[0, row, :, :, :n] = vv.transpose(1, 2)
        else:
            eng.reserve(row, n)
            P = eng.page_len
            pos = torch.arange(n, device=eng.device)
            pages = eng.block_table[row].long()[pos // P]
            k[0][pages, :, pos % P] = kk.transpose(0, 1)
            v[0][pages, :, :, pos % P] = vv.permute(1, 0, 2)
            if n > 4 * P:
                head = eng.block_table[row, :n // P].tolist()
                assert head != sorted(head), "the pages of a row are not scrambled"


def _assert_plan(eng, case, split):
    md = case.model
    assert case.B * case.M <= eng.pass_tokens, "the case must be one pass: one attention launch of B rows"
    got = attention_plan(md.hq, md.hkv, md.D, case.B, case.M, eng.l_max, eng.page_len or 0)
    assert (got.tiles, got.n_split) == (case.tiles, case.n_split if split else 1), got
    want = A.case_plan(case, split)
    assert (got.tiles, got.n_split) == (want["tiles"], want["n_split"])
    if split:
        assert want["cap"] == case.cap and tuple(sorted({r[2] for r in want["rows"]})) == case.s_eff, want
    return want


def _pass(eng, mw, mats, case, tok, what, check=True):
    """one forward of the case's rows, issued twice: bit-identical logits, ids and attention rows; -> (logits, stage / bound)"""
    T = case.B * case.M
    pos = torch.tensor(case.lens, dtype=torch.int32, device="cuda")
    ids, logits = eng.forward(tok, pos, want_logits=True, row0=case.row0)
    attn = eng.debug_rows(HipModel.DEBUG_ATTN, T).clone()
    ids2, logits2 = eng.forward(tok, pos, want_logits=True, row0=case.row0)
    assert torch.equal(attn, eng.debug_rows(HipModel.DEBUG_ATTN, T)), f"{what}: the attention rows of a repeated forward differ"
    assert torch.equal(logits, logits2) and torch.equal(ids, ids2), f"{what}: a repeated forward differs"
    res = None
    if check:
        positions = torch.tensor([p + m for p in case.lens for m in range(case.M)], device="cuda")
        rows = torch.tensor([case.row0 + i for i in range(case.B) for _ in range(case.M)])
        res = check_pass(eng, mw, mats, tok.reshape(-1).long(), positions, rows, logits.reshape(T, -1), R.chain_hip, what)
    assert eng.engine_status() == 0
    return logits, res


def _tokens(case, seed):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(4, case.model.vocab, (case.B, case.M), generator=gen, device="cuda", dtype=torch.int32)


RUNS = [(c, page, split) for c in A.CASES for page in c.pages for split in (True, False)]


@pytest.mark.parametrize("case,page,split", RUNS,
                         ids=[f"{c.id}-{'dense' if p is None else f'page{p}'}-{'split' if s else 'nosplit'}" for c, p, s in RUNS])
def test_attention_geometry(case, page, split, monkeypatch):
    t0 = time.perf_counter()
    if not split:
        monkeypatch.setenv("SPECDEC_NO_ATTN_SPLIT", "1")
    eng, mw = _engine(case, page)
    want = _assert_plan(eng, case, split)
    _write_rows(eng, case)
    what = f"{case.id} {'dense' if page is None else f'page {page}'} {'split' if split else 'no split'}"
    _pass(eng, mw, matrices(mw, "bf16"), case, _tokens(case, len(case.id) + case.M), what)
    torch.cuda.synchronize()
    print(f"[geometry/plan] {what}: tiles {want['tiles']} base {want['base']} n_split {want['n_split']} cap {'/'.join(want['cap']) or '-'} "
          f"s_eff {[r[2] for r in want['rows']]}")
    print(f"[geometry/time] {what}: {time.perf_counter() - t0:.2f} s")


def test_workspace_handover_between_geometries():
    """one engine, no rebind: a 9-way split of one tile per (row, kv head), a launch that does not split, three tiles of which
    3 of 9 slots are used, then the first again — each against fp64, the last bit-identical to its first run. A stale partial
    or an arrival counter left non-zero shows here."""
    t0 = time.perf_counter()
    first = A.HANDOVER[0]
    eng, mw = _engine(first, None)
    mats = matrices(mw, "bf16")
    for case in A.HANDOVER:
        assert case.model is first.model and case.bound_batch == first.bound_batch and case.l_max == first.l_max
        _assert_plan(eng, case, True)
        _write_rows(eng, case)
    toks = [_tokens(case, 31 + i) for i, case in enumerate(A.HANDOVER)]
    logits = [_pass(eng, mw, mats, case, tok, f"handover {case.id}")[0] for case, tok in zip(A.HANDOVER, toks)]
    again, _ = _pass(eng, mw, mats, first, toks[0], f"handover {first.id} again")
    assert torch.equal(again, logits[0]), "the first pass does not repeat after launches of other geometries"
    torch.cuda.synchronize()
    print(f"[geometry/time] handover: {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("backend", ["native", "rocblas"])
def test_prompt_after_a_long_prefix(backend):
    """300 prompt positions at pos0 1500 on both prefill backends: the attention sub-passes of the prompt run split 4 ways over a
    written prefix with the sentinel layout; every row of the chunk (the last 128 among them) against fp64"""
    t0 = time.perf_counter()
    _backend(backend)
    case = A.PROMPT
    eng, mw = _engine(case, None, backend)
    _write_rows(eng, case)
    gen = torch.Generator(device="cuda").manual_seed(1500)
    tok = torch.randint(4, case.model.vocab, (1, case.M), generator=gen, device="cuda", dtype=torch.int32)
    _forward(eng, backend, tok, case.lens[0], 0)
    _check_prompt(eng, mw, matrices(mw, "bf16"), tok[0], case.lens[0], case.M, 0, _chain(backend), f"{backend} 300 positions at 1500")
    torch.cuda.synchronize()
    print(f"[geometry/time] prompt after prefix, {backend}: {time.perf_counter() - t0:.2f} s")
