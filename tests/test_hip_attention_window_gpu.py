"""Sliding-window attention (csrc/attention_window.hip, the WIN instances of csrc/attention_prefill.hip) against fp64, through
HipModel(sliding_window=W) on one-layer models. Reference: stage_ref.attention_stage and its own bound, unchanged, over each query's
own W cache slots lo .. lo + W - 1, lo = max(0, p - W + 1), with the query placed at p - lo (softmax attention over rotated q and k
does not depend on absolute position; slots past p are masked by the reference itself).
Skipping: below ((first window start) & ~63) the cache holds NaN, from there up to the window start +-1e30: a kernel that loads and
masks a block below the window fails on 0 x NaN, one that takes a key below a row's window as visible fails on 1e30.
The split case (l_max 8192, W 1100, rows of 1003 and 7000 cached keys) gives both rows s_eff 2 under n_split 2 by the kernel's own
rule; a third row of 300 keys (s_eff 1) is in the launch so that rows with different s_eff share it."""

import pytest
import torch

import attention_cases as A
import stage_ref as R
from specdec_hip import _abi
from specdec_hip.engine import HipModel
from specdec_hip.ops import attention_window_plan
from test_hip_attention_cascade_gpu import _get, _put
from test_hip_attention_geometry_gpu import _tokens, _weights

pytestmark = pytest.mark.gpu

D64 = A.Model("win-g4-d64", 256, 4, 1, 64, 512, max_pos=8192)      # passes of these two hold the launches below whole
D128 = A.Model("win-g4-d128", 512, 4, 1, 128, 1024, max_pos=8192)


def _window_ref(eng, md, q, row, pos, W):
    """(ref, bound) of the queries q [T] at positions pos [T] of cache row `row`, each over its own window"""
    T, hi = pos.numel(), int(pos.max()) + 1
    lo = (pos - W + 1).clamp(min=0)
    kall, vall = _get(eng, row, 0, hi)                                              # [Hkv][hi][D]
    idx = (lo.view(T, 1) + torch.arange(min(W, hi), device="cuda").view(1, -1)).clamp(max=hi - 1)
    return R.attention_stage(q, kall[:, idx].transpose(0, 1), vall[:, idx].transpose(0, 1), pos - lo, md.hkv, md.D)


def _poison(kk, vv, start):
    """NaN below start & ~63, +-1e30 from there to the window start"""
    cut = start & ~63
    for t in (kk, vv):
        t[:, :cut] = float("nan")
        t[:, cut:start] = 1e30
        t[:, cut:start:2] = -1e30


def _decode(md, W, M, lens, l_max, page=None, poison=False):
    """one launch of len(lens) rows x M tokens, twice -> (worst |attn - ref| / bound, the engine)"""
    case = A.Case(f"window-{md.name}-W{W}-M{M}", md, tuple(lens), M, l_max, pages=(page,))
    eng = HipModel(_weights(md), batch=case.B, l_max=l_max, page_len=page, sliding_window=W)
    assert eng.sliding_window == W and eng.l_max == l_max and not eng.persist_active(1) and case.B * M <= eng.pass_tokens
    for i, n in enumerate(lens):
        kk, vv = (t.to("cuda") for t in A.cache_row(case, i))
        if poison and n - W + 1 >= 64:
            _poison(kk, vv, n - W + 1)
        _put(eng, i, 0, kk, vv)
    tok, pos = _tokens(case, W + M), torch.tensor(lens, dtype=torch.int32, device="cuda")
    T = case.B * M
    eng.forward(tok, pos, skip_head=True)
    q, attn = eng.debug_rows(HipModel.DEBUG_Q, T), eng.debug_rows(HipModel.DEBUG_ATTN, T).clone()
    eng.forward(tok, pos, skip_head=True)
    assert torch.equal(attn, eng.debug_rows(HipModel.DEBUG_ATTN, T)), "a repeated forward differs"
    assert bool(torch.isfinite(attn.float()).all()), "attention rows are not finite"
    worst = 0.0
    for i, n in enumerate(lens):
        ref = _window_ref(eng, md, q[i * M:(i + 1) * M], i, torch.arange(n, n + M, device="cuda"), W)
        worst = max(worst, R.check(attn[i * M:(i + 1) * M], ref, f"{case.id} row {i} ({n} cached keys)"))
    assert eng.engine_status() == 0
    return worst, eng


# W = 40 is no multiple of the block; rows: a window not yet full, exactly full, the first key dropped, two dropped, and a window
# that starts mid-block far from 0. M = 17 at G = 4: five query tiles with different first blocks, tiles that cross a head boundary.
LAUNCHES = [(D64 if W == 64 else D128, W, M, None) for W in (40, 64, 100) for M in (1, 5, 17)]
LAUNCHES += [(D64, 100, 5, 32), (D64, 100, 5, 64), (D128, 40, 17, 32)]


@pytest.mark.parametrize("md,W,M,page", LAUNCHES, ids=[f"{md.name.split('-')[-1]}-W{W}-M{M}-{'dense' if p is None else f'page{p}'}" for md, W, M, p in LAUNCHES])
def test_window_launch_against_fp64(md, W, M, page):
    worst, _ = _decode(md, W, M, (W - 2, W - 1, W, W + 1, 1003), 1152, page)
    print(f"[window/attention] {md.name} W {W} M {M} page {page}: worst / bound {worst:.3f}")


@pytest.mark.parametrize("split", [True, False], ids=["split", "nosplit"])
def test_split_follows_the_span(split, monkeypatch):
    if not split:
        monkeypatch.setenv("SPECDEC_NO_ATTN_SPLIT", "1")
    W, M, lens, l_max = 1100, 5, (1003, 7000, 300), 8192
    plan = attention_window_plan(D128.hq, D128.hkv, D128.D, len(lens), M, l_max, W)
    s_eff = []
    for n in lens:                      # the kernel's rule for the first tile of each row
        b_lo, n_blocks = max(0, n - W + 1) // 32, -(-(n + M) // 32)
        s_eff.append(min(plan.n_split, max(1, -(-(n_blocks - b_lo) // 16))))
    assert (plan.n_split >= 2 and len(set(s_eff)) > 1) if split else plan.n_split == 1, (plan, s_eff)
    worst, _ = _decode(D128, W, M, lens, l_max)
    print(f"[window/attention] split {split}: {plan} s_eff {s_eff} worst / bound {worst:.3f}")


def test_window_longer_than_the_row_is_full_causal_attention():
    print("[window/attention] W 4096 over 300 keys: worst / bound %.3f" % _decode(D128, 4096, 5, (300,), 4224)[0])   # (the gather is the whole row)


@pytest.mark.parametrize("md", [D64, D128], ids=["d64", "d128"])
def test_blocks_below_the_window_are_never_read(md):
    worst, eng = _decode(md, 100, 5, (1003,), 1152, poison=True)
    assert eng.lib.sd_model_set_sliding_window(eng.handle, 64) != 0 and "sliding_window" in _abi.last_error() and "bound" in _abi.last_error()
    with pytest.raises(RuntimeError, match="sliding_window"):
        eng.evict_row(0, 4, 8, 64)
    print(f"[window/attention] NaN below the window, {md.name}: worst / bound {worst:.3f}")


PROMPTS = [(0, 330, 100, "tiled", None), (0, 330, 100, "passes", None), (1003, 140, 100, "tiled", None), (1003, 140, 100, "passes", None),
           (1003, 140, 40, "tiled", None), (1003, 140, 40, "passes", None), (1003, 140, 100, "tiled", 32)]


@pytest.mark.parametrize("pos0,L,W,mode,page", PROMPTS, ids=[f"p{p}-L{L}-W{W}-{m}-{'dense' if pg is None else f'page{pg}'}" for p, L, W, m, pg in PROMPTS])
def test_windowed_prompt_against_fp64(pos0, L, W, mode, page):
    md, l_max = A.G3, 352 if pos0 == 0 else 1152
    eng = HipModel(_weights(md), batch=1, l_max=l_max, page_len=page, prefill_backend="native", prefill_attention=mode, sliding_window=W)
    if pos0:                            # the cached prefix, poisoned below the first query's window
        kk, vv = (t.to("cuda")[:, :pos0] for t in A.cache_row(A.Case("window-prompt", md, (pos0,), L, l_max, pages=(page,)), 0))
        _poison(kk, vv, pos0 - W + 1)
        _put(eng, 0, 0, kk, vv)
    gen = torch.Generator(device="cuda").manual_seed(L + W)
    tok = torch.randint(4, md.vocab, (1, L), generator=gen, device="cuda", dtype=torch.int32)
    pos = torch.tensor([pos0], dtype=torch.int32, device="cuda")
    before = eng.prefill_tiled_launches()
    eng.forward(tok, pos, skip_head=True)
    assert eng.prefill_tiled_launches() == before + (1 if mode == "tiled" else 0)
    q, attn = eng.prefill_rows(HipModel.DEBUG_Q, 0, L), eng.prefill_rows(HipModel.DEBUG_ATTN, 0, L)
    assert bool(torch.isfinite(attn.float()).all()), "attention rows are not finite"
    worst = 0.0
    for g0 in range(0, L, 128):
        m = min(128, L - g0)
        ref = _window_ref(eng, md, q[g0:g0 + m], 0, torch.arange(pos0 + g0, pos0 + g0 + m, device="cuda"), W)
        worst = max(worst, R.check(attn[g0:g0 + m], ref, f"prompt at {pos0}, W {W}, {mode}: positions {pos0 + g0} .."))
    eng.forward(tok, pos, skip_head=True)
    assert torch.equal(attn, eng.prefill_rows(HipModel.DEBUG_ATTN, 0, L)), "a repeated forward differs"
    assert eng.engine_status() == 0
    print(f"[window/prompt] pos0 {pos0} L {L} W {W} {mode} page {page}: worst / bound {worst:.3f}")
