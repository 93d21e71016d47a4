"""attention_prefill_kernel (csrc/attention_prefill.hip) against fp64: prompts into HipModel(prefill_attention="tiled").

A case is one prompt of L positions at pos0 into a one-layer model whose cached prefix [0, pos0) holds tests/attention_cases.py's
sentinel layout. After the forward, for every 128-row group of the last chunk, prefill_rows(DEBUG_Q / DEBUG_ATTN) is held element
by element to stage_ref.attention_stage over the cache read back through kv_view (the chunk's own appended positions included)
and its bound, unchanged. The forward is issued twice and must repeat bit for bit.

On the bound. A query row is walked by ONE wave over 64-key blocks in order: one running-max rescaling per block, (keys / 64)
__expf factors, within eps_c's (keys / 32) + 40; nothing is merged, so the "+ 40" is not drawn on. Its P V sum is one fp32
chain of 2 MFMAs per block, keys / 32 accumulations, within chain_pv's (keys / 32) + 64. The plan never splits a tile's keys."""

import pytest
import torch

import attention_cases as A
import stage_ref as R
from specdec_hip.engine import HipModel
from specdec_hip.ops import attention_prefill_plan
from test_hip_attention_cascade_gpu import _get, _put
from test_hip_attention_geometry_gpu import _weights

pytestmark = pytest.mark.gpu

G4 = A.Model("pf-g4-d64", 256, 4, 1, 64, 512, max_pos=8192)
MHA = A.Model("pf-mha-d64", 256, 4, 4, 64, 512)
MHA16 = A.Model("pf-mha16-d64", 1024, 16, 16, 64, 512)      # 16 kv heads: a 512-position chunk takes PT = 32
G8 = A.Model("pf-g8-d64", 512, 8, 1, 64, 512)               # 128 rows: all 8 waves of a 512-thread launch own rows
G6 = A.Model("pf-g6-d128", 768, 6, 1, 128, 1024)            # 96 rows: 6 of 8 waves, two pieces per thread of each staged tile
G3X16 = A.Model("pf-g3x16-d64", 1024, 48, 16, 64, 512)      # PT = 32 at G = 3: 96 rows, a head's 32 positions span two waves

# id: (model, pos0, L, l_max, page, rows of the bound batch, cache row)
CASES = {
    "g4-d64-L200": (G4, 0, 200, 256, None, 1, 0),               # partial last query tile, the first block is diagonal
    "g3-d128-L330": (A.G3, 0, 330, 352, None, 1, 0),            # the register-heaviest instance, 48 rows in 3 of 4 waves
    "g3-d128-p1003": (A.G3, 1003, 140, 1152, None, 1, 0),       # unmasked prefix blocks, a diagonal that starts mid-block
    "g4-d64-L600": (G4, 0, 600, 608, None, 1, 0),               # a full 512-position launch, a second chunk over its keys
    "mha-d64-L130": (MHA, 0, 130, 160, None, 1, 0),             # one row per position
    "g4-d64-p4100": (G4, 4100, 130, 4256, None, 1, 0),          # dozens of blocks per tile
    "g3-d128-p1003-page32": (A.G3, 1003, 140, 1152, 32, 1, 0),  # every block straddles two pages
    "g3-d128-p1003-page64": (A.G3, 1003, 140, 1152, 64, 1, 0),
    "g4-d64-row1": (G4, 70, 200, 288, None, 2, 1),              # slab addressing by cache row
    "mha16-d64-L512-pt32": (MHA16, 0, 512, 512, None, 1, 0),    # PT = 32: two waves per head, every group of a full chunk
    # the 512-thread instances (dense and paged, both head sizes): ids ending in -w8 assert waves > 4 from the plan
    "g8-d64-L200-w8": (G8, 0, 200, 256, None, 1, 0),
    "g8-d64-p1003-page32-w8": (G8, 1003, 140, 1152, 32, 1, 0),
    "g6-d128-L200-w8": (G6, 0, 200, 256, None, 1, 0),
    "g6-d128-p1003-page64-w8": (G6, 1003, 140, 1152, 64, 1, 0),
    "g3x16-d64-L512-pt32-w8": (G3X16, 0, 512, 512, None, 1, 0),
}


def _engine(md, l_max, page, batch):
    # (every model here is one the native GEMM backend admits)
    eng = HipModel(_weights(md), batch=batch, l_max=l_max, page_len=page, prefill_backend="native", prefill_attention="tiled")
    assert eng.l_max == l_max and eng.prefill_attention == "tiled"
    return eng


def _prompt(eng, md, name, pos0, L, row, sentinel_nan=False):
    """the prefix into the cache, the prompt forwarded twice; -> worst |attn - ref| / bound over the last chunk"""
    case = A.Case(name, md, (pos0,), L, eng.l_max, pages=(eng.page_len,), batch=eng.batch, row0=row)
    if pos0:
        kk, vv = (t.to("cuda")[:, :pos0] for t in A.cache_row(case, 0))
        _put(eng, row, 0, kk, vv)
    if sentinel_nan:                    # everything the kernel must not multiply in: beyond the prompt, and the other row
        k, v = eng.kv_view()
        k[0, row, :, pos0 + L:], v[0, row, :, :, pos0 + L:] = float("nan"), float("nan")
        k[0, 1 - row], v[0, 1 - row] = float("nan"), float("nan")
    gen = torch.Generator(device="cuda").manual_seed(len(name) + L)
    tok = torch.randint(4, md.vocab, (1, L), generator=gen, device="cuda", dtype=torch.int32)
    pos = torch.tensor([pos0], dtype=torch.int32, device="cuda")
    m0 = (L - 1) // 512 * 512           # the last chunk
    mc = L - m0
    before = eng.prefill_tiled_launches()
    eng.forward(tok, pos, row0=row, skip_head=True)
    assert eng.prefill_tiled_launches() == before + (L + 511) // 512
    q, attn = eng.prefill_rows(HipModel.DEBUG_Q, 0, mc), eng.prefill_rows(HipModel.DEBUG_ATTN, 0, mc)
    assert bool(torch.isfinite(attn.float()).all()), "attention rows are not finite"
    worst = 0.0
    for g0 in range(0, mc, 128):
        m = min(128, mc - g0)
        first = pos0 + m0 + g0
        kd, vd = (t.expand(m, -1, -1, -1) for t in _get(eng, row, 0, first + m))
        ref = R.attention_stage(q[g0:g0 + m], kd, vd, torch.arange(first, first + m, device="cuda"), md.hkv, md.D)
        worst = max(worst, R.check(attn[g0:g0 + m], ref, f"{name}: positions {first} .. {first + m - 1}"))
    eng.forward(tok, pos, row0=row, skip_head=True)
    assert torch.equal(attn, eng.prefill_rows(HipModel.DEBUG_ATTN, 0, mc)), "a repeated forward differs"
    assert eng.engine_status() == 0
    return worst


@pytest.mark.parametrize("name", list(CASES))
def test_tiled_prompt_attention_against_fp64(name):
    md, pos0, L, l_max, page, batch, row = CASES[name]
    eng = _engine(md, l_max, page, batch)
    plan = attention_prefill_plan(md.hq, md.hkv, md.D, min(L, 512), l_max, page or 0)
    assert plan.n_split == 1 and plan.pt == (32 if "pt32" in name else 16) and (plan.waves > 4) == name.endswith("-w8"), plan
    worst = _prompt(eng, md, name, pos0, L, row)
    print(f"[prefill/attention] {name}: {plan} worst / bound {worst:.3f}")


def test_keys_beyond_the_prompt_are_never_multiplied_in():
    """NaN at every position of the row beyond pos0 + L and in the neighbouring row of a dense cache: masked and clamped loads
    stay out of the sums. The cache is bound again at l_max = 1160 (a multiple of 8 only; HipModel itself rounds to 32) and the
    prompt ends at key 1157, so the last block's first half, keys 1152 .. 1183, takes the row and V^T clamps at the slab's end
    and its second half lies beyond the tile."""
    eng = _engine(G4, 1184, None, 2)
    eng.l_max = 1160
    eng._bind_dense()
    eng.set_prefill_backend("native")       # (a bind resets the backend; the attention mode is kept)
    assert eng.prefill_attention == "tiled"
    worst = _prompt(eng, G4, "nan-sentinel", 1003, 155, 0, sentinel_nan=True)
    print(f"[prefill/attention] nan-sentinel: worst / bound {worst:.3f}")
