"""attention_cascade_kernel (csrc/attention_cascade.hip) against fp64: groups of rows on a HipModel(cascade=True).

A case is one forward over rows (cached keys, leader, shared_len). Every row's content is tests/attention_cases.py's sentinel
layout; a member's LOGICAL cache is its leader's positions [0, shared_len) followed by its own. The prefix exists in the leader's
row only: on a dense cache the members' own [0, shared_len) hold NaN (a kernel that reads them fails loudly), on a paged cache
the members' tables name the leader's pages (fork_row). After one forward, debug_rows(DEBUG_Q / DEBUG_ATTN) is held element by
element to stage_ref.attention_stage over each row's logical cache (read back, new positions included) and its derived bound; the
forward is issued twice and must repeat bit for bit (workspace and arrival counters left as found).

On the bound. attention_stage's terms hold as they stand. A term of the softmax passes the same three levels of running-max
rescaling as in the split kernel — its wave's blocks, the 4-wave merge, ONE merge over the tile's partials: prefix and suffix
partials meet in that last merge together, there is no level between them — so eps_c's count ((keys / 32) + 40 factors) covers it.
What grows is the number of partials that last merge adds, s_suffix + s_prefix <= 2 * ceil(blocks / 16) instead of <= 32; with the
<= blocks / 4 additions of a wave and the 4 of the wave merge that stays below chain_pv's (keys / 32) + 64 fp32 additions."""

import pytest
import torch

import attention_cases as A
import stage_ref as R
from specdec_hip.engine import HipModel
from specdec_hip.ops import attention_cascade_plan, attention_plan
from test_hip_attention_geometry_gpu import _tokens, _weights

pytestmark = pytest.mark.gpu

G4 = A.Model("cascade-g4-d128", 512, 4, 1, 128, 1024)   # a D = 128 model whose passes hold more than 9 tokens

# id: (model, M, l_max, page, row0, rows); a row: (cached keys, index of its leader among the rows or None, shared_len)
CASES = {
    # 4 x 10 = 40 stacked query rows: 3 tiles, a partial last one, tiles that straddle members; suffixes of 5 .. 81 keys
    "edge-4x1024": (A.EDGE, 5, 1536, None, 0, [(1030, 0, 1024), (1056, 0, 1024), (1100, 0, 1024), (1024, 0, 1024)]),
    # D = 128, 2 tiles per row. This model's passes hold 9 tokens, so each row is a launch of its own: a group of one in the pass,
    # whose leader (rows 1, 2) lies outside the pass
    "g3-d128": (A.G3, 6, 1536, None, 0, [(1030, 0, 1024), (1040, 0, 1024), (1100, 0, 1024)]),
    # 3 x 20 = 60 stacked rows in ONE launch: all NT = 4 tiles of a set at D = 128 (the register limit), tiles that straddle members
    "g4-d128-nt4": (G4, 5, 1536, None, 0, [(1030, 0, 1024), (1040, 0, 1024), (1100, 0, 1024)]),
    # unequal lengths in one group, an ungrouped row, a second group; the pass starts at row 1 of the bound batch
    "unequal-two-groups": (A.EDGE, 5, 1536, None, 1, [(1060, 0, 1024), (600, 0, 512), (50, 0, 32), (700, None, 0), (300, 4, 256), (290, 4, 256)]),
    # 4 prefix workgroups per set (2048 shared keys), 7 stacked tiles: two sets, a row whose tile is met by both
    "split-prefix": (A.EDGE, 5, 2560, None, 0, [(2100, 0, 2048), (2048, 0, 2048), (2300, 0, 2048)] + [(2060 + i, 0, 2048) for i in range(8)]),
    "edge-4x1024-page64": (A.EDGE, 5, 1536, 64, 0, [(1030, 0, 1024), (1056, 0, 1024), (1100, 0, 1024), (1024, 0, 1024)]),
    "draft-m1": (A.EDGE, 1, 1536, None, 0, [(1030, 0, 1024), (1056, 0, 1024), (1024, 0, 1024)]),
}


def _put(eng, row, lo, kk, vv):
    """positions [lo, n) of [Hkv][n][D] tensors into cache row `row` (paged: through its table)"""
    k, v = eng.kv_view()
    n = kk.shape[1]
    if eng.page_len is None:
        k[0, row, :, lo:n] = kk[:, lo:]
        v[0, row, :, :, lo:n] = vv[:, lo:].transpose(1, 2)
    else:
        eng.reserve(row, n)
        pos = torch.arange(lo, n, device="cuda")
        pages = eng.block_table[row].long()[pos // eng.page_len]
        k[0][pages, :, pos % eng.page_len] = kk[:, lo:].transpose(0, 1)
        v[0][pages, :, :, pos % eng.page_len] = vv[:, lo:].permute(1, 0, 2)


def _get(eng, row, lo, hi):
    """K, V [Hkv][hi - lo][D] of positions [lo, hi) as cache row `row` holds them"""
    k, v = eng.kv_view()
    if eng.page_len is None:
        return k[0, row, :, lo:hi], v[0, row, :, :, lo:hi].transpose(1, 2)
    pos = torch.arange(lo, hi, device="cuda")
    pages = eng.block_table[row].long()[pos // eng.page_len]
    return k[0][pages, :, pos % eng.page_len].transpose(0, 1), v[0][pages, :, :, pos % eng.page_len].permute(1, 0, 2)


def _case(name):
    md, M, l_max, page, row0, rows = CASES[name]
    return A.Case(name, md, tuple(r[0] for r in rows), M, l_max, pages=(page,), batch=row0 + len(rows), row0=row0), rows, page


def _check(eng, case, rows, q, attn, leader0=None):
    """every row's attention against fp64 over its logical cache: the leader's [0, shared_len), then its own (leader indices
    count from cache row leader0, default the launch's first row)"""
    md, M = case.model, case.M
    worst = 0.0
    for i, (n, ldr, sl) in enumerate(rows):
        S, row = n + M, case.row0 + i
        parts = [_get(eng, (case.row0 if leader0 is None else leader0) + ldr, 0, sl), _get(eng, row, sl, S)] if sl else [_get(eng, row, 0, S)]
        kd = torch.cat([p[0] for p in parts], 1).expand(M, -1, -1, -1)
        vd = torch.cat([p[1] for p in parts], 1).expand(M, -1, -1, -1)
        ref = R.attention_stage(q[i * M:(i + 1) * M], kd, vd, torch.arange(n, n + M, device="cuda"), md.hkv, md.D)
        worst = max(worst, R.check(attn[i * M:(i + 1) * M], ref, f"{case.id} row {i} ({n} cached keys, {sl} shared)"))
    return worst


def _set_groups(eng, case, rows):
    for i, (_, ldr, sl) in enumerate(rows):      # roots first: the longest length of their members
        if ldr == i:
            eng.set_shared_prefix(case.row0 + i, case.row0 + i, max(r[2] for r in rows if r[1] == i))
    for i, (_, ldr, sl) in enumerate(rows):
        if ldr is not None and ldr != i:
            eng.set_shared_prefix(case.row0 + i, case.row0 + ldr, sl)


def _forward_twice(eng, case, tok):
    T = case.B * case.M
    pos = torch.tensor(case.lens, dtype=torch.int32, device="cuda")
    _, logits = eng.forward(tok, pos, want_logits=True, row0=case.row0)
    q, attn = eng.debug_rows(HipModel.DEBUG_Q, T), eng.debug_rows(HipModel.DEBUG_ATTN, T).clone()
    _, logits2 = eng.forward(tok, pos, want_logits=True, row0=case.row0)
    assert torch.equal(attn, eng.debug_rows(HipModel.DEBUG_ATTN, T)) and torch.equal(logits, logits2), "a repeated forward differs"
    return q, attn


@pytest.mark.parametrize("name", list(CASES))
def test_cascade_attention_against_fp64(name):
    case, rows, page = _case(name)
    md = case.model
    eng = HipModel(_weights(md), batch=case.bound_batch, l_max=case.l_max, page_len=page, cascade=True)
    assert eng.l_max == case.l_max and not eng.persist_active(1) and (case.B * case.M <= eng.pass_tokens) == (name != "g3-d128")
    plan = attention_cascade_plan(md.hq, md.hkv, md.D, case.B, case.M, eng.l_max, page or 0)
    assert (plan.tiles, plan.n_split) == attention_plan(md.hq, md.hkv, md.D, case.B, case.M, eng.l_max, page or 0)[:2]
    if name == "split-prefix":
        assert plan.p_split >= 4 and plan.sets == 2, plan
    if name == "g4-d128-nt4":
        assert plan.sets == 1 and -(-case.B * md.G * case.M // 16) == 4, plan
    content = [tuple(t.to("cuda") for t in A.cache_row(case, i)) for i in range(case.B)]
    for i, (n, ldr, sl) in enumerate(rows):       # leaders and ungrouped rows: their whole content
        if ldr is None or ldr == i:
            _put(eng, case.row0 + i, 0, *content[i])
    for i, (n, ldr, sl) in enumerate(rows):       # members: the prefix is the leader's alone
        if ldr is None or ldr == i:
            continue
        if page is None:
            nan = torch.full((md.hkv, sl, md.D), float("nan"), dtype=torch.bfloat16, device="cuda")
            _put(eng, case.row0 + i, 0, nan, nan)
        else:                                     # pages wholly below (sl + 6) - 2 are shared: exactly [0, sl)
            eng.fork_row(case.row0 + ldr, [case.row0 + i], sl + 6)
            assert eng.block_table[case.row0 + i, :sl // page].tolist() == eng.block_table[case.row0 + ldr, :sl // page].tolist()
        _put(eng, case.row0 + i, sl, *content[i])
    _set_groups(eng, case, rows)
    tok = _tokens(case, len(name) + case.M)
    if case.B * case.M <= eng.pass_tokens:
        worst = _check(eng, case, rows, *_forward_twice(eng, case, tok))
    else:                                         # one launch per row
        worst = 0.0
        for i in range(case.B):
            one = A.Case(name, md, case.lens[i:i + 1], case.M, case.l_max, batch=case.bound_batch, row0=case.row0 + i)
            worst = max(worst, _check(eng, one, rows[i:i + 1], *_forward_twice(eng, one, tok[i:i + 1]), leader0=case.row0))
    assert eng.engine_status() == 0
    print(f"[cascade/attention] {name}: tiles {plan.tiles} n_split {plan.n_split} sets {plan.sets} p_split {plan.p_split} worst / bound {worst:.3f}")


@pytest.mark.parametrize("md", [A.EDGE, G4], ids=["d64", "d128"])
def test_moving_a_root_and_clearing_the_table(md):
    """The root moves from row 0 to row 1 (whose copy of the prefix is real, as a fork leaves it); row 0's cache and row 2's copy
    of the prefix become NaN and the next forward of rows 1, 2 stays in bound. Then every entry is cleared (row 2's prefix
    restored): ungrouped rows are the plain computation — the plain kernel's block order, wave merge and split merge (3
    workgroups per tile here on both engines) — and are held to the fp64 bound. At D = 64 they also equal a cascade=False engine's
    attention rows BIT FOR BIT. At D = 128 they do not (the two kernels are separate instantiations and the compiler contracts
    their fp32 multiply-adds differently), so there the fp64 bound alone holds; the number of differing elements is printed."""
    M, l_max, sl = 5, 1536, 1024
    rows = [(1030, 0, sl), (1056, 0, sl), (1100, 0, sl)]
    case = A.Case("move-root", md, tuple(r[0] for r in rows), M, l_max, batch=3)
    eng = HipModel(_weights(md), batch=3, l_max=l_max, cascade=True)
    content = [tuple(t.to("cuda") for t in A.cache_row(case, i)) for i in range(3)]
    for i in range(3):
        kk, vv = (torch.cat([content[0][j][:, :sl], content[i][j][:, sl:]], 1) for j in (0, 1))
        _put(eng, i, 0, kk, vv)
    _set_groups(eng, case, rows)
    tok = _tokens(case, 11)
    q, attn = _forward_twice(eng, case, tok)
    worst = _check(eng, case, rows, q, attn)
    # ---- the root moves to row 1
    eng.set_shared_prefix(1, 1, sl)
    eng.set_shared_prefix(2, 1, sl)
    eng.set_shared_prefix(0, 0, 0)
    k, v = eng.kv_view()
    k[0, 0], v[0, 0] = float("nan"), float("nan")
    k[0, 2, :, :sl], v[0, 2, :, :, :sl] = float("nan"), float("nan")
    sub = A.Case("move-root", md, case.lens[1:], M, l_max, batch=3, row0=1)
    moved = [(1056, 0, sl), (1100, 0, sl)]
    q, attn = _forward_twice(eng, sub, tok[1:])
    worst = max(worst, _check(eng, sub, moved, q, attn))
    # ---- no entries: the plain computation
    eng.set_shared_prefix(2, 2, 0)
    eng.set_shared_prefix(1, 1, 0)
    k[0, 2, :, :sl], v[0, 2, :, :, :sl] = k[0, 1, :, :sl], v[0, 1, :, :, :sl]
    q, attn = _forward_twice(eng, sub, tok[1:])
    worst = max(worst, _check(eng, sub, [(1056, None, 0), (1100, None, 0)], q, attn))
    plain = HipModel(_weights(md), batch=3, l_max=l_max)
    plain.set_persist_tokens(0)
    assert attention_plan(md.hq, md.hkv, md.D, 2, M, l_max).n_split == 3
    pk, pv = plain.kv_view()
    pk[0, 1:], pv[0, 1:] = k[0, 1:], v[0, 1:]
    _, attn_plain = _forward_twice(plain, sub, tok[1:])
    if md.D == 64:
        assert torch.equal(attn, attn_plain), "ungrouped rows differ from the plain kernel's bits"
    print(f"[cascade/attention] move-root {md.name}: {int((attn != attn_plain).sum())} of {attn.numel()} elements differ from the plain kernel")
    assert eng.engine_status() == 0 and plain.engine_status() == 0
    print(f"[cascade/attention] move-root {md.name}: worst / bound {worst:.3f}")
