"""The stage checks of one forward pass against tests/stage_ref.py, shared by the files that audit a pass (test infrastructure:
no conftest; tests/test_hip_stage_fp64_gpu.py one pass at a time, tests/step_audit.py the passes of a speculative step).

`eng` is a HipModel, or anything with its small reading surface: cfg, device, page_len (None: dense), kv_view(),
block_table (paged), hidden_rows(n) and debug_rows(which, n)."""

import torch

import stage_ref as R
from specdec_hip.engine import HipModel
from specdec_hip.ops import quantize_fp8_rows_hip


def matrices(mw, weight_dtype, layer=0):
    """the matrices the engine multiplies by (those of `layer`, and the lm_head), as fp64 on the device (fp8: the device's own
    quantiser, dequantised)"""
    lw = mw.layers[layer]
    out = {}
    for k, m in (("wqkv", lw.wqkv), ("wo", lw.wo), ("w_up", lw.w_up), ("w_down", lw.w_down), ("head", mw.lm_head)):
        if weight_dtype == "fp8":
            q, s = quantize_fp8_rows_hip(m)
            out[k] = q.to(torch.float64) * s.to(torch.float64)[:, None]
        else:
            out[k] = m
    return out


def cache_rows(eng, row, positions, layer=0):
    """K / V of `positions` of cache row `row` (of `layer`): ([Hkv][n][D], [Hkv][n][D]), dense or paged"""
    k, v = eng.kv_view()
    positions = positions.to(eng.device)
    if eng.page_len is None:
        return k[layer, row][:, positions], v[layer, row][:, :, positions].transpose(1, 2)
    P = eng.page_len
    pages = eng.block_table[row].long()[positions // P]
    off = positions % P
    kk = k[layer][pages, :, off].transpose(0, 1)                   # [Hkv][n][D]
    vv = v[layer][pages, :, :, off].permute(1, 0, 2)                # [Hkv][n][D]
    return kk, vv


def check_pass(eng, mw, mats, tokens, positions, rows, logits, chain, what, layer=0, x_in=None, taps=None):
    """all stage checks of the last pass over query rows with tokens / absolute positions / cache rows [T] (the rows the
    taps hold, in tap order). -> {stage: worst error / bound}. The taps are the last layer's: `layer` > 0 checks the last
    layer of a deeper model from x_in, the exact bf16 rows entering it (the caller's: no input uncertainty), with `mats`
    that layer's matrices. taps(which, T): where the T rows of stage `which` (HipModel.DEBUG_*) come from instead of
    debug_rows / hidden_rows (tests/test_hip_prefill_rows_fp64_gpu.py: any 128 rows of a prompt's last chunk)."""
    c, lw = mw.config, mw.layers[layer]
    Hq, Hkv, D = c.n_heads, c.n_kv_heads, c.head_dim
    T = tokens.shape[0]
    if taps is None:
        taps = lambda which, n: eng.hidden_rows(n) if which == HipModel.DEBUG_X else eng.debug_rows(which, n)
    q = taps(HipModel.DEBUG_Q, T)
    attn = taps(HipModel.DEBUG_ATTN, T)
    act = taps(HipModel.DEBUG_ACT, T)
    x2 = taps(HipModel.DEBUG_X, T)
    res = {}
    x0, x0d = R.embed(c, mw, tokens, positions) if x_in is None else (x_in.to(torch.float64), None)
    ref, bnd = R.qkv_stage(c, lw, mats["wqkv"], x0, x0d, positions, mw.rope_cos, mw.rope_sin, chain)
    res["q"] = R.check(q, (ref[:, :Hq * D], bnd[:, :Hq * D]), f"{what}: q")
    kn = torch.empty(T, Hkv * D, dtype=torch.bfloat16, device=eng.device)
    vn = torch.empty_like(kn)
    S = int(positions.max()) + 1
    kk = torch.empty(T, Hkv, S, D, dtype=torch.bfloat16, device=eng.device)
    vv = torch.empty_like(kk)
    allpos = torch.arange(S)
    for r in sorted(set(rows.tolist())):
        sel = (rows == r).nonzero().flatten().to(eng.device)
        k_r, v_r = cache_rows(eng, r, allpos, layer)
        kk[sel], vv[sel] = k_r, v_r
        kn[sel] = k_r[:, positions[sel]].transpose(0, 1).reshape(-1, Hkv * D)
        vn[sel] = v_r[:, positions[sel]].transpose(0, 1).reshape(-1, Hkv * D)
    res["k"] = R.check(kn, (ref[:, Hq * D:(Hq + Hkv) * D], bnd[:, Hq * D:(Hq + Hkv) * D]), f"{what}: new K rows")
    res["v"] = R.check(vn, (ref[:, (Hq + Hkv) * D:], bnd[:, (Hq + Hkv) * D:]), f"{what}: new V rows")
    res["attn"] = R.check(attn, R.attention_stage(q, kk, vv, positions, Hkv, D), f"{what}: attention")
    _, _, x1, x1d = R.residual_stage(x0, x0d, attn, mats["wo"], lw.bo, chain)
    res["act"] = R.check(act, R.mlp_stage(c, lw, mats["w_up"], x1, x1d, chain), f"{what}: activation")
    ref, bnd, _, _ = R.residual_stage(x1, x1d, act, mats["w_down"], lw.b_down, chain)
    res["x"] = R.check(x2, (ref, bnd), f"{what}: residual")
    if logits is not None:
        res["logits"] = R.check(logits, R.head_stage(c, mw, mats["head"], x2, chain), f"{what}: logits")
    print(f"[stage/bound] {what}: " + " ".join(f"{k} {v:.3f}" for k, v in res.items()))
    return res
