"""fp64 references of the stages of a one-layer forward, each with a per-element error bound derived from the arithmetic
of the device's kernels (test infrastructure: no conftest, imported by the stage tests).

Every function is plain torch in float64 and runs on the device of its inputs. Each returns `(reference, bound)`: the
value the stage computes in exact arithmetic from the inputs it is given, and a bound B such that a correct kernel meets
|device - reference| <= B element by element. Inputs are the bf16 values the kernel actually read wherever the forward
exposes them (embedding rows, the q tap, the KV cache, the attention / activation / residual taps); where it does not
(the normalised rows inside a GEMV prologue, the residual row after the out-projection) the input is recomputed in fp64
and its possible rounding flips are added to the bound (term 3).

The bound of an element with reference value r, summed from:

 1. Output rounding. The kernel rounds an fp32 value y to bf16 with round-to-nearest-even, so the stored value is within
    half a bf16 spacing of y; y itself is within the terms below of r. Half the spacing of bf16 values at |r| + E
    (E = the sum of the other terms; the larger magnitude covers a y across a binade edge). Near a rounding midpoint
    the stored value may be either neighbour of r: that is this term plus E, not a separate allowance.
 2. fp32 accumulation of a matrix product: n * 2^-24 * (|A| @ |B|), with n the longest chain of fp32 additions any
    kernel uses for one output. This project's kernels (gemv / gemm_skinny / gemm_pipe / persist / prefill_mfma) chain
    16x16x32 MFMA steps (K / 32 of them), the MFMA's internal sum of 32 products, at most 16 split-K partials and the
    fp8 row-scale multiply: n = K / 32 + 64 covers all of it. rocBLAS may use MFMAs of 8 k per step: n = K / 8 + 64.
    fp8 storage: A @ B is taken over the dequantised weights (q * scale), which the device multiplies exactly.
    Bias adds, the residual add and RoPE add fp32 roundings of their own (2^-24 of each operand's magnitude).
 3. Rounding flips of inputs the test cannot see. A normalised row x_k = bf16(bf16(x * rs) * w) (RMSNorm, HF rounding
    points) uses an fp32 statistic rs: its relative error is taken as 2^-20, plus the relative change of rs that any
    possible flip of the row's own inputs causes. Where x * rs lies within that of a bf16 midpoint the kernel may hold
    the other neighbour: |x_k(other) - x_k| * |w_k| is added for that k (GPT-2 LayerNorm alike, with the mean's error).
    The residual row after the out-projection x1 = bf16(x0 + y) flips where x0 + y lies within term 2 of a midpoint.
 4. Non-linear epilogues propagate the input error e through the derivative: |f'(y)| e + sup|f''| e^2 / 2 (SwiGLU:
    sup|silu''| = 1/2; GPT-2 gelu_new: 0.8), plus the relative error of __expf / tanhf (2^-22 (1 + |argument|)).
 5. Attention. P is rounded to bf16 before the PV product while the denominator sums fp32 p: a relative error of
    2^-8 per p, i.e. 2^-8 * sum_s p_s |v_sc| / sum_s p_s for channel c. __expf adds 2^-22 (1 + |argument|) relative per
    p, the rescalings of the running maxima one such error per 32-key block; the scores carry term 2 over D (n = D / 32
    + 64) times the scale. The PV sums carry term 2 over the keys (n = S / 32 + 64).

Bounds are fixed by this analysis, not fitted to runs: a failing element means the kernel or the analysis is wrong.
"""

from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

F64 = torch.float64
U32 = 2.0 ** -24          # unit roundoff of fp32
NORM_REL = 2.0 ** -20     # relative error of a kernel's fp32 row statistic (rsqrt of a fp32 sum of squares)
EXP_REL = 2.0 ** -22      # __expf / tanhf: relative error per unit of argument magnitude (plus one)
SILU_D2, GELU_D2 = 0.5, 0.8


def chain_hip(K: int) -> float:
    return K / 32 + 64


def chain_rocblas(K: int) -> float:
    return K / 8 + 64


# ---- bf16 grid in fp64 ---------------------------------------------------------------------------------------------------------
def bf16_spacing(x: torch.Tensor) -> torch.Tensor:
    """spacing of bf16 values at |x| (normal range; below 2^-126 the subnormal spacing)"""
    a = x.abs().clamp_min(2.0 ** -126)
    return torch.exp2(torch.floor(torch.log2(a)) - 7.0)


def bf16_neighbours(x: torch.Tensor, tol: Optional[torch.Tensor] = None):
    """(round-to-nearest-even of x, the other bf16 neighbour of x, |x - midpoint| <= tol) — exact in fp64"""
    sp = bf16_spacing(x)
    lo = torch.floor(x / sp) * sp
    hi = lo + sp
    mid = lo + sp / 2
    lo_even = torch.remainder(torch.round(lo / sp), 2) == 0
    take_lo = (x < mid) | ((x == mid) & lo_even)
    r = torch.where(take_lo, lo, hi)
    alt = torch.where(take_lo, hi, lo)
    near = torch.zeros_like(x, dtype=torch.bool) if tol is None else (x - mid).abs() <= tol
    return r, alt, near


def rne(x: torch.Tensor) -> torch.Tensor:
    return bf16_neighbours(x)[0]


def finish(ref: torch.Tensor, err: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """term 1 on top of the fp32 error bound `err`"""
    return ref, err + 0.5 * bf16_spacing(ref.abs() + err)


# ---- norms with their possible flips (term 3) ----------------------------------------------------------------------------------
def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, x_delta: Optional[torch.Tensor] = None, detail: bool = False):
    """HF LlamaRMSNorm rounding points: bf16(bf16(x * rs) * w). x: exact bf16 values [T][d] (x_delta: how far the kernel's
    own x may be from x, per element). -> (normalised rows, per-element flip magnitude); detail (x_delta None): also the
    share of the allowed statistic error a kernel needs to round an element to the other neighbour (<= 1 where a flip is allowed)"""
    x, w = x.to(F64), w.to(F64)
    d = x.shape[-1]
    ss = (x * x).sum(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(ss / d + eps)
    rel = torch.full_like(rs, NORM_REL)
    if x_delta is not None:   # a flip of x_k moves the statistic: d(rs)/rs = -x dx / (sum x^2 + d eps)
        rel = rel + (x.abs() * x_delta + x_delta * x_delta).sum(-1, keepdim=True) / (ss + d * eps)
    t = x * rs
    r1, alt1, near = bf16_neighbours(t, rel * t.abs())
    xn = rne(r1 * w)
    delta = torch.where(near, (rne(alt1 * w) - xn).abs(), torch.zeros_like(xn))
    if x_delta is not None:   # the kernel's own x_k: either neighbour of it, normalised with either rounding
        moved = x_delta > 0
        for xs in (x + x_delta, x - x_delta):
            ta = xs * rs
            ra, aa, _ = bf16_neighbours(ta)
            for cand in (ra, aa):
                delta = torch.where(moved, torch.maximum(delta, (rne(cand * w) - xn).abs()), delta)
    if detail:
        return xn, delta, (t - (r1 + alt1) / 2).abs() / (rel * t.abs()).clamp_min(2.0 ** -300)
    return xn, delta


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float, x_delta: Optional[torch.Tensor] = None, detail: bool = False):
    """GPT-2 LayerNorm, rounded once: bf16((x - mean) * rs * w + b), fp32 statistics (mean, then the variance around it);
    detail: as rmsnorm"""
    x, w, b = x.to(F64), w.to(F64), b.to(F64)
    d = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    var = ((x - mean) ** 2).mean(-1, keepdim=True)
    rs = 1.0 / torch.sqrt(var + eps)
    t = (x - mean) * rs * w + b
    rel = torch.full_like(rs, NORM_REL)
    if x_delta is not None:
        rel = rel + ((x - mean).abs() * x_delta + x_delta * x_delta).sum(-1, keepdim=True) / (d * (var + eps))
    tol = rel * ((x.abs() + mean.abs()) * rs * w.abs() + b.abs())
    if x_delta is not None:
        tol = tol + (x_delta + x_delta.sum(-1, keepdim=True) / d) * rs * w.abs()
    # every bf16 value the kernel may have stored: t within tol, rounded
    xn = rne(t)
    delta = torch.maximum((rne(t - tol) - xn).abs(), (rne(t + tol) - xn).abs())
    if detail:
        r, alt, _ = bf16_neighbours(t)
        return xn, delta, (t - (r + alt) / 2).abs() / tol.clamp_min(2.0 ** -300)
    return xn, delta


def norm(cfg, x, w, b, x_delta=None):
    if cfg.arch == 0:
        return rmsnorm(x, w, cfg.norm_eps, x_delta)
    return layernorm(x, w, b, cfg.norm_eps, x_delta)


def product(xn: torch.Tensor, delta: torch.Tensor, W: torch.Tensor, chain: float):
    """(Y = xn @ W^T in fp64, its error bound: fp32 accumulation + the inputs' flips)"""
    W = W.to(F64)
    Wa = W.abs()
    y = xn @ W.t()
    err = chain * U32 * (xn.abs() @ Wa.t())
    if bool((delta > 0).any()):
        err = err + delta @ Wa.t()
    return y, err


# ---- stages ----------------------------------------------------------------------------------------------------------------------
def embed(cfg, weights, tokens: torch.Tensor, positions: torch.Tensor):
    """residual rows entering layer 0: (x0, None) — Llama: the embedding rows; GPT-2: bf16(tok + pos) of the fp32 sum the
    embedding kernel forms, rounded to nearest even (exact: no flip)"""
    x = weights.tok_emb[tokens]
    if cfg.arch == 0:
        return x.to(F64), None
    t = x.float() + weights.pos_emb[positions.clamp(0, cfg.max_pos - 1)].float()
    return rne(t.to(F64)), None


def qkv_stage(cfg, lw, W, x0, x0_delta, positions, rope_cos, rope_sin, chain):
    """norm + QKV product (+ bias) + RoPE -> (ref, bound) of [T][(Hq + 2 Hkv) D] in HF column order (q heads, k heads, v heads)"""
    Hq, Hkv, D = cfg.n_heads, cfg.n_kv_heads, cfg.head_dim
    xn, dl = norm(cfg, x0, lw.attn_norm_w, lw.attn_norm_b, x0_delta)
    y, err = product(xn, dl, W, chain(cfg.d_model))
    if lw.bqkv is not None:
        y = y + lw.bqkv.to(F64)
        err = err + U32 * y.abs()
    if cfg.arch == 0:
        T = y.shape[0]
        half = D // 2
        yh = y.view(T, Hq + 2 * Hkv, 2, half)
        eh = err.view(T, Hq + 2 * Hkv, 2, half)
        c = rope_cos[positions].to(F64).unsqueeze(1)      # [T][1][half], the model's fp32 tables
        s = rope_sin[positions].to(F64).unsqueeze(1)
        y0, y1, e0, e1 = yh[:, :, 0], yh[:, :, 1], eh[:, :, 0], eh[:, :, 1]
        o0 = y0 * c - y1 * s
        o1 = y1 * c + y0 * s
        f0 = e0 * c.abs() + e1 * s.abs() + 2 * U32 * ((y0 * c).abs() + (y1 * s).abs())
        f1 = e1 * c.abs() + e0 * s.abs() + 2 * U32 * ((y1 * c).abs() + (y0 * s).abs())
        rope = torch.arange(Hq + 2 * Hkv, device=y.device) < Hq + Hkv        # V heads are not rotated
        o0 = torch.where(rope[None, :, None], o0, y0)
        o1 = torch.where(rope[None, :, None], o1, y1)
        f0 = torch.where(rope[None, :, None], f0, e0)
        f1 = torch.where(rope[None, :, None], f1, e1)
        y = torch.stack([o0, o1], 2).reshape(T, -1)
        err = torch.stack([f0, f1], 2).reshape(T, -1)
    return finish(y, err)


def attention_stage(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_pos: torch.Tensor, n_kv_heads: int,
                    head_dim: int, key_pos: Optional[torch.Tensor] = None):
    """q: bf16 [T][Hq*D] (the q tap); k, v: bf16 [T][Hkv][S][D] — the keys each query row's cache holds; q_pos: [T] absolute
    position of each query (key s is visible to it when s <= q_pos). -> (ref, bound) [T][Hq*D]"""
    T = q.shape[0]
    D, Hkv = head_dim, n_kv_heads
    Hq = q.shape[1] // D
    G = Hq // Hkv
    S = k.shape[2]
    scale = 1.0 / math.sqrt(D)
    qh = q.to(F64).view(T, Hkv, G, D)
    kd, vd = k.to(F64), v.to(F64)
    dot = torch.einsum("thgd,thsd->thgs", qh, kd)
    dabs = torch.einsum("thgd,thsd->thgs", qh.abs(), kd.abs())
    kp = torch.arange(S, device=q.device) if key_pos is None else key_pos
    vis = kp.view(1, 1, 1, S) <= q_pos.view(T, 1, 1, 1)
    sc = torch.where(vis, dot * scale, torch.full_like(dot, -math.inf))
    m = sc.amax(-1, keepdim=True)
    p = torch.exp(sc - m)
    den = p.sum(-1, keepdim=True)
    num = torch.einsum("thgs,thsd->thgd", p, vd)
    nabs = torch.einsum("thgs,thsd->thgd", p, vd.abs())
    out = num / den
    # relative error of each p_s: score error (term 2 over D, times the scale) + __expf at its argument
    arg = torch.where(vis, (sc - m).abs(), torch.zeros_like(sc))
    eps_s = scale * chain_hip(D) * U32 * dabs + EXP_REL * (1 + arg) + 2 * U32 * scale * dot.abs()
    eps_s = torch.where(vis, eps_s, torch.zeros_like(eps_s))
    # the running-max rescalings: one __expf per 32-key block and per merge (4 waves, <= 32 split partials)
    n_blk = (q_pos.view(T, 1, 1, 1).to(F64) + 1) / 32 + 40
    rng = torch.where(vis, arg, torch.zeros_like(arg)).amax(-1, keepdim=True)
    eps_c = n_blk * EXP_REL * (1 + rng)
    w_eps = torch.einsum("thgs,thsd->thgd", p * eps_s, vd.abs()) / den + (p * eps_s).sum(-1, keepdim=True) / den * out.abs()
    chain_pv = (q_pos.view(T, 1, 1, 1).to(F64) + 1) / 32 + 64
    err = (2.0 ** -8 + 2 * eps_c + chain_pv * U32) * nabs / den + w_eps + 2 * eps_c * out.abs() + U32 * out.abs()
    return finish(out.reshape(T, Hq * D), err.reshape(T, Hq * D))


def residual_stage(x: torch.Tensor, x_delta: Optional[torch.Tensor], rows: torch.Tensor, W: torch.Tensor,
                   bias: Optional[torch.Tensor], chain):
    """x + rows @ W^T (+ bias): the out-projection (rows: the attention tap) or the down-projection (rows: the activation
    tap). -> (ref, bound, flip magnitude of the stored row). The flip magnitude is what the next stage needs when the
    stored row is not visible (x1)."""
    y, err = product(rows.to(F64), torch.zeros(1, device=rows.device, dtype=F64), W, chain(rows.shape[1]))
    if bias is not None:
        y = y + bias.to(F64)
        err = err + U32 * y.abs()
    t = x.to(F64) + y
    err = err + U32 * t.abs()
    if x_delta is not None:
        err = err + x_delta
    ref, bound = finish(t, err)
    # every bf16 value the kernel may have stored: within `err` of t, rounded
    lo, hi = rne(t - err), rne(t + err)
    r = rne(t)
    flip = torch.maximum((lo - r).abs(), (hi - r).abs())
    return ref, bound, r, flip


def mlp_stage(cfg, lw, W_up, x1, x1_delta, chain):
    """norm + gate / up product + SwiGLU (GPT-2: + bias, gelu_new) -> (ref, bound) [T][d_ff]"""
    ff = cfg.d_ff
    xn, dl = norm(cfg, x1, lw.mlp_norm_w, lw.mlp_norm_b, x1_delta)
    y, err = product(xn, dl, W_up, chain(cfg.d_model))
    if cfg.arch == 0:
        g, u, eg, eu = y[:, :ff], y[:, ff:], err[:, :ff], err[:, ff:]
        sg = torch.sigmoid(g)
        silu = g * sg
        dsilu = (sg * (1 + g * (1 - sg))).abs() + SILU_D2 * eg
        act = silu * u
        e = dsilu * eg * (u.abs() + eu) + silu.abs() * eu + act.abs() * (EXP_REL * (1 + g.abs()) + 3 * U32)
        return finish(act, e)
    y = y + lw.b_up.to(F64)
    err = err + U32 * y.abs()
    c = 0.7978845608028654
    inner = c * (y + 0.044715 * y ** 3)
    th = torch.tanh(inner)
    gel = 0.5 * y * (1 + th)
    dgel = (0.5 * (1 + th) + 0.5 * y * (1 - th * th) * c * (1 + 3 * 0.044715 * y * y)).abs() + GELU_D2 * err
    e = dgel * err + 0.5 * y.abs() * EXP_REL * (1 + inner.abs()) + 4 * U32 * gel.abs()
    return finish(gel, e)


def head_stage(cfg, weights, W_head, x, chain):
    """final norm + lm_head over the residual rows x (the device's hidden rows) -> (ref, bound) [T][V]"""
    xn, dl = norm(cfg, x, weights.final_norm_w, weights.final_norm_b)
    y, err = product(xn, dl, W_head, chain(cfg.d_model))
    return finish(y, err)


def head_stage_normed(xn: torch.Tensor, W_head: torch.Tensor, chain):
    """a head over rows that are final-norm outputs already (the EAGLE step's extrapolated rows; sd_model_head_argmax with
    SD_HEADS_NORMALISED): the product alone. xn: the exact bf16 rows the kernel reads -> (ref, bound) [T][V]. The value the
    argmax epilogue compares and reports is the bf16-ROUNDED product (epilogue<EPI_ARGMAX>, csrc/gemv_device.h), so the
    output rounding term stays."""
    xn = xn.to(F64)
    y, err = product(xn, torch.zeros(1, device=xn.device, dtype=F64), W_head, chain(xn.shape[-1]))
    return finish(y, err)


def gemv_geometry(n_pairs: int, K: int) -> dict:
    """The work split of one matrix over the chip (csrc/pack.hip, gemv_geometry), restated: the tests pick shapes and tie
    positions from it. grid workgroups own ppw consecutive row pairs each, cut into n_tiles tiles of tile_pairs pairs;
    ksplit K slices per tile."""
    grid = min(256, n_pairs)
    ppw = -(-n_pairs // grid)
    grid = -(-n_pairs // ppw)
    n_tiles = 1
    while n_tiles * 8 < ppw:
        n_tiles *= 2
    tile_pairs = -(-ppw // n_tiles)
    ksplit = 16 // min(n_tiles, 16)
    while ksplit > 1 and -(-K // (ksplit * 32)) < 2:
        ksplit //= 2
    return dict(grid=grid, ppw=ppw, n_tiles=n_tiles, tile_pairs=tile_pairs, ksplit=ksplit, kw=-(-K // (ksplit * 32)) * 32)


def check_head_argmax(ids: torch.Tensor, vals: torch.Tensor, ref_bound, what: str) -> float:
    """ids / vals [B][n_heads] (row-major, as sd_model_head_argmax returns them) against (ref, bound) [n_heads][B][V]:
    for every (head j, row b), with id = ids[b][j],
      |vals[b][j] - ref[j][b][id]| <= bound[j][b][id]                  the value the kernel attached to its winner is that logit
      ref[j][b][id] >= max_v ref[j][b][v] - 2 max_v bound[j][b][v]     and no other logit can have been the larger one
    (every computed logit is within its bound of ref, so the computed maximum is at least max(ref) - max(bound), and the
    winner's reference is within its own bound of that). Holds for every correct kernel on every row: none is excluded.
    -> worst |value - ref[id]| / bound[id]"""
    ref, bound = ref_bound
    nh, B, V = ref.shape
    assert tuple(ids.shape) == (B, nh) and tuple(vals.shape) == (B, nh), (tuple(ids.shape), tuple(vals.shape), (B, nh))
    idx = ids.t().long()
    if bool(((idx < 0) | (idx >= V)).any()):
        raise AssertionError(f"{what}: an id outside [0, {V}): {ids.tolist()}")
    r_at = ref.gather(2, idx.unsqueeze(-1)).squeeze(-1)
    b_at = bound.gather(2, idx.unsqueeze(-1)).squeeze(-1)
    ratio = (vals.t().to(F64) - r_at).abs() / b_at
    worst = float(ratio.max())
    if not worst <= 1.0:
        j, b = (int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))
        raise AssertionError(f"{what}: head {j} row {b}: value {float(vals[b, j]):.6g} at id {int(ids[b, j])}, reference "
                             f"{float(r_at[j, b]):.6g}, bound {float(b_at[j, b]):.3g} ({worst:.2f} x)")
    slack = ref.amax(-1) - 2 * bound.amax(-1) - r_at
    if bool((slack > 0).any()):
        j, b = (int(v) for v in torch.unravel_index(slack.argmax(), slack.shape))
        raise AssertionError(f"{what}: head {j} row {b}: id {int(ids[b, j])} has reference {float(r_at[j, b]):.6g}, but index "
                             f"{int(ref[j, b].argmax())} has {float(ref[j, b].max()):.6g} (2 x worst bound {2 * float(bound[j, b].max()):.3g})")
    return worst


def tie_copies(V: int, d: int, r: int) -> list:
    """indices that get a copy of a head's winning row `r` in the tie tests, placed by the work split of a [V][d] head: BOTH
    slots of one row pair (one lane of the argmax epilogue compares them), a second pair of that tile, another tile of the same
    workgroup, another workgroup, the workgroup 64 further on (which the finalize folds in the same lane), and the last two
    rows of the vocabulary (for an odd V: the second slot of the last full pair and the first slot of a pair whose second row
    does not exist) -> sorted, with r itself"""
    n_pairs = (V + 1) // 2
    g = gemv_geometry(n_pairs, d)
    p0 = g["ppw"] * min(3, g["grid"] - 1)                         # first pair of a workgroup
    other_tile = p0 + (g["tile_pairs"] if g["n_tiles"] > 1 else 0)
    other_wg = min(p0 + g["ppw"] * 5, n_pairs - 1)
    same_lane = min(p0 + g["ppw"] * 64, n_pairs - 1)              # 64 workgroups on: the same lane of the finalize's fold over workgroups
    cand = [2 * p0, 2 * p0 + 1, 2 * (p0 + min(1, g["ppw"] - 1)), 2 * other_tile, 2 * other_wg + 1, 2 * same_lane, V - 2, V - 1, r]
    return sorted({c for c in cand if 0 <= c < V})


def plant_ties(head: torch.Tensor, r: int, positions) -> torch.Tensor:
    """a copy of `head` (bf16 [V][d]) whose rows at `positions` hold 2 x row r — exact in bf16, and exact under the fp8
    row quantiser too (the scale doubles, the codes stay) — so that their logits tie exactly and clear every other row's"""
    out = head.clone()
    out[torch.as_tensor(list(positions), device=head.device)] = (head[r].float() * 2).to(head.dtype)
    return out


def check_ties(ids_row: torch.Tensor, vals_row: torch.Tensor, copies, ref_bound, b: int, what: str) -> None:
    """row b of a call over the heads [all `copies` planted] + [copy i alone for every i] (plant_ties): the first head must
    return the lowest of the copies, head 1 + i its only copy, and all returned values are the same bits — the planted rows
    are identical, so their sums tie exactly wherever the work split puts them. The planted logit must clear every other
    logit of the row by more than the bounds (checked first, from the reference: the construction's precondition)."""
    ref, bound = ref_bound
    r0 = ref[0, b]
    other = torch.ones_like(r0, dtype=torch.bool)
    other[torch.as_tensor(list(copies), device=r0.device)] = False
    gap = float(r0[~other].min() - r0[other].max())
    assert gap > 2 * float(bound[0, b].max()), f"{what}: the planted rows do not clear the rest ({gap:.3g}): pick another row"
    got = [int(v) for v in ids_row.tolist()]
    if got[0] != min(copies):
        raise AssertionError(f"{what}: copies at {list(copies)}: the kernel returned {got[0]}, not the lowest")
    if got[1:] != list(copies):
        raise AssertionError(f"{what}: single copies at {list(copies)} returned as {got[1:]}")
    if not bool((vals_row.view(torch.int32) == vals_row.view(torch.int32)[0]).all()):
        raise AssertionError(f"{what}: the copies' values differ: {vals_row.tolist()} (the ties were not exact)")


# ---- EAGLE extrapolation (eagle_extrapolate_kernel, csrc/misc.hip) -----------------------------------------------------------
def eagle_recurrence(h_t: torch.Tensor, prev: torch.Tensor, has_prev: torch.Tensor, alpha: float, K: int):
    """Everything after the norm, restated: elementwise fp32 with three bf16 roundings per step, no reduction, so a correct
    kernel matches it bit for bit. h_t, prev: bf16 [B][d] (the device's own bits); has_prev [B]; alpha is used as a float32.
      prv = prev if has_prev else h_t;  cur = h_t
      diff = bf16(cur - prv);  sc = bf16(float32(alpha) * diff);  h = bf16(cur + sc);  prv, cur = cur, h
    -> (H bf16 [B][K][d], state E = h_K bf16 [B][d])"""
    a = torch.tensor(alpha, dtype=torch.float32, device=h_t.device)
    cur = h_t.float()
    prv = torch.where(has_prev.view(-1, 1) != 0, prev.float(), cur)
    rows = []
    for _ in range(K):
        diff = (cur - prv).bfloat16().float()
        sc = (a * diff).bfloat16().float()
        h = (cur + sc).bfloat16()
        rows.append(h)
        prv, cur = cur, h.float()
    return torch.stack(rows, 1), rows[-1]


def check_eagle_norm(h_t: torch.Tensor, x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], eps: float, rms: bool,
                     what: str):
    """the kernel's h_t (bf16 [B][d]: row 0 of a call with has_prev = 0) against the fp64 norm of x: each element equals the
    reference's rounding unless the reference arithmetic itself (an fp32 statistic: two-pass for LayerNorm) could have
    rounded to the other neighbour, and then differs by at most that flip (rmsnorm / layernorm above).
    -> (elements on the other neighbour, the largest share of the allowed statistic error any of them needed to get there)"""
    xn, delta, need = rmsnorm(x, w, eps, detail=True) if rms else layernorm(x, w, b, eps, detail=True)
    err = (h_t.to(F64) - xn).abs()
    bad = err > delta
    if bool(bad.any()):
        i = int((err - delta).argmax())
        r, c = (int(v) for v in torch.unravel_index(torch.tensor(i), err.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {err.numel()} elements outside the derived bound; worst at [{r}, {c}]: "
                             f"got {float(h_t[r, c]):.6g}, reference {float(xn[r, c]):.6g}, allowed flip {float(delta[r, c]):.3g}")
    moved = err > 0
    worst = float(need[moved].max()) if bool(moved.any()) else 0.0
    return int(moved.sum()), worst


def check_eagle_exact(H, prev_out, has_out, h_t, prev_in, has_in, alpha: float, what: str) -> None:
    """H [B][K][d], the stored state and flags of one call against the restated recurrence from the device's own h_t and
    prev bits: bit for bit"""
    K = H.shape[1]
    want_H, want_E = eagle_recurrence(h_t, prev_in, has_in, alpha, K)
    for name, got, want in (("H", H, want_H), ("state", prev_out, want_E)):
        ne = got.view(torch.int16) != want.view(torch.int16)
        if bool(ne.any()):
            idx = [int(v[0]) for v in ne.nonzero(as_tuple=True)]
            raise AssertionError(f"{what}: {name} differs from the restated recurrence in {int(ne.sum())} of {ne.numel()} elements; first at "
                                 f"{idx}: got {float(got[tuple(idx)]):.6g}, want {float(want[tuple(idx)]):.6g}")
    if not bool((has_out == 1).all()):
        raise AssertionError(f"{what}: has_prev after the call is {has_out.tolist()}, want all 1")


def check(got: torch.Tensor, ref_bound, what: str) -> float:
    """assert |got - ref| <= bound everywhere; -> worst |got - ref| / bound"""
    ref, bound = ref_bound
    err = (got.to(F64) - ref).abs()
    ratio = err / bound
    worst = float(ratio.max())
    if not worst <= 1.0:
        i = int(ratio.argmax())
        idx = [int(v) for v in torch.unravel_index(torch.tensor(i), ratio.shape)]
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.numel()} elements outside the derived bound; worst at "
                             f"{idx}: got {float(got.reshape(-1)[i]):.6g}, reference {float(ref.reshape(-1)[i]):.6g}, "
                             f"bound {float(bound.reshape(-1)[i]):.3g} ({worst:.2f} x)")
    return worst
