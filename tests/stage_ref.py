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
def rmsnorm(x: torch.Tensor, w: torch.Tensor, eps: float, x_delta: Optional[torch.Tensor] = None):
    """HF LlamaRMSNorm rounding points: bf16(bf16(x * rs) * w). x: exact bf16 values [T][d] (x_delta: how far the kernel's
    own x may be from x, per element). -> (normalised rows, per-element flip magnitude)"""
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
    return xn, delta


def layernorm(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, eps: float, x_delta: Optional[torch.Tensor] = None):
    """GPT-2 LayerNorm, rounded once: bf16((x - mean) * rs * w + b), fp32 statistics"""
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
