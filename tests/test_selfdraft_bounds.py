"""The self-drafting references of tests/stage_ref.py have teeth (CPU only).

The Medusa-head evaluation and the EAGLE extrapolation are emulated in float32 with the device's rounding points, on
`random_init`-style inputs without successor structure. Each emulation must pass the checks the GPU tests apply
(tests/test_hip_selfdraft_fp64_gpu.py), and each named mutation of it — a bug the kernels or the step's wiring could have,
none of which changes a token on the engineered weights of the pipeline tests — must fail at least one."""

import numpy as np
import pytest
import torch

import stage_ref as R
from selfdraft_cases import eagle_inputs, eagle_protocol, hidden_rows, random_heads
from oracle.fp8_ref import quantize_rows
from specdec_hip import weights as W

LLAMA = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=1, d_model=256, n_heads=4, n_kv_heads=2, head_dim=64, d_ff=256, vocab=1001,
                      max_pos=256, rope_theta=500000.0, tie_embeddings=False, name="heads-llama")
GPT2 = W.ModelConfig(arch=W.ARCH_GPT2, n_layers=1, d_model=256, n_heads=4, n_kv_heads=4, head_dim=64, d_ff=256, vocab=1001,
                     max_pos=256, tie_embeddings=False, name="heads-gpt2")


def _bf(x):
    return x.to(torch.bfloat16).float()


# ---- Medusa heads -----------------------------------------------------------------------------------------------------------------
def emu_heads(mw, x, rows, heads, wd="bf16", normalised=False, mut=None, K=None):
    """float32 emulation of enqueue_head_argmax: gather, final norm (fp32 statistics, the rounding points of the
    architecture), bf16 x bf16 products accumulated in fp32, fp8 row scales on the accumulator, bf16 logits, argmax with
    ties to the lower index -> (ids int32 [B][n_heads], values float32 [B][n_heads])"""
    c = mw.config
    rows = torch.as_tensor(rows)
    if mut == "row_base":
        rows = rows // (K + 1) * (K + 1)
    xs = x[rows].float()
    if normalised:
        xn = xs
    elif c.arch == W.ARCH_LLAMA:
        rs = torch.rsqrt((xs * xs).sum(-1, keepdim=True) / c.d_model + c.norm_eps)
        xn = _bf(_bf(xs * rs) * mw.final_norm_w.float())
    else:
        mean = xs.mean(-1, keepdim=True)
        rs = torch.rsqrt(((xs - mean) ** 2).mean(-1, keepdim=True) + c.norm_eps)
        xn = _bf((xs - mean) * rs * mw.final_norm_w.float() + mw.final_norm_b.float())
    nh, B = heads.shape[0], rows.numel()
    mats = [quantize_rows(h) if wd == "fp8" else (h.float(), None) for h in heads]
    ids = torch.empty(nh, B, dtype=torch.int32)
    vals = torch.empty(nh, B)
    for j, (q, s) in enumerate(mats):
        xj = xn
        if mut == "drop_k" and j == nh - 1:
            xj = xn.clone()
            xj[:, 64:96] = 0
        y = xj @ q.float().t()
        if s is not None:
            y = y * (mats[j - 1][1] if mut == "scale_prev_head" and j > 0 else s)
        y = _bf(y)
        top = y.max(-1, keepdim=True).values
        where = (y == top) * torch.arange(1, y.shape[1] + 1)
        ids[j] = (where.max(-1).values if mut == "tie_high" else torch.where(where > 0, where, y.shape[1] + 1).min(-1).values) - 1
        vals[j] = top[:, 0]
    if mut == "layout_swap":       # head-major results stored without the transpose
        return ids.reshape(B, nh), vals.t().contiguous()
    return ids.t().contiguous(), vals.t().contiguous()


def ref_heads(mw, x, rows, heads, wd="bf16", normalised=False):
    """(ref, bound) [n_heads][B][V] of tests/stage_ref.py for the same call"""
    xs = x[torch.as_tensor(rows)]
    out = []
    for h in heads:
        if wd == "fp8":
            q, s = quantize_rows(h)
            m = q.double() * s.double()[:, None]
        else:
            m = h.double()
        out.append(R.head_stage_normed(xs, m, R.chain_hip) if normalised else R.head_stage(mw.config, mw, m, xs, R.chain_hip))
    return torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])


HEAD_CASES = [(LLAMA, "bf16", False), (LLAMA, "fp8", False), (GPT2, "bf16", False), (LLAMA, "bf16", True), (LLAMA, "fp8", True)]


@pytest.mark.parametrize("cfg,wd,normalised", HEAD_CASES, ids=[f"{c.name}-{w}-{'normed' if n else 'norm'}" for c, w, n in HEAD_CASES])
def test_head_emulation_within_bounds(cfg, wd, normalised):
    mw = W.random_init(cfg, seed=1)
    K, B = 3, 4
    heads = random_heads(K, cfg.vocab, cfg.d_model, 2)
    x = hidden_rows(B * (K + 1), cfg.d_model, 3)
    rows = [b * (K + 1) + a for b, a in enumerate([2, 0, 3, 1])]
    ids, vals = emu_heads(mw, x, rows, heads, wd, normalised)
    worst = R.check_head_argmax(ids, vals, ref_heads(mw, x, rows, heads, wd, normalised), f"{cfg.name} {wd}")
    assert worst <= 1.0
    # a non-monotone permutation with repeats
    rows = [7, 0, 7, 3]
    ids, vals = emu_heads(mw, x, rows, heads, wd, normalised)
    R.check_head_argmax(ids, vals, ref_heads(mw, x, rows, heads, wd, normalised), f"{cfg.name} {wd} permuted rows")
    assert torch.equal(ids[0], ids[2]) and torch.equal(vals[0], vals[2])


@pytest.mark.parametrize("mut,wd", [("drop_k", "bf16"), ("scale_prev_head", "fp8"), ("row_base", "bf16"), ("layout_swap", "bf16")])
def test_head_mutation_is_caught(mut, wd):
    mw = W.random_init(LLAMA, seed=1)
    K, B = 3, 4
    heads = random_heads(K, LLAMA.vocab, LLAMA.d_model, 2)
    x = hidden_rows(B * (K + 1), LLAMA.d_model, 3)
    rows = [b * (K + 1) + a for b, a in enumerate([2, 0, 3, 1])]
    ref = ref_heads(mw, x, rows, heads, wd)
    R.check_head_argmax(*emu_heads(mw, x, rows, heads, wd), ref, "unmutated")
    with pytest.raises(AssertionError, match="head \\d row \\d"):
        R.check_head_argmax(*emu_heads(mw, x, rows, heads, wd, mut=mut, K=K), ref, mut)


def _tie_case(mw, wd, seed):
    """one row, its fp64 winner of a random head, and the heads of the tie test: all copies planted, then each copy alone"""
    c = mw.config
    base = random_heads(1, c.vocab, c.d_model, seed)[0]
    x = hidden_rows(1, c.d_model, seed + 1)
    r = int(ref_heads(mw, x, [0], base[None], wd)[0][0, 0].argmax())
    copies = R.tie_copies(c.vocab, c.d_model, r)
    heads = torch.stack([R.plant_ties(base, r, copies)] + [R.plant_ties(base, r, [p]) for p in copies])
    return x, r, copies, heads


@pytest.mark.parametrize("wd", ["bf16", "fp8"])
def test_ties_go_to_the_lowest_copy(wd):
    mw = W.random_init(LLAMA, seed=1)
    x, r, copies, heads = _tie_case(mw, wd, 11)
    assert len(copies) >= 7 and copies[-2:] == [LLAMA.vocab - 2, LLAMA.vocab - 1]
    ref = ref_heads(mw, x, [0], heads, wd)
    ids, vals = emu_heads(mw, x, [0], heads, wd)
    R.check_head_argmax(ids, vals, ref, "ties")
    R.check_ties(ids[0], vals[0], copies, ref, 0, "ties")
    ids, vals = emu_heads(mw, x, [0], heads, wd, mut="tie_high")
    with pytest.raises(AssertionError, match="lowest"):
        R.check_ties(ids[0], vals[0], copies, ref, 0, "ties to the higher index")


def test_geometry_of_the_gpu_shapes():
    """the shapes of the GPU tests hit the work splits they are chosen for (csrc/pack.hip)"""
    g = R.gemv_geometry(100, 128)
    assert (g["grid"], g["ppw"], g["ksplit"]) == (100, 1, 2)
    g = R.gemv_geometry(2050, 2048)
    assert (g["grid"], g["ppw"], g["n_tiles"], g["tile_pairs"], g["ksplit"]) == (228, 9, 2, 5, 8)
    g = R.gemv_geometry(16501, 256)
    assert (g["n_tiles"], g["ksplit"]) == (16, 1)
    for V, d in ((4099, 2048), (33001, 256)):
        c = R.tie_copies(V, d, V // 2)
        g = R.gemv_geometry((V + 1) // 2, d)
        wg = sorted({(p // 2) // g["ppw"] for p in c})
        tiles = {((p // 2) // g["ppw"], ((p // 2) % g["ppw"]) // g["tile_pairs"]) for p in c}
        assert len(c) == 9 and V % 2 == 1 and c[-2:] == [V - 2, V - 1], c
        assert any(p % 2 == 0 and p + 1 in c for p in c if p + 1 < V - 1), c            # one pair holds a copy in both slots
        assert any(p % 2 == 0 and p + 2 in c for p in c), c                              # two pairs of one tile
        assert any(a[0] == b[0] and a[1] != b[1] for a in tiles for b in tiles), tiles   # two tiles of one workgroup
        assert len(wg) >= 4 and any(b - a == 64 for a in wg for b in wg), wg             # workgroups, two of them in one finalize lane


# ---- EAGLE extrapolation ----------------------------------------------------------------------------------------------------------
def _rne_bf16(a: np.ndarray) -> np.ndarray:
    """float32 -> the nearest bf16 value (ties to even) as float32, on the bits"""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    u = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) & np.uint32(0xFFFF0000)
    return u.view(np.float32)


def emu_eagle(x, prev, has_prev, w, b, eps, alpha, K, rms, mut=None):
    """numpy float32 emulation of eagle_extrapolate_kernel: norm (two-pass LayerNorm statistics), K-step recurrence with the
    three bf16 roundings, state E <- h_K, has_prev <- 1. Inputs are torch bf16 / int32; -> (H, prev_out, has_out) as torch"""
    xf, wf = x.float().numpy(), w.float().numpy()
    bfv = None if b is None else b.float().numpy()
    d = xf.shape[1]
    if mut == "norm_swap":
        rms = not rms
    if rms:
        rs = (1.0 / np.sqrt((xf * xf).sum(-1, keepdims=True, dtype=np.float32) / np.float32(d) + np.float32(eps))).astype(np.float32)
        ht = _rne_bf16(_rne_bf16(xf * rs) * wf)
    else:
        mean = xf.mean(-1, keepdims=True, dtype=np.float32)
        var = ((xf - mean) ** 2).mean(-1, keepdims=True, dtype=np.float32)
        rs = (1.0 / np.sqrt(var + np.float32(eps))).astype(np.float32)
        bias = np.zeros_like(wf) if (bfv is None or mut == "no_bias") else bfv
        ht = _rne_bf16((xf - mean) * rs * wf + bias)
    has = has_prev.numpy().reshape(-1, 1) != 0
    if mut == "ignore_has_prev":
        has = np.ones_like(has)
    prv = np.where(has, prev.float().numpy(), ht)
    cur = ht
    a = np.float32(alpha)
    H = np.empty((xf.shape[0], K, d), dtype=np.float32)
    for k in range(K):
        if mut == "alpha_before_rounding":
            sc = _rne_bf16(a * (cur - prv))
        else:
            sc = _rne_bf16(a * _rne_bf16(cur - prv))
        H[:, k] = _rne_bf16(cur + sc)
        if mut != "prv_not_advanced":
            prv = cur
        cur = H[:, k]
    state = ht if mut == "state_is_h_t" else cur
    return (torch.from_numpy(H).bfloat16(), torch.from_numpy(np.ascontiguousarray(state)).bfloat16(),
            torch.ones(xf.shape[0], dtype=torch.int32))


@pytest.mark.parametrize("form", ["plain", "spikes", "offset"])
@pytest.mark.parametrize("d,rms", [(64, True), (136, True), (768, False), (2048, True)])
def test_eagle_emulation_passes(d, rms, form):
    x, prev, w, b = eagle_inputs(3, d, d, form)
    has = torch.tensor([1, 0, 1], dtype=torch.int32)
    for K, alpha in ((1, 0.7), (4, 0.7), (8, 1.5), (2, 0.0)):
        eagle_protocol(emu_eagle, x, prev, has, w, None if rms else b, 1e-5, alpha, K, rms, f"d={d} {form} K={K} alpha={alpha}")


EAGLE_MUTATIONS = ["prv_not_advanced", "alpha_before_rounding", "state_is_h_t", "ignore_has_prev", "norm_swap", "no_bias"]


@pytest.mark.parametrize("mut", EAGLE_MUTATIONS)
def test_eagle_mutation_is_caught(mut):
    rms = mut != "no_bias"
    x, prev, w, b = eagle_inputs(3, 256, 5, "offset" if mut == "norm_swap" else "plain")
    has = torch.tensor([1, 0, 1], dtype=torch.int32)
    args = (x, prev, has, w, b, 1e-5, 0.7, 4, rms)
    eagle_protocol(emu_eagle, *args, "unmutated")
    with pytest.raises(AssertionError, match="outside the derived bound|differs from the restated recurrence"):
        eagle_protocol(lambda *a: emu_eagle(*a, mut=mut), *args, mut)
