"""The stage bounds of tests/stage_ref.py have teeth (CPU only).

A small emulation of the device's rounding points (bf16 operands, fp32 accumulation, bf16 outputs, fp32 row statistics,
bf16 P in the PV product, fp8 row scales on the fp32 accumulator) runs one layer of a one-layer model on one row: it must
pass every stage check over a grid of shapes and positions, and each named mutation of it — a bug a kernel could have —
must fail at least one. The shapes are those the GPU tests use (tests/test_hip_stage_fp64_gpu.py)."""

import math

import pytest
import torch

import prefill_cases as P
import stage_ref as R
from oracle.fp8_ref import quantize_rows
from specdec_hip import weights as W

TOY = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=1, d_model=256, n_heads=4, n_kv_heads=2, head_dim=64, d_ff=512,
                    vocab=512, max_pos=2048, rope_theta=500000.0, tie_embeddings=False, name="toy")
TOY32 = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=1, d_model=128, n_heads=4, n_kv_heads=2, head_dim=32, d_ff=256,
                      vocab=512, max_pos=2048, rope_theta=500000.0,
                      rope_scaling={"factor": 8.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0,
                                    "original_max_position_embeddings": 64, "rope_type": "llama3"},
                      tie_embeddings=False, name="toy32")
TOY128 = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=1, d_model=384, n_heads=3, n_kv_heads=1, head_dim=128, d_ff=1024,
                       vocab=512, max_pos=2048, rope_theta=500000.0, tie_embeddings=False, name="toy128")
GPT2 = W.ModelConfig(arch=W.ARCH_GPT2, n_layers=1, d_model=256, n_heads=4, n_kv_heads=4, head_dim=64, d_ff=1024,
                     vocab=512, max_pos=1024, tie_embeddings=False, name="gpt2-toy")


def _bf(x):
    return x.to(torch.bfloat16).float()


def _trunc(x):
    return (x.float().view(torch.int32) & -65536).view(torch.float32)


class Emu:
    """One row of M new tokens at positions pos0.. over a cache of pos0 prefix keys, with the device's rounding points."""

    def __init__(self, cfg, weight_dtype="bf16", seed=0, weights=None):
        self.cfg = cfg
        self.w = W.random_init(cfg, seed=seed) if weights is None else weights
        self.fp8 = weight_dtype == "fp8"
        self.mats = {}
        for name in ("wqkv", "wo", "w_up", "w_down"):
            self.mats[name] = self._mat(getattr(self.w.layers[0], name))
        self.mats["head"] = self._mat(self.w.lm_head)

    def _mat(self, m):
        if not self.fp8:
            return m.float(), None
        q, s = quantize_rows(m)
        return q.float(), s

    def ref_matrix(self, name):
        """the matrix the device multiplies by, as the reference sees it (fp8: the dequantised values)"""
        q, s = self.mats[name]
        return q.double() if s is None else q.double() * s.double()[:, None]

    def _product(self, x, name, mut, scale_shift=False, drop=None):
        q, s = self.mats[name]
        if drop is not None:
            x = x.clone()
            x[:, drop[0]:drop[1]] = 0
        y = x.float() @ q.t()
        if s is not None:
            y = y * (torch.roll(s, 1) if scale_shift else s)
        return y

    def _norm(self, x, w, b):
        c = self.cfg
        if c.arch == W.ARCH_LLAMA:
            rs = torch.rsqrt((x * x).sum(-1, keepdim=True) / c.d_model + c.norm_eps)
            return _bf(_bf(x * rs) * w.float())
        mean = x.mean(-1, keepdim=True)
        rs = torch.rsqrt(((x - mean) ** 2).mean(-1, keepdim=True) + c.norm_eps)
        return _bf((x - mean) * rs * w.float() + b.float())

    def run(self, tokens, pos0, k_pre, v_pre, mut=None, spikes=(), stale=0, kv_only=False):
        """tokens [M]; k_pre / v_pre bf16 [Hkv][pos0][D]; `stale` positions after the pass hold old keys (never visible);
        the V rows at `spikes` (any position of the cache) are scaled by 256 in one channel each before the attention.
        -> dict of taps (fp32 holding bf16 values) and the caches (kv_only: the caches alone, no attention and nothing after it)"""
        c, lw = self.cfg, self.w.layers[0]
        Hq, Hkv, D, ff = c.n_heads, c.n_kv_heads, c.head_dim, c.d_ff
        M = tokens.shape[0]
        pos = torch.arange(pos0, pos0 + M)
        x0 = self.w.tok_emb[tokens].float()
        if c.arch == W.ARCH_GPT2:
            x0 = _bf(x0 + self.w.pos_emb[pos].float())
        rnd = _trunc if mut == "truncate" else _bf
        xn = self._norm(x0, lw.attn_norm_w, lw.attn_norm_b)
        y = self._product(xn, "wqkv", mut, scale_shift=(mut == "fp8_scale"))
        if lw.bqkv is not None:
            y = y + lw.bqkv.float()
        yh = y.view(M, Hq + 2 * Hkv, D)
        if c.arch == W.ARCH_LLAMA:
            rp = pos + 1 if mut == "rope_pos" else pos
            cs, sn = self.w.rope_cos[rp][:, None], self.w.rope_sin[rp][:, None]
            a, b = yh[..., : D // 2], yh[..., D // 2:]
            rot = torch.cat([a * cs - b * sn, b * cs + a * sn], -1)
            yh = torch.cat([rot[:, : Hq + Hkv], yh[:, Hq + Hkv:]], 1)
        yh = rnd(yh)
        q = yh[:, :Hq].reshape(M, Hq * D)
        kn, vn = yh[:, Hq:Hq + Hkv].reshape(M, Hkv * D), yh[:, Hq + Hkv:].reshape(M, Hkv * D)
        g = torch.Generator().manual_seed(pos0 + 7)
        k = torch.cat([k_pre.float(), yh[:, Hq:Hq + Hkv].permute(1, 0, 2), _bf(torch.randn(Hkv, stale, D, generator=g))], 1)  # [Hkv][S][D]
        v = torch.cat([v_pre.float(), yh[:, Hq + Hkv:].permute(1, 0, 2), _bf(torch.randn(Hkv, stale, D, generator=g))], 1)
        for j, s in enumerate(spikes):
            if 0 <= s < v.shape[1]:
                v[:, s, j % D] *= 256
        if kv_only:
            return dict(k=k, v=v)
        S = v.shape[1]
        G = Hq // Hkv
        attn = torch.empty(M, Hq, D)
        kp = torch.arange(S)
        for m in range(M):
            p_m = pos0 + m
            vis = kp <= p_m
            if mut == "mask_future_32":
                vis = vis | ((kp == p_m + 1) & ((p_m + 1) % 32 == 0))
            if mut == "mask_future_split":
                vis = vis | ((kp == p_m + 1) & ((p_m + 1) % 512 == 0))
            if mut == "leak_next":        # the last query but one also sees the pass's last key: ONE key of its future
                vis = vis | ((kp == p_m + 1) & (m == M - 2))
            if mut == "mask_diag_32":
                vis = vis & ~((kp == p_m) & (p_m % 32 == 0))
            if mut == "mask_diag_split":
                vis = vis & ~((kp == p_m) & (p_m % 512 == 0))
            for h in range(Hq):
                kvh = h // G
                if mut == "gqa":
                    kvh = (kvh + 1) % Hkv if h % G == G - 1 else kvh
                sc = (k[kvh] @ q[m, h * D:(h + 1) * D]) * (1.0 / math.sqrt(D))
                sc = torch.where(vis, sc, torch.full_like(sc, -math.inf))
                p = torch.exp(sc - sc.max())
                attn[m, h] = (_bf(p) @ v[kvh]) / p.sum()
        attn = _bf(attn.reshape(M, Hq * D))
        y = self._product(attn, "wo", mut)
        if lw.bo is not None:
            y = y + lw.bo.float()
        x1 = _bf(x0 + y)
        xn = self._norm(x1, lw.mlp_norm_w, lw.mlp_norm_b)
        y = self._product(xn, "w_up", mut)
        if c.arch == W.ARCH_LLAMA:
            g, u = y[:, :ff], y[:, ff:]
            if mut == "swiglu_swap":
                g, u = u, g
            act = _bf(g / (1 + torch.exp(-g)) * u)
        else:
            y = y + lw.b_up.float()
            act = _bf(0.5 * y * (1 + torch.tanh(0.7978845608028654 * (y + 0.044715 * y * y * y))))
        y = self._product(act, "w_down", mut, drop=(64, 128) if mut == "drop_k64" else None)
        if lw.b_down is not None:
            y = y + lw.b_down.float()
        x2 = _bf(x1 + y)
        logits = _bf(self._product(self._norm(x2, self.w.final_norm_w, self.w.final_norm_b), "head", mut))
        return dict(x0=x0, q=q, kn=kn, vn=vn, k=k, v=v, attn=attn, act=act, x2=x2, logits=logits, pos=pos)


def stage_checks(emu, tokens, out):
    """every stage of tests/stage_ref.py against the taps of one run; -> {stage: worst error / bound}"""
    c, lw, w = emu.cfg, emu.w.layers[0], emu.w
    Hq, Hkv, D = c.n_heads, c.n_kv_heads, c.head_dim
    pos = out["pos"]
    M = pos.shape[0]
    res = {}
    x0, x0d = R.embed(c, w, tokens, pos)
    ref, bnd = R.qkv_stage(c, lw, emu.ref_matrix("wqkv"), x0, x0d, pos, w.rope_cos, w.rope_sin, R.chain_hip)
    res["q"] = R.check(out["q"], (ref[:, :Hq * D], bnd[:, :Hq * D]), "q")
    res["k"] = R.check(out["kn"], (ref[:, Hq * D:(Hq + Hkv) * D], bnd[:, Hq * D:(Hq + Hkv) * D]), "k")
    res["v"] = R.check(out["vn"], (ref[:, (Hq + Hkv) * D:], bnd[:, (Hq + Hkv) * D:]), "v")
    kk = out["k"].unsqueeze(0).expand(M, -1, -1, -1)
    vv = out["v"].unsqueeze(0).expand(M, -1, -1, -1)
    res["attn"] = R.check(out["attn"], R.attention_stage(out["q"], kk, vv, pos, Hkv, D), "attention")
    _, _, x1, x1d = R.residual_stage(x0, x0d, out["attn"], emu.ref_matrix("wo"), lw.bo, R.chain_hip)
    res["act"] = R.check(out["act"], R.mlp_stage(c, lw, emu.ref_matrix("w_up"), x1, x1d, R.chain_hip), "activation")
    ref, bnd, _, _ = R.residual_stage(x1, x1d, out["act"], emu.ref_matrix("w_down"), lw.b_down, R.chain_hip)
    res["x"] = R.check(out["x2"], (ref, bnd), "residual")
    res["logits"] = R.check(out["logits"], R.head_stage(c, w, emu.ref_matrix("head"), out["x2"], R.chain_hip), "logits")
    return res


def _prefix(cfg, pos0, seed, peaked=False):
    g = torch.Generator().manual_seed(seed)
    k = torch.randn(cfg.n_kv_heads, pos0, cfg.head_dim, generator=g).bfloat16()
    v = torch.randn(cfg.n_kv_heads, pos0, cfg.head_dim, generator=g).bfloat16()
    return (k * 32 if peaked else k), v


def _tokens(cfg, M, seed):
    return torch.randint(4, cfg.vocab, (M,), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("pos0", [0, 1, 31, 32, 33, 509, 512, 513])
@pytest.mark.parametrize("cfg,dtype", [(TOY, "bf16"), (TOY, "fp8"), (TOY32, "bf16"), (TOY128, "bf16"), (TOY128, "fp8"), (GPT2, "bf16")],
                         ids=lambda v: getattr(v, "name", v))
def test_emulation_within_bounds(cfg, dtype, pos0):
    emu = Emu(cfg, dtype, seed=pos0)
    M = 5
    toks = _tokens(cfg, M, pos0)
    k, v = _prefix(cfg, pos0, pos0 + 1, peaked=(pos0 % 2 == 1))
    res = stage_checks(emu, toks, emu.run(toks, pos0, k, v, spikes=(31, 32, 511, 512, pos0 - 1, pos0 + 2), stale=40))
    assert all(r <= 1.0 for r in res.values()), res


# (mutation, config, first new position, V spikes): each at a place the GPU tests also cover (5 new positions, stale keys after them)
MUTATIONS = [
    ("truncate", TOY, 40, ()),
    ("rope_pos", TOY, 40, ()),
    ("mask_future_32", TOY, 27, (32,)),             # queries 27..31: query 31 also sees key 32 (a stale key of the next block)
    ("mask_diag_32", TOY, 30, (32,)),               # query 32 misses its own key
    ("mask_future_split", TOY, 507, (512,)),        # query 511 also sees key 512 (the first key past a split edge)
    ("mask_diag_split", TOY, 510, (512,)),
    ("fp8_scale", TOY, 8, ()),
    ("drop_k64", TOY, 8, ()),
    ("swiglu_swap", TOY, 8, ()),
    ("gqa", TOY, 40, ()),
]


@pytest.mark.parametrize("mut,cfg,pos0,spikes", MUTATIONS, ids=[m[0] for m in MUTATIONS])
def test_mutation_is_caught(mut, cfg, pos0, spikes):
    emu = Emu(cfg, "fp8" if mut == "fp8_scale" else "bf16", seed=3)
    M = 5
    toks = _tokens(cfg, M, 11)
    k, v = _prefix(cfg, pos0, 5)
    kw = dict(spikes=spikes, stale=40)
    stage_checks(emu, toks, emu.run(toks, pos0, k, v, **kw))       # the unmutated run passes at the same place
    with pytest.raises(AssertionError, match="outside the derived bound"):
        stage_checks(emu, toks, emu.run(toks, pos0, k, v, mut=mut, **kw))


# ---- the future-key construction of tests/test_hip_prefill_rows_fp64_gpu.py ------------------------------------------------------
def test_one_leaked_spike_key_exceeds_the_attention_bound_at_the_largest_position():
    """A prompt chunk's K / V are all appended before its attention runs, so a query at p has up to 384 keys of its own future
    in the cache. An ordinary future key moves it by ~1/p of the V scale: under the attention bound at p ~ 400. The GPU test
    therefore makes every future key a spike key (prefill_cases.spike_weights: V rows ~256 x the others, from the direction
    of one embedding row). Here, at the largest query position it uses (the last ordinary position of its 1024 prompt, one
    before the first spike): the emulation with the causal mask stays inside every bound, and a leak of that ONE spike key into
    that one query exceeds the attention bound."""
    L, s = max(P.FUTURE, key=lambda f: f[1])
    emu = Emu(TOY, weights=P.spike_weights(W.random_init(TOY, seed=7)))
    M = 6
    pos0 = s - (M - 1)                                                    # queries s-5 .. s-1 are ordinary, the last token is the spike
    toks = torch.cat([_tokens(TOY, s, 21), torch.full((1,), P.SPIKE_TOKEN)])
    assert int((toks[:s] == P.SPIKE_TOKEN).sum()) == 0
    empty = torch.empty(TOY.n_kv_heads, 0, TOY.head_dim)
    pre = emu.run(toks[:pos0], 0, empty, empty, kv_only=True)             # the keys below the queries: the model's own, of ordinary size
    out = emu.run(toks[pos0:], pos0, pre["k"], pre["v"])
    v_abs = out["v"].abs().mean((0, 2))
    assert float(v_abs[s]) > 100 * float(v_abs[:s].max())                 # the construction: the spike row's V is two orders up
    res = stage_checks(emu, toks[pos0:], out)
    assert all(r <= 1.0 for r in res.values()), res
    leaked = emu.run(toks[pos0:], pos0, pre["k"], pre["v"], mut="leak_next")
    assert torch.equal(leaked["attn"][:M - 2], out["attn"][:M - 2])        # one query moved, by one key
    with pytest.raises(AssertionError, match=r"attention: .* outside the derived bound; worst at \[4, "):
        stage_checks(emu, toks[pos0:], leaked)
