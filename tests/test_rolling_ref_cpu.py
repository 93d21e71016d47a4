"""The rolling context window on the CPU: the restatement tests/rolling_ref.py against a from-scratch fp64 RoPE, and the roll
decision (src/specdec/core/rolling.py: plan / Window.roll) driven through a model of DecodeSession's launch protocol."""

import math
import random

import pytest
import torch

import rolling_ref as RR
from oracle.model_ref import OracleLM
from specdec_hip import weights as W
from src.specdec.core import rolling

F64 = torch.float64


def test_a_rolled_key_is_the_key_of_the_same_token_at_its_new_position():
    """One layer: the K row of a position is a function of the token there and the position alone. Keys computed at positions
    0..L-1 with the model's fp32 tables, stored as bf16, rolled by the restatement (keep 4, drop 24), against the unrotated key times
    a from-scratch fp64 rotation at the NEW position. Bound per element, with n the norm of its (i, i + D/2) pair (a rotation keeps
    it): 2^-8 sqrt(2) n (the rounding of the stored pair — half an ulp of bf16's 8 significant bits is at most 2^-8 of the value —
    carried through the rotation: |a| + |b| <= sqrt(2) n) + 2^-8 |want| (the rounding of the result) + 2^-16 n (fp32 arithmetic and the fp32 tables' angles, < 100 rad here, against fp64)."""
    D, L, keep, drop = 64, 72, 4, 24
    cfg = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=1, d_model=4 * D, n_heads=4, n_kv_heads=2, head_dim=D, d_ff=256, vocab=512, max_pos=128,
                        rope_theta=500000.0, rope_scaling=None, tie_embeddings=False, name="roll-ref")
    mw = W.random_init(cfg, seed=2, std=0.1)
    lm = OracleLM(mw, "fp32")
    toks = torch.randint(4, cfg.vocab, (1, L), generator=torch.Generator().manual_seed(3))
    _, past = lm.forward(toks, need_logits=False)
    stored = [(k.to(torch.bfloat16).float(), v) for k, v in past]
    (k_new, v_new), = RR.roll_past(stored, keep, drop, mw.rope_cos[drop], mw.rope_sin[drop])
    assert k_new.shape[2] == L - drop and torch.equal(v_new[:, :, keep:], past[0][1][:, :, keep + drop:])
    assert torch.equal(k_new[:, :, :keep], stored[0][0][:, :, :keep])                 # the sinks keep their bits
    # the unrotated keys in fp64, from the weights
    x = mw.tok_emb.to(F64)[toks[0]]
    xn = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + cfg.norm_eps) * mw.layers[0].attn_norm_w.to(F64)
    qkv = xn @ mw.layers[0].wqkv.to(F64).t()
    Hq, Hkv = cfg.n_heads, cfg.n_kv_heads
    k_pre = qkv[:, Hq * D:(Hq + Hkv) * D].view(L, Hkv, D).permute(1, 0, 2)             # [Hkv][L][D]
    moved = k_pre[:, keep + drop:]
    cos, sin = RR.rope_fp64(cfg, torch.arange(keep, L - drop))                         # their NEW positions
    a, b = moved[..., : D // 2], moved[..., D // 2:]
    want = torch.cat([a * cos - b * sin, b * cos + a * sin], -1)
    n = (want[..., : D // 2].pow(2) + want[..., D // 2:].pow(2)).sqrt().repeat(1, 1, 2)
    bound = 2.0 ** -8 * math.sqrt(2) * n + 2.0 ** -8 * want.abs() + 2.0 ** -16 * n
    err = (k_new[0, :, keep:].to(F64) - want).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert float((err / bound).max()) > 0.05                                           # (and the bound is not slack by orders)
    # moved but not rotated is far outside (at the pairs that turn fast; the slowest ones barely move in 24 positions)
    lazy = (stored[0][0][0, :, keep + drop:].to(F64) - want).abs()
    assert float((lazy / bound).max()) > 10 and float((lazy > bound).double().mean()) > 0.25


def test_kernel_bound_holds_for_the_restated_arithmetic():
    """the bound of RR.rotate_back against fp32 arithmetic rounded once to bf16, on random pairs and angles"""
    g = torch.Generator().manual_seed(0)
    n = 200_000
    k = torch.randn(n, 2, generator=g).bfloat16()
    ang = torch.rand(n, generator=g) * 4000
    c, s = ang.cos().unsqueeze(1), ang.sin().unsqueeze(1)
    a, b = k[:, :1].float(), k[:, 1:].float()
    got = torch.cat([a * c + b * s, b * c - a * s], -1).bfloat16().to(F64)
    want = torch.cat([a.to(F64) * c.to(F64) + b.to(F64) * s.to(F64), b.to(F64) * c.to(F64) - a.to(F64) * s.to(F64)], -1)
    mag = torch.cat([(a * c).abs() + (b * s).abs(), (b * c).abs() + (a * s).abs()], -1).to(F64)
    assert bool(((got - want).abs() <= 2.0 ** -8 * want.abs() + 3 * 2.0 ** -24 * mag).all())
    # and rotate_back states the same thing for a [.., D] row
    w2, b2 = RR.rotate_back(k[:1], c[0], s[0])
    assert torch.allclose(w2, want[:1]) and float(b2.min()) > 0


@pytest.mark.parametrize("size,sinks,k", [(96, 4, 4), (128, 4, 8), (4096, 4, 4), (100, 0, 1), (61, 4, 2), (512, 16, 4)])
def test_plan_drops_whole_units_and_leaves_room(size, sinks, k):
    w = rolling.plan(size, sinks, k)
    assert w.drop % 8 == 0 and w.drop >= 8 and w.drop <= max(8, (size - sinks) // 2) and w.drop + 8 > (size - sinks) // 2
    assert w.room == 3 * (k + 1) + 2 and w.l_max == size + w.room
    # a roll happens at a cache length c in (W - room, W]: sinks and block lie inside what the cache holds, and room is left
    for c in range(size - w.room + 1, size + 1):
        assert w.roll(c) == w.drop and sinks + w.drop <= c - 1 and w.roll(c - w.drop) is None
    assert w.roll(size - w.room) is None and w.fits(size - w.room) and not w.fits(size - w.room + 1)


@pytest.mark.parametrize("size,sinks,k,msg", [(40, 4, 4, "too small"), (16, 4, 1, "too small"), (64, 40, 2, "too small"), (0, 4, 4, "positive"),
                                              (96, -1, 4, "attention_sinks"), (8192, 4, 4, "max_pos")])
def test_plan_refuses(size, sinks, k, msg):
    with pytest.raises(ValueError, match=msg):
        rolling.plan(size, sinks, k, max_pos=4096)


def test_every_window_plan_always_fits_accepts():
    for k in (1, 2, 4, 8):
        for sinks in (0, 4, 13):
            room = 3 * (k + 1) + 2
            assert rolling.plan(sinks + 2 * room + 16, sinks, k).drop >= room


@pytest.mark.parametrize("depth", [1, 2])
@pytest.mark.parametrize("size,sinks,k", [(96, 4, 4), (61, 4, 2), (160, 8, 8), (75, 0, 4)])
def test_no_launched_step_passes_the_cache(size, sinks, k, depth):
    """DecodeSession's protocol with the window's decision in it: steps are launched `depth` deep while no row is flagged; the
    device advances the row in every launched step (1..K+1 tokens), void or not, and a step addresses positions up to its
    length + K; the host sees a record later, flags "roll" by Window.roll, and from then on the steps in flight are void; the roll
    happens with an empty queue. No position >= l_max is ever addressed, a valid step stays below W, and the cache length the
    host sees never exceeds W."""
    w = rolling.plan(size, sinks, k)
    rng = random.Random(size * 31 + depth)
    for prompt in (2, size - w.room):
        c = d = prompt                    # host's cache length, device's
        queue, flagged, top, top_valid, rolls = [], False, 0, 0, 0
        for _ in range(3000):
            if flagged and not queue:     # the repair point
                drop = w.roll(c)
                assert drop is not None and sinks + drop <= c - 1
                c -= drop
                d, flagged, rolls = c, False, rolls + 1
                assert w.roll(c) is None
            while len(queue) < depth and not flagged:
                n_new = rng.randint(1, k + 1)
                reach = d + k             # the verify pass writes positions d - 1 .. d - 1 + K; allow one more
                queue.append((n_new, False))
                top = max(top, reach)
                top_valid = max(top_valid, reach)
                d += n_new
                if len(queue) == 1 and rng.random() < 0.3:
                    break                 # (the host does not always get ahead)
            n_new, void = queue.pop(0)
            if not void:
                c += n_new
                assert c <= size
                if w.roll(c) is not None:
                    flagged = True
                    queue = [(n, True) for n, _ in queue]
        assert rolls >= 3 and top < w.l_max and top_valid < size, (rolls, top, top_valid)
