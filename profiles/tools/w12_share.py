#!/usr/bin/env python3
"""Narrow-block share of the W12 weight format (specdec_hip/w12.py) on the weights the benchmark streams, on the CPU.

    python profiles/tools/w12_share.py            # first layer + lm_head of the synthetic 3B and 1B, and a plain randn matrix

Prints, per matrix class and for both forms of the copy, the share of (tile, 32-k step) blocks whose exponents fit the form's
16-value window (the code form's ends at the largest exponent, the split-byte form's is aligned to an even one) and the size
of the copy relative to the packed bf16 stream. Layers of `synthetic_llama` are drawn alike, so
the first one stands for all of them."""

from __future__ import annotations

import dataclasses
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "llm-inference-lab_amd"))

from specdec_hip import w12, weights as W  # noqa: E402


def bits(t: torch.Tensor) -> np.ndarray:
    return t.contiguous().view(torch.int16).numpy().view(np.uint16)


def report(name: str, w: torch.Tensor, n_pairs: int, epi: int, head_dim: int = 0) -> None:
    N, K = w.shape
    stream = w12.pack_bf16(bits(w), n_pairs, epi, head_dim)
    line = f"{name:28s} N={N:6d} K={K:5d}"
    for tag, form in (("w12", w12.W12_CODES), ("w12s", w12.W12_SPLIT)):   # the code form, then the split-byte form
        _, _, narrow = w12.block_classes(stream, n_pairs, K, form)
        size = w12.w12_bytes(n_pairs, K, int((~narrow).sum()))
        line += f"  {tag}: blocks={narrow.size:7d} narrow={narrow.mean() * 100:6.2f} % /bf16 bytes={size / stream.nbytes:.4f}"
    print(line, flush=True)


def model(cfg: W.ModelConfig, seed: int, **kw) -> W.ModelWeights:
    one = dataclasses.replace(cfg, n_layers=1)    # same generator order: the tables and layer 0 of the full model
    m = W.synthetic_llama(one, seed=seed, **kw)
    l = m.layers[0]
    Nqkv = (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim
    report(f"{cfg.name} qkv", l.wqkv, Nqkv // 2, w12.EPI_QKV_ROPE, cfg.head_dim)
    report(f"{cfg.name} out", l.wo, cfg.d_model // 2, w12.EPI_RESID)
    report(f"{cfg.name} gate/up", l.w_up, cfg.d_ff, w12.EPI_SWIGLU)
    report(f"{cfg.name} down", l.w_down, cfg.d_model // 2, w12.EPI_RESID)
    report(f"{cfg.name} lm_head", m.lm_head, (cfg.vocab + 1) // 2, w12.EPI_ARGMAX)
    return m


def main() -> None:
    tgt = model(W.LLAMA_3_2_3B, seed=0)
    model(W.LLAMA_3_2_1B, seed=1, embed_from=tgt, flip_fraction=0.2)
    g = torch.Generator().manual_seed(0)
    report("randn 4096 x 4096", torch.randn(4096, 4096, generator=g).bfloat16(), 2048, w12.EPI_RESID)


if __name__ == "__main__":
    main()
