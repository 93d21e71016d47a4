"""The launch geometry of the K-token attention kernel (csrc/attention.hip, csrc/attention_device.h) restated in Python, the
cases that walk it, and the cache contents that make a fault of that geometry visible (test infrastructure: no conftest, no
GPU code; tests/test_attention_cases_cpu.py proves the cases on the reference alone, tests/test_hip_attention_geometry_gpu.py
runs them on the device).

The geometry, from the code:
  tiles   = ceil(G * M / 16) query tiles per (row, kv head), G = Hq / Hkv; query (head gh, token m) of a kv head is row
            gh * M + m: tile (gh * M + m) // 16, in-tile row (gh * M + m) % 16
  base    = Hkv * B * tiles workgroups before any split
  n_split = l_max // 512, at most 32, at most 1024 // base (the workspace's partial tiles), at most 512 // base (about one
            wave of workgroups over the chip), at least 1; 1 under SPECDEC_NO_ATTN_SPLIT
  per row: n_keys = pos0 + M, n_blocks = ceil(n_keys / 32), s_eff = min(n_split, max(1, ceil(n_blocks / 16))) workgroups used
  block blk belongs to split (blk // 4) % s_eff and wave blk % 4: a (split, wave) CLASS of blocks is what one wave walks
  the partial of (b, kvh, tile, split) lives in workspace slot ((b * Hkv + kvh) * tiles + tile) * n_split + split

With the present constants the 1024 // base cap never binds below the 512 // base cap (1024 // base >= 512 // base for every
base; tests/test_attention_cases_cpu.py sweeps it): the workspace holds twice what the chip cap admits.

A cache row's contents (`cache_row`): seeded normal K / V, and SENTINELS — single keys whose V holds +- a power of two
>= n_keys / 4 in one channel, so that under a flat softmax one sentinel alone moves its channel by ~1/4 or more while the
attention bound (2^-8 of the weighted |V| mean) stays near 0.01. They sit, for every kv head, in the last block of every
(split, wave) class (for the split launch and for the unsplit one), at key 0, at the last cached key pos0 - 1, in the last
(partial) block, at the first and last slot of a page, and at every position of the last block BEYOND n_keys (never visible to
a correct kernel). Adversaries: "sentinel" (that alone), "peaked" (every K x 32: a concentrated softmax, K addressing; the keys beyond n_keys x 256, so that one of them would win),
"stale" (V x 256 at every position from pos0 to pos0 + M + 64: in-pass causality)."""

from __future__ import annotations

import dataclasses
import math
import zlib
from typing import Optional, Tuple

import torch

ROWS, BLOCK, SPLIT_BLOCKS, MAX_SPLIT, WAVES, SLOTS, CHIP = 16, 32, 16, 32, 4, 1024, 512   # attention_device.h, kernels.h, attention.hip
ARCH_LLAMA, ARCH_GPT2 = 0, 1


@dataclasses.dataclass(frozen=True)
class Model:
    name: str
    d_model: int
    hq: int
    hkv: int
    D: int
    d_ff: int
    vocab: int = 512
    max_pos: int = 4096
    arch: int = ARCH_LLAMA

    @property
    def G(self) -> int:
        return self.hq // self.hkv


EDGE = Model("geo-edge-d64", 256, 4, 2, 64, 512)
G3 = Model("geo-g3-d128", 384, 3, 1, 128, 1024, max_pos=33280)
MHA = Model("geo-mha-gpt2", 256, 4, 4, 64, 1024, max_pos=1024, arch=ARCH_GPT2)
CAP = Model("geo-cap-d32", 512, 16, 8, 32, 1024, max_pos=8192)
C1B = Model("geo-1b-heads", 2048, 32, 8, 64, 1024, max_pos=8192)
MAXS = Model("geo-maxsplit-d32", 128, 4, 2, 32, 256, max_pos=16640)


@dataclasses.dataclass(frozen=True)
class Case:
    id: str
    model: Model
    lens: Tuple[int, ...]            # cached keys (pos0) of every row of the launch
    M: int
    l_max: int
    pages: Tuple[Optional[int], ...] = (None,)     # engines the case runs on: None dense, else the page length
    adversary: str = "sentinel"
    batch: Optional[int] = None      # rows of the bound batch (default: the launch's)
    row0: int = 0
    # the regime the case is listed for (asserted from the plan): tiles, n_split, the binding cap(s), every s_eff of its rows
    tiles: int = 1
    n_split: int = 1
    cap: Tuple[str, ...] = ("lmax",)
    s_eff: Tuple[int, ...] = (1,)

    @property
    def B(self) -> int:
        return len(self.lens)

    @property
    def bound_batch(self) -> int:
        return self.batch if self.batch is not None else self.row0 + self.B


_CAP_LENS = (4200, 4200, 4200, 2500, 1100, 700, 40, 0)

CASES = [
    # G * M = 16 exactly, 18, 34: 1, 2, 3 tiles, a 2-row last tile, a tile edge inside query head 1 (M = 9: row 16 = head 1, m 7)
    Case("tile-edge-M8", EDGE, (1100,), 8, 1536, tiles=1, n_split=3, s_eff=(3,)),
    Case("tile-edge-M9", EDGE, (1100,), 9, 1536, tiles=2, n_split=3, s_eff=(3,)),
    Case("tile-edge-M17", EDGE, (1100,), 17, 1536, tiles=3, n_split=3, s_eff=(3,)),
    Case("g3-d128", G3, (1030,), 6, 1536, tiles=2, n_split=3, s_eff=(3,)),
    Case("mha-gpt2", MHA, (600,), 17, 1024, tiles=2, n_split=2, s_eff=(2,)),
    # every s_eff from 1 to 5 in one launch at row0 > 0. (Lengths 0 .. 2049 give s_eff 1, 2, 3 and 5 only: 2047 + 5 keys are
    # 65 blocks already. The ninth row, 1537 keys = 49 blocks, is the one that uses 4 workgroups.)
    Case("ragged", EDGE, (0, 511, 512, 513, 1023, 1025, 2047, 2049, 1537), 5, 2560, batch=11, row0=2, tiles=1, n_split=5,
         s_eff=(1, 2, 3, 4, 5)),
    # base 128: n_split 4 where l_max / 512 = 9; a workgroup of a 4200-key row walks 132 / 4 = 33 blocks
    Case("cap-512", CAP, _CAP_LENS * 2, 5, 4608, pages=(None, 64), tiles=1, n_split=4, cap=("chip",), s_eff=(1, 2, 3, 4)),
    Case("cap-1b", C1B, _CAP_LENS, 5, 4608, tiles=2, n_split=4, cap=("chip",), s_eff=(1, 2, 3, 4)),
    Case("max-split", MAXS, (16500,), 5, 16512, pages=(None, 32), tiles=1, n_split=32, cap=("lmax", "max"), s_eff=(32,)),
    # 1032 blocks over 32 workgroups: more than 32 blocks each
    Case("past-max", G3, (33000,), 5, 33024, pages=(None, 64), tiles=1, n_split=32, cap=("max",), s_eff=(32,)),
    Case("stale", EDGE, (1030,), 9, 1536, adversary="stale", tiles=2, n_split=3, s_eff=(3,)),
    Case("peaked-tile-edge", EDGE, (1100,), 9, 1536, adversary="peaked", tiles=2, n_split=3, s_eff=(3,)),
    Case("peaked-max-split", MAXS, (16500,), 5, 16512, adversary="peaked", tiles=1, n_split=32, cap=("lmax", "max"), s_eff=(32,)),
]
BY_ID = {c.id: c for c in CASES}

# The passes of the handover test, in turn on ONE 16-row engine of the cap-512 model without a rebind: the merge workspace and
# its arrival counters pass from a 9-way split of one tile per (row, kv head), to a launch that does not split, to three tiles
# of 9 slots each of which 3 are used — and back.
HANDOVER = [
    Case("handover-4200x3", CAP, (4200, 4200, 4200), 5, 4608, batch=16, row0=0, tiles=1, n_split=9, s_eff=(9,)),
    Case("handover-40", CAP, (40,), 1, 4608, batch=16, row0=3, tiles=1, n_split=9, s_eff=(1,)),
    Case("handover-1100x2", CAP, (1100, 1100), 17, 4608, batch=16, row0=4, tiles=3, n_split=9, s_eff=(3,)),
]
# the cached prefix of the prompt test: 300 positions at pos0 1500 (its attention runs as the prefill's sub-passes of <= 128
# positions, l_max 2048: n_split 4, all four used by a row of 1500+ keys; the regime fields are not used)
PROMPT = Case("prompt-after-prefix", EDGE, (1500,), 300, 2048)


# ---- the plan, restated --------------------------------------------------------------------------------------------------------
def plan(hq: int, hkv: int, B: int, M: int, l_max: int, split: bool = True) -> dict:
    """tiles, base, n_split and the cap(s) that hold n_split where it is ("lmax", "max", "slots", "chip"; () unsplit)"""
    tiles = -(-(hq // hkv) * M // ROWS)
    base = hkv * B * tiles
    if not split:
        return dict(tiles=tiles, base=base, n_split=1, cap=())
    caps = {"lmax": l_max // (BLOCK * SPLIT_BLOCKS), "max": MAX_SPLIT, "slots": SLOTS // base, "chip": CHIP // base}
    ns = min(caps.values())
    return dict(tiles=tiles, base=base, n_split=max(ns, 1), cap=tuple(k for k, v in caps.items() if v == ns))


def row_plan(n_split: int, pos0: int, M: int, l_max: int) -> Tuple[int, int, int]:
    """(n_keys, n_blocks, s_eff) of a row whose first query sits at pos0"""
    n_keys = max(0, min(pos0 + M, l_max))
    n_blocks = -(-n_keys // BLOCK)
    s_eff = min(n_split, max(1, -(-n_blocks // SPLIT_BLOCKS))) if n_split > 1 else 1
    return n_keys, n_blocks, s_eff


def block_class(blk: int, s_eff: int) -> Tuple[int, int]:
    """(split, wave) that walks block blk"""
    return (blk // WAVES) % s_eff, blk % WAVES


def key_classes(n: int, s_eff: int) -> torch.Tensor:
    """class index split * 4 + wave of every key position [0, n)"""
    blk = torch.arange(n) // BLOCK
    return ((blk // WAVES) % s_eff) * WAVES + blk % WAVES


def query_row(G: int, M: int, gh: int, m: int) -> Tuple[int, int]:
    """(tile, in-tile row) of query head gh (within its kv head), token m"""
    return divmod(gh * M + m, ROWS)


def slot(b: int, kvh: int, tile: int, split: int, hkv: int, tiles: int, n_split: int) -> int:
    return ((b * hkv + kvh) * tiles + tile) * n_split + split


def case_plan(case: Case, split: bool = True) -> dict:
    p = plan(case.model.hq, case.model.hkv, case.B, case.M, case.l_max, split)
    p["rows"] = [row_plan(p["n_split"], n, case.M, case.l_max) for n in case.lens]
    return p


# ---- cache contents ------------------------------------------------------------------------------------------------------------
def written(case: Case, i: int) -> int:
    """positions [0, written) of row i hold layout values: through the end of the last block (the keys beyond n_keys), and
    the stale positions of the `stale` adversary"""
    n = -(-(case.lens[i] + case.M) // BLOCK) * BLOCK
    if case.adversary == "stale":
        n = max(n, case.lens[i] + case.M + 64)
    return min(n, case.l_max)


def sentinel_positions(case: Case, i: int, kvh: int) -> list:
    """positions below pos0 (cached keys) that hold a sentinel for kv head kvh, in a fixed order"""
    pos0, M = case.lens[i], case.M
    if pos0 <= 0:
        return []
    out = [0, pos0 - 1]
    for split in (True, False):
        n_keys, n_blocks, s_eff = row_plan(case_plan(case, split)["n_split"], pos0, M, case.l_max)
        last = {}
        for blk in range(n_blocks):
            if blk * BLOCK < pos0:
                last[block_class(blk, s_eff)] = blk          # the last block of the class that holds a cached key
        for ci, (cls, blk) in enumerate(sorted(last.items())):
            room = min(BLOCK, pos0 - blk * BLOCK)
            out.append(blk * BLOCK + (7 * ci + 11 * kvh + 3) % room)
    n_blocks = -(-(pos0 + M) // BLOCK)
    if (n_blocks - 1) * BLOCK < pos0:                        # the last, partial block
        out.append((n_blocks - 1) * BLOCK)
    for P in case.pages:
        if P is not None and pos0 >= P:
            pg = (pos0 // P) // 2                            # a full page in the middle of the row
            out += [pg * P, pg * P + P - 1]
    seen, uniq = set(), []
    for p in out:
        if 0 <= p < pos0 and p not in seen:
            seen.add(p)
            uniq.append(p)
    return uniq


def amplitude(n_keys: int) -> float:
    """the power of two >= n_keys / 4 (at least 1)"""
    return float(2 ** max(0, math.ceil(math.log2(max(n_keys, 1) / 4))))


def cache_row(case: Case, i: int):
    """K, V bf16 [Hkv][written][D] (CPU) of row i of the case. Positions [pos0, pos0 + M) are the forward's to overwrite: they
    hold plain normal values here (the new rows of a pass cannot be planted), so the reference-only tests see a cache a pass
    could have left."""
    md, pos0, M = case.model, case.lens[i], case.M
    n = written(case, i)
    gen = torch.Generator().manual_seed(zlib.crc32(case.id.encode()) + i)
    k = torch.randn(md.hkv, n, md.D, generator=gen).bfloat16()
    v = torch.randn(md.hkv, n, md.D, generator=gen).bfloat16()
    A = amplitude(pos0 + M)
    for h in range(md.hkv):
        for j, p in enumerate(sentinel_positions(case, i, h)):
            v[h, p, (j + 3 * h) % md.D] = A if (j + h) % 2 == 0 else -A
        for j, p in enumerate(range(pos0 + M, -(-(pos0 + M) // BLOCK) * BLOCK)):     # beyond n_keys, inside the last block
            if p < n:
                v[h, p, (5 * j + h) % md.D] = -A if (j + h) % 2 == 0 else A
    if case.adversary == "peaked":
        k = k * 32
        k[:, pos0 + M:] *= 8          # a concentrated softmax sees a key beyond n_keys only if it can win: theirs are 8 x longer still
    if case.adversary == "stale":
        v[:, pos0 + M:pos0 + M + 64] *= 256
    return k, v
