"""Shared builders of W12 / W12S test matrices: the format's edge values, and wide blocks PLANTED at chosen places of a GEMV's
work split. numpy only; nothing here touches a device.

Used by the two CPU format tests (tests/test_w12_format_cpu.py, tests/test_w12s_format_cpu.py), checked on its own by
tests/test_w12_cases_cpu.py, and fed to the device packer and the GEMVs by tests/test_hip_w12_edges_gpu.py.

Everything is bf16 BIT PATTERNS (uint16): inf, nan and denormal patterns pass through unharmed.

A matrix [N][K] with n_pairs row pairs is cut by specdec_hip.w12.geometry into workgroups c, tiles t and 32-k steps; a BLOCK is
one (c, t, step). Its table index is (c * n_tiles_full + t) * (K / 32) + step; gt = c * n_tiles_full + t is the GLOBAL TILE.
K is cut into ksplit slices of S = kw / 32 steps: step = slice * S + s, and a wave walks its slice in batches of kb steps, so
s % kb is the block's position j in its batch."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Dict, Tuple

import numpy as np

from specdec_hip import w12

# (N, K, epi, head_dim): the six small geometries of the format tests
SHAPES = {
    "8 pairs per tile": (4096, 64, w12.EPI_RESID, 0),            # 2048 pairs: 256 workgroups x 8
    "5 pairs per tile": (2560, 256, w12.EPI_RESID, 0),           # 1280 pairs: 256 x 5
    "1 pair per tile": (64, 512, w12.EPI_RESID, 0),              # 32 workgroups of one pair, 16 K slices
    "qkv pairs": (512, 64, w12.EPI_QKV_ROPE, 64),                # rows (i, i + 32) of a head
    "swiglu pairs, short last": (2 * 2051, 96, w12.EPI_SWIGLU, 0),   # 2051 pairs = 227 x 9 + 8: two tiles of 5 and 4, a short last workgroup
    "odd N head": (1001, 64, w12.EPI_ARGMAX, 0),                 # 501 pairs, the last second row is zero
}

FORCERS = {
    "zero": 0x0000, "negative zero": 0x8000, "denormal": 0x0001, "2^-30": ((127 - 30) << 7), "+inf": 0x7F80, "-inf": 0xFF80,
    "nan": 0x7FC1,
}


def n_pairs_of(N: int, epi: int) -> int:
    return N // 2 if epi == w12.EPI_SWIGLU else (N + 1) // 2


def bf16(x: np.ndarray) -> np.ndarray:
    """float32 -> bf16 bits, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def one_binade(N, K, seed):
    rng = np.random.default_rng(seed)
    return bf16((1.0 + 0.98 * rng.random((N, K))).astype(np.float32))    # [1, 1.98]: exponent 127 only, after rounding too


def one_binade_both_signs(N, K, seed=1):
    """ALL NARROW in both forms: exponent 127 only, both signs"""
    wb = one_binade(N, K, seed)
    wb[np.random.default_rng(seed + 1).random((N, K)) < 0.5] |= 0x8000
    return wb


def all_wide(N, K, seed=2):
    """ALL WIDE in both forms: N(0, 1) with an exact zero in every 8-weight chunk"""
    wb = bf16(np.random.default_rng(seed).standard_normal((N, K)).astype(np.float32))
    wb[:, ::8] = 0
    return wb


def normal(N, K, seed, std=0.02):
    return bf16(np.random.default_rng(seed).standard_normal((N, K)).astype(np.float32) * std)


def exps(lo, hi):
    """64 bf16 patterns whose exponents are lo..hi (every value present, both signs, varied mantissas)"""
    e = np.resize(np.arange(lo, hi + 1), 64).astype(np.uint16)
    i = np.arange(64, dtype=np.uint16)
    return (((i & 1) << 15) | (e << 7) | ((i * 37) & 0x7F)).astype(np.uint16).reshape(2, 32)


# ---- fills of ONE block: f(b) rewrites b, the block's [rows][32] bits (first rows of its pairs, then second rows) ----------------
def _tiled(pattern: np.ndarray, shape) -> np.ndarray:
    """a [2][32] pattern over a block of more rows: row r takes pattern row r % 2 (every row keeps all 32 values)"""
    return pattern[np.arange(shape[0]) % 2]


def fill_span(emax: int, span: int) -> Callable:
    """exponents emax - span + 1 .. emax, every one present"""
    def fill(b):
        b[:] = _tiled(exps(emax - span + 1, emax), b.shape)
    return fill


# (emax, span, narrow in the split-byte form): odd largest exponent: the window 112..127 ends at it and 16 values fit;
# even: the window 114..129 reaches one past it, 15 values fit below
SPLIT_SPANS = [(127, 16, True), (127, 17, False), (128, 15, True), (128, 16, False), (128, 17, False)]

# all eight high-byte offsets (exponents 112 .. 127) with both signs in one 8-weight lane
OFFSETS_LANE = np.array([(s << 15) | ((112 + 2 * o + (o & 1)) << 7) | (0x55 ^ o) for o, s in zip(range(8), [0, 1, 0, 1, 1, 0, 1, 0])],
                        dtype=np.uint16)


def fill_offsets(b):
    b[:] = (127 << 7) | 0x11
    b[1, 8:16] = OFFSETS_LANE


def fill_base0(b):
    b[:] = _tiled(exps(0, 15), b.shape)              # zeros' and denormals' exponent 0 up to 15: h = 0..7, base 0
    b[0, 0], b[0, 1], b[0, 2] = 0x0000, 0x8000, 0x0001


def fill_below_the_clamp(b):
    b[:] = _tiled(exps(0, 9), b.shape)               # largest exponent 9: emax - 15 and (emax >> 1) - 7 are NEGATIVE, the base is 0


def fill_zeros_and_denormals(b):
    b[:] = _tiled(exps(0, 0), b.shape)               # exponent 0 only (a block of pruned weights): denormals of both signs ...
    b[:, 0::4] &= 0x8000                             # ... and exact zeros, positive (even columns) ...
    b[:, 1::8] &= 0x8000                             # ... and negative


def fill_base0_wide(b):
    b[:] = _tiled(exps(0, 16), b.shape)


def fill_254_255(b):
    b[:] = _tiled(exps(240, 255), b.shape)           # inf and nan patterns among huge values: h = 120..127
    b[0, 0], b[0, 1], b[1, 2] = 0x7F80, 0xFF80, 0x7FC1


BLOCK_FILLS: Dict[str, Callable] = {
    **{f"span {span} under {emax}": fill_span(emax, span) for emax, span, _ in SPLIT_SPANS},
    "eight offsets, both signs": fill_offsets, "base 0": fill_base0, "base 0, 17 exponents": fill_base0_wide,
    "exponents 254 / 255": fill_254_255, "exponents 0 .. 9": fill_below_the_clamp, "zeros and denormals": fill_zeros_and_denormals,
}


# ---- the work split, as arrays ---------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Grid:
    """every tile of a matrix in table (= stream) order, and its K steps. Arrays over tiles are [n][1], over steps [1][K/32]."""
    q: w12.Geom
    ntf: int                 # n_tiles_full: the table's tiles per workgroup
    nst: int                 # K / 32
    S: int                   # steps per K slice
    c: np.ndarray            # workgroup
    t: np.ndarray            # tile of the workgroup
    gt: np.ndarray           # global tile c * ntf + t
    p0: np.ndarray           # first pair
    np_: np.ndarray          # pairs (<= tile_pairs)
    step: np.ndarray         # 0 .. K/32 - 1
    s: np.ndarray            # step within its slice

    @property
    def short_last_tile(self) -> np.ndarray:
        """a workgroup's last tile, where it holds fewer pairs than the others"""
        last = np.ones_like(self.c, dtype=bool)
        last[:-1] = self.c[1:] != self.c[:-1]
        return last & (self.np_ < self.q.tile_pairs)

    @property
    def last_workgroup(self) -> np.ndarray:
        return self.c == self.q.grid - 1


def grid(n_pairs: int, K: int) -> Grid:
    q = w12.geometry(n_pairs, K)
    ntf, nst = w12.n_tiles_full(q), ((K + 31) & ~31) // 32
    c, t = np.divmod(np.arange(q.grid * ntf), ntf)
    p0 = c * q.ppw + t * q.tile_pairs
    p_hi = np.minimum((c + 1) * q.ppw, n_pairs)
    ok = p0 < p_hi
    c, t, p0, p_hi = c[ok], t[ok], p0[ok], p_hi[ok]
    step = np.arange(nst)
    return Grid(q, ntf, nst, q.kw // 32, c[:, None], t[:, None], (c * ntf + t)[:, None], p0[:, None],
                np.minimum(q.tile_pairs, p_hi - p0)[:, None], step[None, :], (step % (q.kw // 32))[None, :])


def tile_rows(N: int, n_pairs: int, epi: int, head_dim: int, p0: int, npairs: int) -> np.ndarray:
    """matrix rows of a tile: first rows of its pairs, then second rows (rows past an odd N left out)"""
    r0, r1 = w12.pair_rows(epi, np.arange(p0, p0 + npairs), n_pairs, head_dim)
    r = np.concatenate([r0, r1])
    return r[r < N]


def block_case(N, K, epi, head_dim, fill, tile=3, step=5, seed=7):
    """A one-binade [1, 2) matrix (every block narrow) whose block (tile-th tile in table order, step) is rewritten by `fill`
    -> (matrix, the block's table index). At the "1 pair per tile" shape the default block is pair 3, step 5."""
    g = grid(n_pairs_of(N, epi), K)
    tile, step = min(tile, g.gt.size - 2), min(step, g.nst - 1)          # (never the last tile: it may hold an odd N's zero row)
    wb = one_binade(N, K, seed)
    rows = tile_rows(N, n_pairs_of(N, epi), epi, head_dim, int(g.p0[tile, 0]), int(g.np_[tile, 0]))
    b = wb[rows, 32 * step:32 * step + 32]
    fill(b)
    wb[rows, 32 * step:32 * step + 32] = b
    return wb, int(g.gt[tile, 0]) * g.nst + step


def forcer_case(N, K, what, seed=3):
    """every block narrow but the one that holds (N // 3, 40), which one value forces wide"""
    wb = one_binade(N, K, seed)
    wb[N // 3, 40] = FORCERS[what]
    return wb


def alternating(N, K, seed=5):
    """an exact zero in every other 32-k step of every row: the blocks alternate wide, narrow along K"""
    wb = one_binade(N, K, seed)
    wb[:, 0::64] = 0
    return wb


def edge_cases() -> Dict[str, Callable]:
    """name -> f(N, K, epi, head_dim) -> bf16 bits [N][K]: every edge of the format, at any shape with K >= 64"""
    out: Dict[str, Callable] = {
        "all narrow": lambda N, K, epi, hd: one_binade_both_signs(N, K),
        "all wide": lambda N, K, epi, hd: all_wide(N, K),
        "alternating": lambda N, K, epi, hd: alternating(N, K),
        "normal": lambda N, K, epi, hd: normal(N, K, N + K),
        "window": lambda N, K, epi, hd: window_background(N, K, epi, hd, 9)[0],
    }
    for name, fill in BLOCK_FILLS.items():
        out[name] = lambda N, K, epi, hd, fill=fill: block_case(N, K, epi, hd, fill)[0]
    for what in FORCERS:
        out[f"forcer {what}"] = lambda N, K, epi, hd, what=what: forcer_case(N, K, what)
    return out


# ---- a background that is narrow in both forms, and wide blocks planted in it ------------------------------------------------------
def narrow_background(N: int, K: int, seed: int) -> np.ndarray:
    """bf16 bits of +-(1 + u) * 2^e, e uniform in -9 .. -4: a block spans at most 7 exponents (118 .. 124), narrow in both forms"""
    rng = np.random.default_rng(seed)
    v = (1.0 + rng.random((N, K), dtype=np.float32)) * np.exp2(rng.integers(-9, -3, (N, K))).astype(np.float32)
    return bf16(v) | (rng.integers(0, 2, (N, K)).astype(np.uint16) << 15)


def plant_coords(n_pairs: int, K: int, epi: int, head_dim: int, predicate: Callable[[Grid], np.ndarray]):
    """-> (rows, columns, table indices) of the planted element of every block the predicate selects, in table order: the
    first row of the block's first pair, column 32 * step + 5"""
    g = grid(n_pairs, K)
    mask = np.broadcast_to(predicate(g), (g.gt.size, g.nst))
    ti, st = np.nonzero(mask)
    rows = w12.pair_rows(epi, g.p0[ti, 0], n_pairs, head_dim)[0]
    return rows, 32 * st + 5, g.gt[ti, 0] * g.nst + st


def plant(wb: np.ndarray, n_pairs: int, K: int, epi: int, head_dim: int, predicate) -> np.ndarray:
    """set one element to exact 0 in every block the predicate selects (in place) -> the planted blocks' table indices"""
    rows, cols, idx = plant_coords(n_pairs, K, epi, head_dim, predicate)
    wb[rows, cols] = 0
    return idx


def last_batch(g: Grid, kb: int) -> int:
    """first step of a slice's last batch"""
    return (g.S - 1) // kb * kb


def pattern(name: str, m: int = 1) -> Callable[[Grid], np.ndarray]:
    """the predicates on (global tile gt, step s of the slice, S steps per slice); m: every m-th global tile only"""
    kind, _, arg = name.partition(":")
    kb = int(arg) if arg else 0

    def pred(g: Grid) -> np.ndarray:
        thin = g.gt % m == 0
        if kind == "none":
            return np.zeros((g.gt.size, g.nst), dtype=bool)
        if kind == "stairs":          # one wide block per batch, at position gt % kb: every position j, in every slice
            return thin & (g.s % kb == (g.gt // m) % kb)
        if kind == "runs":            # every step of the first and of the last batch of every slice
            return thin & ((g.s < kb) | (g.s >= last_batch(g, kb)))
        if kind == "edges":           # the first and the last (clamped) step of every slice
            return thin & ((g.s == 0) | (g.s == g.S - 1))
        if kind == "tail":            # every step of short last tiles and of the last workgroup's tiles
            return (g.short_last_tile | g.last_workgroup) & thin & (g.s >= 0)
        raise KeyError(name)
    return pred


PATTERNS = ("none", "stairs:6", "stairs:12", "runs:12", "edges", "tail")
UNTHINNED = ("none", "stairs:6", "stairs:12")       # m = 1 wherever a tile has at least 4 pairs


def taken(n_pairs: int, K: int, n_wide: int) -> bool:
    """the size rule (w12_taken, csrc/pack.hip): the copy is at least 15 % smaller than the padded bf16 stream"""
    K32 = (K + 31) & ~31
    return w12.w12_bytes(n_pairs, K, n_wide) <= (1 - w12.MIN_SAVING) * ((n_pairs * 2 * K32 * 2 + 255) & ~255)


def n_planted(n_pairs: int, K: int, name: str, m: int) -> int:
    g = grid(n_pairs, K)
    return int(np.broadcast_to(pattern(name, m)(g), (g.gt.size, g.nst)).sum())


def thinning(n_pairs: int, K: int, name: str) -> int:
    """the smallest m for which the matrix with the pattern planted keeps its W12 copy"""
    for m in range(1, 4097):
        if taken(n_pairs, K, n_planted(n_pairs, K, name, m)):
            return m
    raise ValueError((n_pairs, K, name))


# ---- window edges that can go through a forward ------------------------------------------------------------------------------------
def window_tops(n_blocks: int, seed: int) -> np.ndarray:
    """per block (table order): its largest exponent, 127 - 20 .. 127 - 4; every 16th block: 15 (exponents 0 .. 15, base 0)"""
    top = np.random.default_rng(seed).integers(127 - 20, 127 - 3, n_blocks)
    top[::16] = 15
    return top


def window_background(N: int, K: int, epi: int, head_dim: int, seed: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Every block spans its whole split-byte window: 16 exponents ending at an odd largest one, 15 at an even one, both signs;
    in every 16th block the exponents are 0 .. 15 with zeros and denormals (base 0). Products stay finite: no exponent is
    above 127 - 4. -> (bits [N][K], table index of every block, its largest exponent). Narrow in both forms by construction
    (the code form's window is the 16 values ending at the largest); w12.block_classes gives the expected classes."""
    n_pairs = n_pairs_of(N, epi)
    g = grid(n_pairs, K)
    idx = (g.gt * g.nst + g.step).reshape(-1)
    top_of = np.zeros(g.q.grid * g.ntf * g.nst, dtype=np.int32)
    top_of[idx] = window_tops(idx.size, seed)
    # the global tile of every matrix row
    row_gt = np.zeros(N + 1, dtype=np.int32)
    jp = np.arange(g.q.tile_pairs)[None, :]
    pairs = (g.p0 + jp)[jp < g.np_]
    gts = np.broadcast_to(g.gt, (g.gt.size, g.q.tile_pairs))[jp < g.np_]
    r0, r1 = w12.pair_rows(epi, pairs, n_pairs, head_dim)
    row_gt[np.minimum(r0, N)] = gts
    row_gt[np.minimum(r1, N)] = gts
    r, c = np.arange(N, dtype=np.int32)[:, None], np.arange(K, dtype=np.int32)[None, :]
    top = top_of[row_gt[:N, None] * g.nst + (c >> 5)]
    span = np.where(top & 1, 16, 15).astype(np.int32)
    e = top - (c + r) % span                        # 32 consecutive columns of a row: every exponent of the window
    rng = np.random.default_rng(seed + 1)
    mant = rng.integers(0, 128, (N, K), dtype=np.int32)
    sign = rng.integers(0, 2, (N, K), dtype=np.int32)
    mant[(e == 0) & ((c >> 4) & 1 == 1)] = 0        # exponent 0 (base-0 blocks): exact zeros of both signs, and denormals
    wb = ((sign << 15) | (e << 7) | mant).astype(np.uint16)
    return wb, idx, top_of[idx]


# ---- the GEMV cases of tests/test_hip_w12_edges_gpu.py, as numbers (tests/test_w12_cases_cpu.py checks them without a GPU) ---------
# one-layer models: the 1B / 3B / 8B layer dimensions over a 1024-token vocabulary (ksplit 16 / 8 / 4 / 2; 4 / 12 / 16 / 24 / 64
# steps per slice), and three heads whose work split is the production lm_head's at small K (ksplit 1):
#   128256 x 256: 251 pairs per workgroup, 32 tiles of 8 (the last of 3), two rounds over the 16 waves, 8 steps per slice
#   66000 x 1024: 129 pairs, 26 tiles of 5 (the last of 4) where the round-up to a power of two says 32; 32 steps
#   33000 x 512:  65 pairs, 13 tiles of 5 where the round-up says 16, one round; 16 steps; a last workgroup of 11 tiles
GPU_MODELS = {
    "1b": dict(d_model=2048, n_heads=32, n_kv_heads=8, head_dim=64, d_ff=8192, vocab=1024),
    "3b": dict(d_model=3072, n_heads=24, n_kv_heads=8, head_dim=128, d_ff=8192, vocab=1024),
    "8b": dict(d_model=4096, n_heads=32, n_kv_heads=8, head_dim=128, d_ff=14336, vocab=1024),
    "head-128256x256": dict(d_model=256, n_heads=4, n_kv_heads=2, head_dim=64, d_ff=512, vocab=128256),
    "head-66000x1024": dict(d_model=1024, n_heads=8, n_kv_heads=2, head_dim=128, d_ff=1024, vocab=66000),
    "head-33000x512": dict(d_model=512, n_heads=8, n_kv_heads=2, head_dim=64, d_ff=1024, vocab=33000),
}
# the matrices (0 qkv, 1 out, 2 gate / up, 3 down, 4 lm_head) a pattern is planted in and that must stream their copy. The 8B
# down-projection (K = 14336) is a MASK shape that W12 does not cover; the small layer of a head model is background only.
UNDER_TEST = {"1b": (0, 1, 2, 3, 4), "3b": (0, 1, 2, 3, 4), "8b": (0, 1, 2, 4),
              "head-128256x256": (4,), "head-66000x1024": (4,), "head-33000x512": (4,)}
WINDOW_MODELS = ("1b", "head-128256x256")
GPU_CASES = [(m, p) for m in GPU_MODELS for p in PATTERNS] + [(m, "window") for m in WINDOW_MODELS]
TOKENS = (1, 2, 3, 5, 9)


def model_matrices(d_model, n_heads, n_kv_heads, head_dim, d_ff, vocab):
    """(N, K, epi, head_dim of the pair map) of a Llama layer's four matrices and the lm_head"""
    return [((n_heads + 2 * n_kv_heads) * head_dim, d_model, w12.EPI_QKV_ROPE, head_dim), (d_model, n_heads * head_dim, w12.EPI_RESID, 0),
            (2 * d_ff, d_model, w12.EPI_SWIGLU, 0), (d_model, d_ff, w12.EPI_RESID, 0), (vocab, d_model, w12.EPI_ARGMAX, 0)]


def covered(n_pairs: int, K: int) -> bool:
    """gemv_w12_covers (csrc/gemv.hip): whole 32-k steps in equal slices, rows that one workgroup's threads stage in registers"""
    q = w12.geometry(n_pairs, K)
    return K >= 32 and q.kw * q.ksplit == K and K // 8 <= 1024
