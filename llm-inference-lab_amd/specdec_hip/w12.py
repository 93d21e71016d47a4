"""W12: the lossless 12-bit storage of bf16 weights that csrc/pack.hip builds and csrc/gemv.hip streams — a
Python / numpy restatement of the format (the native packer is checked against it, and it decodes native streams).

The packed bf16 stream of a matrix (csrc/pack.hip) is a sequence of BLOCKS: one (tile, 32-k step) unit, 2*np rows x 32
weights (np = pairs of the tile, <= 8), laid out as 8*np chunks of 16 bytes, chunk c = g*2*np + second*np + jp holding
the 8 weights k = 32*step + 8*g + 0..7 of one row. W12 keeps the order of the blocks and of the chunks and stores

  main stream   every block has a slot of 8*np x 12 bytes at 3/4 of its byte offset in the bf16 stream.
                NARROW block (every exponent of its 16*np*16 weights within 16 values, base .. base+15): chunk c's 12
                bytes are its 8 weights as 12-bit codes  sign<<11 | (exp - base)<<7 | mantissa, weight i at bit 12*i.
                WIDE block (anything else: an exact zero or a denormal next to normal weights, an outlier more than 15
                binades under the block's largest, inf / nan): chunk c's 12 bytes are the first 12 of its 16 raw bytes.
  overflow      wide block number k (in stream order) owns 256 bytes at 256*k: chunk c's last 4 raw bytes at 4*c.
  table         one uint32 per (tile, step), index (workgroup * n_tiles_full + tile) * (K/32) + step:
                wide<<31 | base<<23 | k   (k: the wide block's overflow number, 0 for a narrow block).

A block's slot is at an address the kernel computes without the table, so the weight loads do not wait for it; only
the widening (base) and the rare fourth dword of a wide block do. Decode of a code c: ((c & 0x800) << 4) | ((c & 0x7ff) +
(base << 7)) — the bf16 bits again, exactly.

W12S, the split-byte FORM (W12_SPLIT; the *_split / w12s_* functions below), keeps the blocks, slots, overflow and table and
changes what a narrow chunk's 12 bytes hold. A bf16 weight is a high byte h = sign<<7 | exp>>1 and a low byte
l = (exp&1)<<7 | mantissa:

  bytes 0..7    the low bytes of weights 0..7, raw
  bytes 8..11   eight 4-bit codes  sign<<3 | ((exp>>1) - base),  byte 8 + j = code[j] | code[j+4] << 4

with base = max(0, (emax>>1) - 7) in the entry's base field: a block is narrow when its exponents lie in the even-aligned
16-value window 2*base .. 2*base + 15. Decode: h = (code & 8) << 4 | ((code & 7) + base), bits = h << 8 | l."""

from __future__ import annotations

from dataclasses import dataclass
from typing import Iterator, Tuple

import numpy as np

EPI_QKV_ROPE, EPI_RESID, EPI_SWIGLU, EPI_GELU, EPI_ARGMAX = 0, 1, 2, 3, 4
OVF_BLOCK = 256           # bytes of overflow per wide block
MIN_SAVING = 0.15         # a matrix takes W12 when its W12 bytes are at least this much below its bf16 bytes
W12_CODES, W12_SPLIT = 1, 2   # enum W12Form (csrc/kernels.h): what a narrow block's 12 bytes per lane hold


@dataclass(frozen=True)
class Geom:
    grid: int
    ppw: int
    n_tiles: int
    tile_pairs: int
    ksplit: int
    kw: int


def geometry(n_pairs: int, K: int) -> Geom:
    """gemv_geometry of csrc/pack.hip."""
    grid = min(256, n_pairs)
    ppw = (n_pairs + grid - 1) // grid
    grid = (n_pairs + ppw - 1) // ppw
    n_tiles = 1
    while n_tiles * 8 < ppw:
        n_tiles <<= 1
    tile_pairs = (ppw + n_tiles - 1) // n_tiles
    ksplit = 16 // min(n_tiles, 16)
    while ksplit > 1 and (K + ksplit * 32 - 1) // (ksplit * 32) < 2:
        ksplit >>= 1
    kw = ((K + ksplit * 32 - 1) // (ksplit * 32)) * 32
    return Geom(grid, ppw, n_tiles, tile_pairs, ksplit, kw)


def n_tiles_full(q: Geom) -> int:
    return (q.ppw + q.tile_pairs - 1) // q.tile_pairs


def pair_rows(epi: int, p: np.ndarray, n_pairs: int, head_dim: int) -> Tuple[np.ndarray, np.ndarray]:
    if epi == EPI_QKV_ROPE:
        half = head_dim >> 1
        h, i = p // half, p % half
        r0 = h * head_dim + i
        return r0, r0 + half
    if epi == EPI_SWIGLU:
        return p, p + n_pairs
    return 2 * p, 2 * p + 1


def tiles(n_pairs: int, K: int) -> Iterator[Tuple[int, int, int, int]]:
    """(workgroup, tile, first pair, pairs) of every tile, in stream order."""
    q = geometry(n_pairs, K)
    for c in range(q.grid):
        p_lo, p_hi = c * q.ppw, min((c + 1) * q.ppw, n_pairs)
        t = 0
        while p_lo + t * q.tile_pairs < p_hi:
            p0 = p_lo + t * q.tile_pairs
            yield c, t, p0, min(q.tile_pairs, p_hi - p0)
            t += 1


def pack_bf16(w_bits: np.ndarray, n_pairs: int, epi: int, head_dim: int = 0) -> np.ndarray:
    """The packed bf16 stream (pack_kernel) of a [N][K] matrix of bf16 bit patterns: uint16 [n_pairs * 2 * K32]."""
    N, K = w_bits.shape
    assert K % 8 == 0
    K32 = (K + 31) & ~31
    rows = np.zeros((N + 1, K32), dtype=np.uint16)    # row N: the zero row of a missing second row
    rows[:N, :K] = w_bits
    out = np.empty(n_pairs * 2 * K32, dtype=np.uint16)
    for _, _, p0, npairs in tiles(n_pairs, K):
        p = np.arange(p0, p0 + npairs)
        r0, r1 = pair_rows(epi, p, n_pairs, head_dim)
        r = np.concatenate([r0, r1])
        r = np.where(r < N, r, N)
        blk = rows[r].reshape(2 * npairs, K32 // 32, 4, 8)               # [row][step][g][8]
        out[p0 * 2 * K32:(p0 + npairs) * 2 * K32] = blk.transpose(1, 2, 0, 3).reshape(-1)   # [step][g][row][8]
    return out


@dataclass
class W12Matrix:
    main: np.ndarray     # uint8
    ovf: np.ndarray      # uint8 [n_wide * 256]
    table: np.ndarray    # uint32
    n_blocks: int
    n_wide: int

    @property
    def nbytes(self) -> int:
        return self.main.nbytes + self.ovf.nbytes + self.table.nbytes


def table_entries(n_pairs: int, K: int) -> int:
    q = geometry(n_pairs, K)
    return q.grid * n_tiles_full(q) * (((K + 31) & ~31) // 32)


def _block_view(stream: np.ndarray, p0: int, npairs: int, K32: int) -> np.ndarray:
    return stream[p0 * 2 * K32:(p0 + npairs) * 2 * K32].reshape(K32 // 32, 8 * npairs, 8)   # [step][chunk][8]


def block_base(emax: np.ndarray, form: int = W12_CODES) -> np.ndarray:
    """A block's base from its largest exponent: the code form's window ends at emax, the split form's at emax | 1."""
    emax = np.asarray(emax, dtype=np.int64)
    return np.maximum((emax >> 1) - 7, 0) if form == W12_SPLIT else np.maximum(emax - 15, 0)


def block_classes(stream: np.ndarray, n_pairs: int, K: int, form: int = W12_CODES):
    """Per (tile, step): (table index, base, narrow) arrays over all blocks in stream order."""
    K32 = (K + 31) & ~31
    q = geometry(n_pairs, K)
    ntf, nst = n_tiles_full(q), K32 // 32
    idx, base, narrow = [], [], []
    for c, t, p0, npairs in tiles(n_pairs, K):
        e = (_block_view(stream, p0, npairs, K32) >> 7) & 0xFF
        emax = e.max(axis=(1, 2)).astype(np.int64)
        emin = e.min(axis=(1, 2)).astype(np.int64)
        b = block_base(emax, form)
        idx.append((c * ntf + t) * nst + np.arange(nst))
        base.append(b)
        narrow.append((emin >> 1) >= b if form == W12_SPLIT else emin >= b)
    return np.concatenate(idx), np.concatenate(base), np.concatenate(narrow)


def narrow_share(stream: np.ndarray, n_pairs: int, K: int, form: int = W12_CODES) -> float:
    return float(block_classes(stream, n_pairs, K, form)[2].mean())


def w12_bytes(n_pairs: int, K: int, n_wide: int) -> int:
    """Bytes of the W12 copy of a matrix with n_wide wide blocks: main stream, overflow and table, each padded to 256."""
    K32 = (K + 31) & ~31
    pad = lambda v: (v + 255) & ~255   # noqa: E731
    return pad(n_pairs * 2 * K32 * 2 * 3 // 4) + pad(n_wide * OVF_BLOCK) + pad(table_entries(n_pairs, K) * 4)


def encode_codes(bits: np.ndarray, base) -> np.ndarray:
    """12 bytes per 8 weights: bits uint16 [..., 8] -> uint8 [..., 12]."""
    b = bits.astype(np.uint64)
    c = ((b >> 15) << 11) | (((((b >> 7) & 0xFF) - np.asarray(base, dtype=np.uint64)) & 0xF) << 7) | (b & 0x7F)
    lo = c[..., 0] | (c[..., 1] << 12) | (c[..., 2] << 24) | (c[..., 3] << 36)
    hi = c[..., 4] | (c[..., 5] << 12) | (c[..., 6] << 24) | (c[..., 7] << 36)
    lo8 = np.ascontiguousarray(lo).astype("<u8").view(np.uint8).reshape(*lo.shape, 8)[..., :6]
    hi8 = np.ascontiguousarray(hi).astype("<u8").view(np.uint8).reshape(*hi.shape, 8)[..., :6]
    return np.concatenate([lo8, hi8], axis=-1)


def decode_codes(b12: np.ndarray, base) -> np.ndarray:
    """uint8 [..., 12] -> bf16 bits uint16 [..., 8]: ((c & 0x800) << 4) | ((c & 0x7ff) + (base << 7))."""
    z = np.zeros((*b12.shape[:-1], 2), dtype=np.uint8)
    lo = np.ascontiguousarray(np.concatenate([b12[..., :6], z], axis=-1)).view("<u8")[..., 0]
    hi = np.ascontiguousarray(np.concatenate([b12[..., 6:], z], axis=-1)).view("<u8")[..., 0]
    c = np.stack([(v >> s) & 0xFFF for v in (lo, hi) for s in (0, 12, 24, 36)], axis=-1)
    base = np.asarray(base, dtype=np.uint64)
    return (((c & 0x800) << 4) | ((c & 0x7FF) + (base << 7))).astype(np.uint16)


def encode_split(bits: np.ndarray, base) -> np.ndarray:
    """W12S, 12 bytes per 8 weights: bits uint16 [..., 8] -> uint8 [..., 12] (high-byte offsets taken mod 8)."""
    b = bits.astype(np.int64)
    code = ((b >> 15) << 3) | ((((b >> 8) & 0x7F) - np.asarray(base, dtype=np.int64)) & 7)
    return np.concatenate([b & 0xFF, code[..., :4] | (code[..., 4:] << 4)], axis=-1).astype(np.uint8)


def decode_split(b12: np.ndarray, base) -> np.ndarray:
    """uint8 [..., 12] -> bf16 bits uint16 [..., 8]: h = (code & 8) << 4 | ((code & 7) + base), bits = h << 8 | l."""
    n = b12[..., 8:].astype(np.int64)
    code = np.concatenate([n & 0xF, n >> 4], axis=-1)
    h = ((code & 8) << 4) | (((code & 7) + np.asarray(base, dtype=np.int64)) & 0x7F)
    return ((h << 8) | b12[..., :8].astype(np.int64)).astype(np.uint16)


def w12_pack(stream: np.ndarray, n_pairs: int, K: int, form: int = W12_CODES) -> W12Matrix:
    """W12 copy of a packed bf16 stream. A block is narrow only if its codes decode to its bits."""
    enc, dec = (encode_split, decode_split) if form == W12_SPLIT else (encode_codes, decode_codes)
    K32 = (K + 31) & ~31
    q = geometry(n_pairs, K)
    ntf, nst = n_tiles_full(q), K32 // 32
    main = np.zeros(n_pairs * 2 * K32 * 2 * 3 // 4, dtype=np.uint8)
    table = np.zeros(q.grid * ntf * nst, dtype=np.uint32)
    ovf = []
    n_wide = n_blocks = 0
    for c, t, p0, npairs in tiles(n_pairs, K):
        blk = _block_view(stream, p0, npairs, K32)                      # [step][chunk][8]
        e = (blk >> 7) & 0xFF
        base = block_base(e.max(axis=(1, 2)), form)
        codes = enc(blk, base[:, None, None])   # (exponent offsets taken mod 16 / mod 8: a block that does not fit decodes to other bits)
        narrow = (dec(codes, base[:, None, None]) == blk).all(axis=(1, 2))
        raw = np.ascontiguousarray(blk).view(np.uint8).reshape(nst, 8 * npairs, 16)
        slot = np.where(narrow[:, None, None], codes, raw[..., :12])
        o = p0 * 2 * K32 * 2 * 3 // 4
        main[o:o + slot.size] = slot.reshape(-1)
        k = n_wide + np.cumsum(~narrow) - 1
        for s in np.nonzero(~narrow)[0]:
            ob = np.zeros(OVF_BLOCK, dtype=np.uint8)
            ob[:4 * 8 * npairs] = raw[s, :, 12:].reshape(-1)
            ovf.append(ob)
        ent = np.where(narrow, base.astype(np.uint32) << 23, (np.uint32(1) << 31) | k.astype(np.uint32))
        table[(c * ntf + t) * nst:(c * ntf + t + 1) * nst] = ent
        n_wide += int((~narrow).sum())
        n_blocks += nst
    ovf_arr = np.concatenate(ovf) if ovf else np.zeros(0, dtype=np.uint8)
    return W12Matrix(main, ovf_arr, table, n_blocks, n_wide)


def w12_unpack(m: W12Matrix, n_pairs: int, K: int, form: int = W12_CODES) -> np.ndarray:
    """The packed bf16 stream a W12 copy decodes to."""
    dec = decode_split if form == W12_SPLIT else decode_codes
    K32 = (K + 31) & ~31
    q = geometry(n_pairs, K)
    ntf, nst = n_tiles_full(q), K32 // 32
    out = np.empty(n_pairs * 2 * K32, dtype=np.uint16)
    for c, t, p0, npairs in tiles(n_pairs, K):
        ent = m.table[(c * ntf + t) * nst:(c * ntf + t + 1) * nst]
        wide = (ent >> 31).astype(bool)
        base = ((ent >> 23) & 0xFF).astype(np.uint64)
        o = p0 * 2 * K32 * 2 * 3 // 4
        slot = m.main[o:o + nst * 8 * npairs * 12].reshape(nst, 8 * npairs, 12)
        blk = dec(slot, base[:, None, None])
        for s in np.nonzero(wide)[0]:
            k = int(ent[s] & 0x7FFFFF)
            raw = np.empty((8 * npairs, 16), dtype=np.uint8)
            raw[:, :12] = slot[s]
            raw[:, 12:] = m.ovf[k * OVF_BLOCK:k * OVF_BLOCK + 4 * 8 * npairs].reshape(8 * npairs, 4)
            blk[s] = raw.view("<u2").reshape(8 * npairs, 8)
        out[p0 * 2 * K32:(p0 + npairs) * 2 * K32] = blk.reshape(-1)
    return out


def w12s_pack(stream: np.ndarray, n_pairs: int, K: int) -> W12Matrix:
    """W12S copy of a packed bf16 stream: w12_pack in the split-byte form."""
    return w12_pack(stream, n_pairs, K, W12_SPLIT)


def w12s_unpack(m: W12Matrix, n_pairs: int, K: int) -> np.ndarray:
    return w12_unpack(m, n_pairs, K, W12_SPLIT)
