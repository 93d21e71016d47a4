"""The W12 weight format (csrc/pack.hip) as restated in specdec_hip/w12.py: pack, then unpack, equals the input bit for bit.

No tolerance appears here: the format is lossless or it is wrong. Shapes are small and chosen for the geometry: 8 pairs per
tile, fewer than 8 (5, 1), an odd N (a zero second row in the last pair), one and several K slices."""

import numpy as np
import pytest
import torch

import w12_cases as C
from specdec_hip import w12
from w12_cases import FORCERS, SHAPES


def _bits(t: torch.Tensor) -> np.ndarray:
    return t.bfloat16().contiguous().view(torch.int16).numpy().view(np.uint16).copy()


def _n_pairs(N, epi):
    return (N + 1) // 2


def _roundtrip(wb, epi, head_dim):
    N, K = wb.shape
    n_pairs = _n_pairs(N, epi)
    stream = w12.pack_bf16(wb, n_pairs, epi, head_dim)
    m = w12.w12_pack(stream, n_pairs, K)
    back = w12.w12_unpack(m, n_pairs, K)
    assert back.dtype == stream.dtype and np.array_equal(back, stream)
    assert m.main.nbytes * 4 == stream.nbytes * 3 and m.ovf.nbytes == m.n_wide * w12.OVF_BLOCK
    return stream, m


@pytest.mark.parametrize("name", list(SHAPES))
def test_random_matrices_round_trip(name):
    N, K, epi, hd = SHAPES[name]
    g = torch.Generator().manual_seed(N + K)
    wb = _bits(torch.randn(N, K, generator=g) * 0.02)
    stream, m = _roundtrip(wb, epi, hd)
    assert 0 < m.n_wide < m.n_blocks or name == "odd N head"     # N(0, s) weights: mostly narrow, some wide
    assert m.n_wide < 0.2 * m.n_blocks


def test_packed_stream_holds_every_weight_once():
    N, K, epi, hd = SHAPES["qkv pairs"]
    wb = np.arange(N * K, dtype=np.uint32).reshape(N, K).astype(np.uint16)   # distinct while N * K <= 65536
    assert N * K <= 65536
    stream = w12.pack_bf16(wb, N // 2, epi, hd)
    assert np.array_equal(np.sort(stream), np.arange(N * K, dtype=np.uint16))


def test_all_narrow_matrix():
    N, K, epi, hd = SHAPES["8 pairs per tile"]
    stream, m = _roundtrip(C.one_binade_both_signs(N, K), epi, hd)   # one binade, both signs
    assert m.n_wide == 0 and (m.table >> 31 == 0).all()
    # base = the block's largest exponent - 15: 127 for [1, 2), 128 where a value rounded up to 2.0 in bf16
    assert set(((m.table >> 23) & 0xFF).tolist()) <= {127 - 15, 128 - 15}
    assert m.nbytes < 0.77 * stream.nbytes


def test_all_wide_matrix():
    N, K, epi, hd = SHAPES["5 pairs per tile"]
    stream, m = _roundtrip(C.all_wide(N, K), epi, hd)     # an exact zero in every chunk
    assert m.n_wide == m.n_blocks
    wide = m.table[m.table >> 31 == 1] & 0x7FFFFF
    assert np.array_equal(np.sort(wide), np.arange(m.n_blocks))    # numbered once each, in stream order
    assert np.array_equal(wide, np.sort(wide))


@pytest.mark.parametrize("what", list(FORCERS))
@pytest.mark.parametrize("name", ["8 pairs per tile", "5 pairs per tile", "odd N head"])
def test_one_value_forces_its_block_wide(what, name):
    N, K, epi, hd = SHAPES[name]
    if name == "odd N head":
        N -= 1                                            # (even N here: the zero row of an odd N is its own forcer, below)
    wb = C.forcer_case(N, K, what)                        # every block narrow but the one of (N // 3, 40)
    stream, m = _roundtrip(wb, epi, hd)
    assert m.n_wide == 1
    # the wide block is the one that holds (r, k): its 16 raw bytes per chunk come back, its neighbours alternate narrow
    pos = int(np.nonzero(stream == FORCERS[what])[0][0])
    idx, base, narrow = w12.block_classes(stream, _n_pairs(N, epi), K)
    wide_entry = int(np.nonzero(m.table >> 31)[0][0])
    assert wide_entry == int(idx[~narrow][0])
    assert stream[pos] == FORCERS[what]


def test_odd_n_zero_row_is_wide_and_exact():
    N, K, epi, hd = SHAPES["odd N head"]
    g = torch.Generator().manual_seed(4)
    stream, m = _roundtrip(_bits(1.0 + torch.rand(N, K, generator=g)), epi, hd)
    assert m.n_wide == K // 32                            # the last tile's blocks hold the zero row


def test_alternating_wide_and_narrow_blocks():
    N, K, epi, hd = 64, 512, w12.EPI_RESID, 0             # one pair per tile, 16 steps per tile
    stream, m = _roundtrip(C.alternating(N, K), epi, hd)  # a zero in every other 32-k step of every row
    flags = (m.table >> 31).reshape(-1, K // 32)
    assert (flags[:, 0::2] == 1).all() and (flags[:, 1::2] == 0).all()


def test_codes_are_the_documented_bit_layout():
    bits = np.array([[0x3F80, 0xBF81, 0x4000, 0x3E7F, 0x3F80, 0x3F80, 0x3F80, 0xC07F]], dtype=np.uint16)   # 1, -1.0078, 2, ...
    base = 128 - 15
    codes = w12.encode_codes(bits, base)
    v = int.from_bytes(codes[0].tobytes(), "little")
    for i, b in enumerate(bits[0].tolist()):
        c = (v >> (12 * i)) & 0xFFF
        assert c == ((b >> 15) << 11) | ((((b >> 7) & 0xFF) - base) << 7) | (b & 0x7F)
        assert (((c & 0x800) << 4) | ((c & 0x7FF) + (base << 7))) == b
    assert np.array_equal(w12.decode_codes(codes, base), bits)


def test_size_rule():
    # 1536 pairs x 3072 (the 3B out-projection): 3 % wide blocks leave the copy ~0.76 of bf16, all wide makes it larger than bf16
    n_pairs, K = 1536, 3072
    blocks = w12.table_entries(n_pairs, K)
    bf16 = n_pairs * 2 * K * 2
    assert 0.75 < w12.w12_bytes(n_pairs, K, int(0.03 * blocks)) / bf16 < 0.77
    assert w12.w12_bytes(n_pairs, K, blocks) > bf16 * (1 - w12.MIN_SAVING)
