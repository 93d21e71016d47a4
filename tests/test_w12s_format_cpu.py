"""W12S, the split-byte form of the W12 weight copy (csrc/gemv_device.h, csrc/pack.hip), as restated in
specdec_hip/w12.py: pack, then unpack, equals the input bit for bit. No tolerance appears here.

A narrow block keeps its low bytes raw and its high bytes h = sign<<7 | exp>>1 as 4-bit codes over a base
B = max(0, (emax>>1) - 7): the exponents that fit are the EVEN-ALIGNED window 2B .. 2B + 15. With an odd largest exponent
the window ends at it and 16 consecutive exponents fit; with an even one the window reaches one past it and only the 15
below-and-including it do, so a span of 16 is already wide there (the cases below pin both)."""

import numpy as np
import pytest

import w12_cases as C
from specdec_hip import w12
from w12_cases import FORCERS, SHAPES, SPLIT_SPANS, bf16 as _bf16, exps as _exps, one_binade as _one_binade


def _roundtrip(wb, epi, head_dim):
    N, K = wb.shape
    n_pairs = (N + 1) // 2
    stream = w12.pack_bf16(wb, n_pairs, epi, head_dim)
    m = w12.w12s_pack(stream, n_pairs, K)
    back = w12.w12s_unpack(m, n_pairs, K)
    assert back.dtype == stream.dtype and np.array_equal(back, stream)
    assert m.main.nbytes * 4 == stream.nbytes * 3 and m.ovf.nbytes == m.n_wide * w12.OVF_BLOCK
    assert m.table.size == w12.table_entries(n_pairs, K)
    # the exponent rule and the widen-and-compare rule name the same blocks
    idx, base, narrow = w12.block_classes(stream, n_pairs, K, w12.W12_SPLIT)
    assert np.array_equal((m.table[idx] >> 31) == 0, narrow)
    assert np.array_equal(((m.table[idx] >> 23) & 0xFF)[narrow], base[narrow])
    return stream, m


# ---- one pair per tile (N = 64, K = 512): block (p, s) is rows 2p, 2p + 1 x columns 32 s .. 32 s + 31 --------------------------
def _block_case(fill):
    """A [1, 2) matrix whose block (pair 3, step 5) is rewritten by fill(view of its 2 x 32 bits); returns (matrix, its entry)"""
    N, K, epi, hd = SHAPES["1 pair per tile"]
    wb, index = C.block_case(N, K, epi, hd, fill)
    assert index == 3 * (K // 32) + 5
    stream, m = _roundtrip(wb, epi, hd)
    q = w12.geometry(N // 2, K)
    assert q.grid == 32 and q.tile_pairs == 1 and w12.n_tiles_full(q) == 1
    others = np.delete(m.table, 3 * (K // 32) + 5)
    assert (others >> 31 == 0).all()                                   # every other block: one binade, narrow
    return m, int(m.table[3 * (K // 32) + 5])


@pytest.mark.parametrize("name", list(SHAPES))
def test_random_matrices_round_trip(name):
    N, K, epi, hd = SHAPES[name]
    rng = np.random.default_rng(N + K)
    stream, m = _roundtrip(_bf16(rng.standard_normal((N, K)).astype(np.float32) * 0.02), epi, hd)
    assert 0 < m.n_wide < 0.25 * m.n_blocks                             # N(0, s) weights: mostly narrow, some wide


def test_one_binade_with_both_signs_has_no_wide_block():
    N, K, epi, hd = SHAPES["8 pairs per tile"]
    wb = C.one_binade_both_signs(N, K)
    assert np.unique((wb >> 7) & 0xFF).tolist() == [127] and np.unique(wb >> 15).tolist() == [0, 1]
    stream, m = _roundtrip(wb, epi, hd)
    assert m.n_wide == 0 and (m.table >> 31 == 0).all()
    assert set(((m.table >> 23) & 0xFF).tolist()) == {(127 >> 1) - 7}
    assert m.nbytes < 0.77 * stream.nbytes


def test_the_span_cases_are_the_window_edges():
    # odd largest exponent: the window 112..127 ends at it; even: the window 114..129 reaches one past it, 15 values fit below
    assert SPLIT_SPANS == [(127, 16, True), (127, 17, False), (128, 15, True), (128, 16, False), (128, 17, False)]
    assert np.array_equal(np.unique((_exps(112, 127) >> 7) & 0xFF), np.arange(112, 128))


@pytest.mark.parametrize("emax, span, narrow", SPLIT_SPANS)
def test_exponent_span_against_the_even_aligned_window(emax, span, narrow):
    m, ent = _block_case(C.fill_span(emax, span))
    assert (ent >> 31 == 0) == narrow and m.n_wide == (0 if narrow else 1)
    if narrow:
        assert (ent >> 23) & 0xFF == (emax >> 1) - 7


def test_all_eight_offsets_and_both_signs_in_one_lane():
    lane = C.OFFSETS_LANE
    m, ent = _block_case(C.fill_offsets)
    assert ent >> 31 == 0 and (ent >> 23) & 0xFF == 56
    codes = w12.encode_split(lane[None], 56)[0, 8:]
    nib = np.concatenate([codes & 0xF, codes >> 4])
    assert sorted((nib & 7).tolist()) == list(range(8)) and set((nib >> 3).tolist()) == {0, 1}


def test_base_is_clamped_at_zero():
    m, ent = _block_case(C.fill_base0)   # zeros' and denormals' exponent 0 up to 15: h = 0..7, base 0
    assert ent == 0                      # narrow, base 0: no value is special, only the span decides
    m, ent = _block_case(C.fill_base0_wide)
    assert ent >> 31 == 1


def test_exponents_254_and_255_inside_a_fitting_window():
    m, ent = _block_case(C.fill_254_255)   # inf and nan patterns among huge values: h = 120..127
    assert ent >> 31 == 0 and (ent >> 23) & 0xFF == 120


@pytest.mark.parametrize("what", list(FORCERS))
@pytest.mark.parametrize("name", ["8 pairs per tile", "5 pairs per tile", "odd N head"])
def test_one_value_forces_exactly_one_block_wide(what, name):
    N, K, epi, hd = SHAPES[name]
    if name == "odd N head":
        N -= 1                           # (even N here: the zero row of an odd N is a forcer of its own, below)
    wb = C.forcer_case(N, K, what)
    stream, m = _roundtrip(wb, epi, hd)
    assert m.n_wide == 1
    idx, base, narrow = w12.block_classes(stream, (N + 1) // 2, K, w12.W12_SPLIT)
    assert int(np.nonzero(m.table >> 31)[0][0]) == int(idx[~narrow][0])


def test_odd_n_zero_row_is_wide_and_exact():
    N, K, epi, hd = SHAPES["odd N head"]
    stream, m = _roundtrip(_one_binade(N, K, 4), epi, hd)
    assert m.n_wide == K // 32           # the last tile's blocks hold the zero row


def test_alternating_wide_and_narrow_blocks_along_k():
    N, K, epi, hd = SHAPES["1 pair per tile"]
    wb = C.alternating(N, K)
    stream, m = _roundtrip(wb, epi, hd)
    flags = (m.table >> 31).reshape(-1, K // 32)
    assert (flags[:, 0::2] == 1).all() and (flags[:, 1::2] == 0).all()
    wide = m.table[m.table >> 31 == 1] & 0x7FFFFF
    assert np.array_equal(wide, np.arange(m.n_wide))                    # numbered once each, in stream order


def test_a_hand_written_lane_has_the_documented_layout():
    #                 1.0     -1.0078  2.0     0.2480  -3.98   1.0     0.0156  -1.5
    bits = np.array([[0x3F80, 0xBF81, 0x4000, 0x3E7E, 0xC07F, 0x3F80, 0x3C80, 0xBFC0]], dtype=np.uint16)
    base = (128 >> 1) - 7                # 57: high bytes 57..64, exponents 114..129
    out = w12.encode_split(bits, base)[0]
    assert out[:8].tolist() == [0x80, 0x81, 0x00, 0x7E, 0x7F, 0x80, 0x80, 0xC0]            # dwords 0, 1: the low bytes, weight i at byte i
    code = [0x3F - 57, 8 | (0x3F - 57), 0x40 - 57, 0x3E - 57, 8 | (0x40 - 57), 0x3F - 57, 0x3C - 57, 8 | (0x3F - 57)]
    assert out[8:].tolist() == [code[j] | (code[j + 4] << 4) for j in range(4)]             # dword 2: byte j = code[j] | code[j+4] << 4
    assert out[8:].tolist() == [0xF6, 0x6E, 0x37, 0xE5]
    assert np.array_equal(w12.decode_split(out[None], base), bits)
    for c, b in zip(code, bits[0].tolist()):
        assert ((((c & 8) << 4) | ((c & 7) + base)) << 8) | (b & 0xFF) == b


def test_size_rule_for_the_3b_out_projection():
    n_pairs, K = 1536, 3072
    blocks = w12.table_entries(n_pairs, K)
    bf16 = n_pairs * 2 * K * 2
    assert 0.75 < w12.w12_bytes(n_pairs, K, int(0.04 * blocks)) / bf16 < 0.77          # 96 % narrow (measured: 96.04 %)
    assert w12.w12_bytes(n_pairs, K, int(0.04 * blocks)) <= (1 - w12.MIN_SAVING) * bf16
    assert w12.w12_bytes(n_pairs, K, blocks) > bf16 * (1 - w12.MIN_SAVING)             # all wide: not taken


def test_narrow_share_of_normal_weights():
    """randn measures 95.0 % (profiles/w12_split.md); the floor is a condition of the size rule's margin, not a guess at it"""
    N = K = 4096                          # 8 pairs per tile: the largest blocks, narrow least often
    rng = np.random.default_rng(6)
    stream = w12.pack_bf16(_bf16(rng.standard_normal((N, K)).astype(np.float32) * 0.02), N // 2, w12.EPI_RESID)
    assert w12.narrow_share(stream, N // 2, K, w12.W12_SPLIT) >= 0.90
    assert w12.narrow_share(stream, N // 2, K, w12.W12_SPLIT) <= w12.narrow_share(stream, N // 2, K, w12.W12_CODES)
