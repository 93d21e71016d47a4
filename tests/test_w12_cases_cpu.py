"""The case builders of tests/w12_cases.py, checked without a GPU against the Python restatement of the format
(specdec_hip/w12.py): what tests/test_hip_w12_edges_gpu.py plants is what it believes it plants.

  * a planted pattern makes exactly the planted blocks wide, in both forms, and the background alone makes none;
  * every GEMV case of the GPU list keeps its W12 copy under the size rule (from block counts alone: no large matrix is built);
  * the window background fills every block's whole window and round-trips through the codes of both forms;
  * the case list reaches every batch depth a W12 launch of a production shape is planned with."""

import dataclasses
import re

import numpy as np
import pytest

import gemv_cases
import w12_cases as C
from specdec_hip import w12
from specdec_hip import weights as W
from specdec_hip.ops import gemv_instance

FORMS = {"w12": w12.W12_CODES, "w12s": w12.W12_SPLIT}

# (N, K, epi, head_dim) for the planting checks: small enough to pack in Python
PLANT_SHAPES = {
    # 2051 pairs = 227 workgroups x 9 + 8: tiles of 5 and 4 pairs (a short last tile), a short last workgroup, 8 slices of 4 steps
    "5 and 4 pairs per tile": (2 * 2051, 1024, w12.EPI_SWIGLU, 0),
    "8 pairs per tile": (4096, 1024, w12.EPI_RESID, 0),           # 2048 pairs, 16 slices of 2 steps
    "16 steps per slice": (64, 8192, w12.EPI_RESID, 0),           # more steps than a deep batch: a first and a last batch that differ
    "qkv pairs, 13 steps": (192, 6656, w12.EPI_QKV_ROPE, 64),     # 96 pairs (i, i + 32), 16 slices of 13 steps: a last batch of one step
}


def _wide_flags(wb, n_pairs, K, epi, hd, form):
    m = w12.w12_pack(w12.pack_bf16(wb, n_pairs, epi, hd), n_pairs, K, form)
    return np.nonzero(m.table >> 31)[0], m


@pytest.mark.parametrize("shape", list(PLANT_SHAPES))
def test_planted_blocks_are_exactly_the_wide_blocks(shape):
    N, K, epi, hd = PLANT_SHAPES[shape]
    n_pairs = C.n_pairs_of(N, epi)
    g = C.grid(n_pairs, K)
    assert g.q.kw * g.q.ksplit == K
    background = C.narrow_background(N, K, N + K)
    seen = {}
    for name in C.PATTERNS:
        for m in (1, 3):
            wb = background.copy()
            planted = C.plant(wb, n_pairs, K, epi, hd, C.pattern(name, m))
            assert np.array_equal(planted, np.sort(planted)) and np.unique(planted).size == planted.size      # table order, once each
            assert (wb != background).sum() == planted.size
            for form in FORMS.values():
                wide, packed = _wide_flags(wb, n_pairs, K, epi, hd, form)
                assert np.array_equal(wide, planted), (shape, name, m, form)
                assert packed.n_wide == planted.size == C.n_planted(n_pairs, K, name, m)
            seen[name, m] = planted
    S, nst = g.S, g.nst
    assert seen["none", 1].size == 0
    for kb in (6, 12):                          # stairs: one block per (tile, slice, batch), every batch position in use
        idx = seen[f"stairs:{kb}", 1]
        gt, s = idx // nst, idx % nst % S
        assert np.array_equal(s % kb, gt % kb)
        assert set((s % kb).tolist()) == set(range(min(kb, S))) or g.gt.size < kb
    idx = seen["runs:12", 1]                    # runs: whole first and last batches
    s = idx % nst % S
    assert set(s.tolist()) == set(range(min(12, S))) | set(range((S - 1) // 12 * 12, S))
    assert idx.size == g.gt.size * g.q.ksplit * len(set(s.tolist()))
    idx = seen["edges", 1]
    assert set((idx % nst % S).tolist()) == {0, S - 1} and idx.size == g.gt.size * g.q.ksplit * 2
    idx = seen["tail", 1]                       # tail: whole tiles; the last workgroup's, and the short last tile of every other
    tiles = np.unique(idx // nst)
    assert idx.size == tiles.size * nst
    short = g.gt[g.short_last_tile][:, None] if g.short_last_tile.any() else np.zeros((0, 1), dtype=int)
    want = set(short.reshape(-1).tolist()) | set(g.gt[g.last_workgroup].tolist())
    assert set(tiles.tolist()) == want and (g.q.grid - 1) * g.ntf in want
    if shape == "5 and 4 pairs per tile":
        # 227 tiles of 4 pairs, and the last workgroup's 8 pairs as tiles of 5 and 3: both of its tiles are in the set
        assert g.short_last_tile.sum() == g.q.grid and len(want) == g.q.grid + 1


@pytest.mark.parametrize("what, N, K, epi, hd", [
    ("toy-b gate / up", 4096, 256, w12.EPI_SWIGLU, 0), ("toy-b head", 2560, 256, w12.EPI_ARGMAX, 0), ("1B qkv", 3072, 2048, w12.EPI_QKV_ROPE, 64)])
def test_the_background_is_narrow_in_both_forms(what, N, K, epi, hd):
    wb = C.narrow_background(N, K, 3)
    e = (wb >> 7) & 0xFF
    assert 127 - 9 <= e.min() and e.max() <= 127 - 3 and np.unique(wb >> 15).tolist() == [0, 1]
    stream = w12.pack_bf16(wb, C.n_pairs_of(N, epi), epi, hd)
    for form in FORMS.values():
        assert w12.block_classes(stream, C.n_pairs_of(N, epi), K, form)[2].all(), (what, form)


def test_every_gemv_case_keeps_its_copy():
    """the size rule, from the planted counts alone; stairs and none are never thinned where a tile has 4 pairs or more"""
    for model, dims in C.GPU_MODELS.items():
        mats = C.model_matrices(**dims)
        for which in C.UNDER_TEST[model]:
            N, K, epi, hd = mats[which]
            n_pairs = C.n_pairs_of(N, epi)
            assert C.covered(n_pairs, K), (model, which)
            g = C.grid(n_pairs, K)
            for name in C.PATTERNS:
                m = C.thinning(n_pairs, K, name)
                n = C.n_planted(n_pairs, K, name, m)
                assert C.taken(n_pairs, K, n) and (m == 1 or not C.taken(n_pairs, K, C.n_planted(n_pairs, K, name, m - 1)))
                assert n > 0 or name == "none"
                if name in C.UNTHINNED and g.q.tile_pairs >= 4:
                    assert m == 1, (model, which, name)
            # stairs of period 6: a sixth of the blocks
            if g.gt.size % 6 == 0 or g.S % 6 == 0:
                assert C.n_planted(n_pairs, K, "stairs:6", 1) * 6 == g.gt.size * g.nst
    assert not C.covered(2048, 14336)            # the 8B down-projection: a MASK shape, left on bf16
    # the 1B out-projection (4 pairs per tile: a wide block's 256 overflow bytes are half its bf16 bytes) allows a share of 0.184
    blocks = w12.table_entries(1024, 2048)
    assert C.taken(1024, 2048, int(0.184 * blocks)) and not C.taken(1024, 2048, int(0.20 * blocks))


def test_the_head_models_have_the_production_split():
    q = w12.geometry(64128, 256)
    assert (q.grid, q.ppw, q.n_tiles, q.tile_pairs, q.ksplit, q.kw // 32, w12.n_tiles_full(q)) == (256, 251, 32, 8, 1, 8, 32)
    assert q == dataclasses.replace(w12.geometry(64128, 2048), kw=256) and 64128 - 255 * 251 == 123      # the 1B lm_head's split
    q = w12.geometry(33000, 1024)
    assert (q.ppw, q.n_tiles, q.tile_pairs, q.ksplit, q.kw // 32, w12.n_tiles_full(q)) == (129, 32, 5, 1, 32, 26)
    q = w12.geometry(16500, 512)
    assert (q.ppw, q.n_tiles, q.ksplit, q.kw // 32) == (65, 16, 1, 16)
    assert w12.geometry(14336, 4096).n_tiles == 8                                                         # the 8B gate / up
    for name, cfg in (("1b", W.LLAMA_3_2_1B), ("3b", W.LLAMA_3_2_3B), ("8b", W.LLAMA_3_8B)):
        d = C.GPU_MODELS[name]
        assert (cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.d_ff) == (d["d_model"], d["n_heads"], d["n_kv_heads"], d["head_dim"], d["d_ff"])
    slices = {(w12.geometry(C.n_pairs_of(N, epi), K).ksplit, w12.geometry(C.n_pairs_of(N, epi), K).kw // 32)
              for m in ("1b", "3b", "8b") for i, (N, K, epi, hd) in enumerate(C.model_matrices(**C.GPU_MODELS[m])) if i in C.UNDER_TEST[m]}
    assert {k for k, _ in slices} == {16, 8, 4, 2} and {s for _, s in slices} >= {4, 12, 16, 24, 64}


@pytest.mark.parametrize("shape", ["1 pair per tile", "5 pairs per tile", "qkv pairs", "odd N head"])
def test_window_background_fills_every_window_and_round_trips(shape):
    N, K, epi, hd = C.SHAPES[shape]
    n_pairs = C.n_pairs_of(N, epi)
    wb, index, top = C.window_background(N, K, epi, hd, 5)
    assert (((wb >> 7) & 0xFF) <= 127 - 4).all()                         # finite products
    stream = w12.pack_bf16(wb, n_pairs, epi, hd)
    K32 = (K + 31) & ~31
    for form, (enc, dec) in ((w12.W12_CODES, (w12.encode_codes, w12.decode_codes)), (w12.W12_SPLIT, (w12.encode_split, w12.decode_split))):
        idx, base, narrow = w12.block_classes(stream, n_pairs, K, form)
        assert np.array_equal(idx, index)
        zero_row = np.zeros(idx.size, dtype=bool)
        if N & 1:
            zero_row[-(K32 // 32):] = True                               # the last tile holds the zero second row of an odd N
        assert narrow[~zero_row].all(), (shape, form)
        assert np.array_equal(base[~zero_row], w12.block_base(top, form)[~zero_row])
        n = 0
        for (c, t, p0, npairs) in w12.tiles(n_pairs, K):
            blk = w12._block_view(stream, p0, npairs, K32)
            for s in range(K32 // 32):
                if narrow[n]:
                    assert np.array_equal(dec(enc(blk[s], base[n]), base[n]), blk[s]), (shape, form, n)
                n += 1
    # every block spans its whole split-byte window: 16 exponents under an odd top, 15 under an even one; every 16th has base 0
    n = 0
    for (c, t, p0, npairs) in w12.tiles(n_pairs, K):
        e = (w12._block_view(stream, p0, npairs, K32) >> 7) & 0xFF
        for s in range(K32 // 32):
            if not (N & 1 and n >= index.size - K32 // 32):
                want = np.arange(top[n] - (15 if top[n] & 1 else 14), top[n] + 1)
                assert np.array_equal(np.unique(e[s]), want), (shape, n)
            n += 1
    assert (top[::16] == 15).all() and set(np.unique(wb >> 15).tolist()) == {0, 1}
    assert (wb == 0x0000).any() and (wb == 0x8000).any() and (((wb >> 7) & 0xFF == 0) & (wb & 0x7F != 0)).any()   # zeros, denormals


def test_edge_cases_have_their_shapes_and_classes():
    """every edge case at the shape of the device test's out-projection and at a shape with more pairs per tile"""
    cases = C.edge_cases()
    assert len(cases) >= 23
    for N, K, epi, hd in (C.SHAPES["1 pair per tile"], C.SHAPES["5 pairs per tile"]):
        n_pairs = C.n_pairs_of(N, epi)
        for name, f in cases.items():
            wb = f(N, K, epi, hd)
            assert wb.shape == (N, K) and wb.dtype == np.uint16, name
        for emax, span, narrow in C.SPLIT_SPANS:
            wb, index = C.block_case(N, K, epi, hd, C.fill_span(emax, span))
            wide, _ = _wide_flags(wb, n_pairs, K, epi, hd, w12.W12_SPLIT)
            assert wide.tolist() == ([] if narrow else [index]), (N, emax, span)
            wide, _ = _wide_flags(wb, n_pairs, K, epi, hd, w12.W12_CODES)
            assert wide.tolist() == ([] if span <= 16 else [index])        # the code form's window ends at the largest exponent


@pytest.mark.parametrize("fill", [C.fill_below_the_clamp, C.fill_zeros_and_denormals, C.fill_base0])
def test_blocks_below_the_clamp_are_narrow_with_base_zero(fill):
    """a largest exponent under 15 (code form) / 14 (split-byte form): the base is CLAMPED at 0, not negative, in both forms"""
    for N, K, epi, hd in (C.SHAPES["1 pair per tile"], C.SHAPES["5 pairs per tile"]):
        wb, index = C.block_case(N, K, epi, hd, fill)
        for form in FORMS.values():
            wide, m = _wide_flags(wb, C.n_pairs_of(N, epi), K, epi, hd, form)
            assert wide.size == 0 and m.table[index] == 0, (N, form)
    b = np.zeros((2, 32), dtype=np.uint16)
    C.fill_below_the_clamp(b)
    assert ((b >> 7) & 0xFF).max() == 9
    C.fill_zeros_and_denormals(b)
    assert ((b >> 7) & 0xFF).max() == 0 and {0x0000, 0x8000} <= set(b.reshape(-1).tolist()) and (b & 0x7F != 0).any()


def _w12_depths(names):
    return {m.group(0) for n in names if "w12" in n for m in [re.search(r"kb\d+", n)]}


def test_the_case_list_reaches_every_batch_depth_of_production():
    """kb6 and kb12: what gemv_instance reports for the W12 / W12S launches of the production shapes at 1..9 tokens"""
    for form in FORMS.values():
        want = set()
        for cfg in gemv_cases.G.PRODUCTION:
            _, _, shapes = gemv_cases.G.model_facts(cfg, "bf16")
            want |= _w12_depths(gemv_instance(T, n_pairs, K, False, pro, epi, w12=form) for T in range(1, 10) for (_, K, n_pairs, epi, pro) in shapes)
        got = set()
        for model, dims in C.GPU_MODELS.items():
            cfg = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=1, name=f"w12-edges-{model}", **dims)
            created, _, shapes = gemv_cases.G.model_facts(cfg, "bf16")
            assert created
            for which in C.UNDER_TEST[model]:
                _, K, n_pairs, epi, pro = shapes[which]
                assert (C.n_pairs_of(C.model_matrices(**dims)[which][0], epi), C.model_matrices(**dims)[which][1]) == (n_pairs, K)
                got |= _w12_depths(gemv_instance(T, n_pairs, K, False, pro, epi, w12=form) for T in C.TOKENS)
        assert want and got >= want, (form, want, got)
