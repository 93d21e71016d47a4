"""sd_prefill_plan on a machine without a GPU: the query itself, the pinned plan of every case of
tests/test_hip_prefill_rows_fp64_gpu.py, the closure of that case list over every class the plan can produce, and the two
things a wrong table would break silently — the row blocks cover every packed row exactly once, and the workgroup-to-block
mapping is a bijection.

A row block or a (row block, token block) that no workgroup computes leaves the previous product's values in the reused Y
buffer: plausible numbers, which only a check of every row of every token block sees. The GPU test checks kernels by plan; a
new block height, threshold or mapping that its case list (tests/prefill_cases.py) does not reach fails here first."""

import ctypes

import pytest

import prefill_cases as P
from specdec_hip import _abi
from specdec_hip import weights as W
from specdec_hip.ops import prefill_plan

LL = W.ARCH_LLAMA


# ---- the entry ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_additive():
    lib = _abi.load()
    for name in ("sd_prefill_plan", "sd_prefill_plan_tables", "sd_model_prefill_rows"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    assert lib.sd_abi_version() == _abi.SD_ABI_VERSION == 1


def test_plan_of_a_known_model():
    """Llama-3.2-1B at 300 positions, written out by hand: QKV is 1536 pairs in 256 tiles of 6 (12 rows), 5 tiles to a 64-row
    block (60 rows: four lanes of every last fragment have no row), 51 such blocks and a last one of a single tile; gate / up is
    8192 pairs in tiles of 8, 128 blocks of 128 rows x 3 token blocks = 384 workgroups >= 256: the tall blocks"""
    c = W.LLAMA_3_2_1B
    p = [P.plan(c, w, 300) for w in range(4)]
    assert [x.name for x in p] == ["mfma<rf2,bf16>", "mfma<rf2,bf16>", "mfma<rf4,bf16>", "mfma<rf2,bf16>"]
    assert [(x.row_blocks, x.token_blocks, x.grid, x.swizzled) for x in p] == [(52, 3, 156, False), (32, 3, 96, True), (128, 3, 384, True), (32, 3, 96, True)]
    assert [x.last_rows for x in p] == [44] * 4 and [x.k_stages for x in p] == [32, 32, 32, 128]
    assert [x.min_block_rows for x in p] == [12, 64, 128, 64]
    assert p[0].blocks[:2] == ((0, 60), (30, 60)) and p[0].blocks[-1] == (1530, 12)
    assert P.plan(c, 2, 300, "fp8").name == "mfma<rf4,fp8>" and P.plan(c, 2, 128, "fp8").name == "mfma<rf2,fp8>"
    # the threshold itself: 128 row blocks of 128 rows fill 256 workgroups from 2 token blocks on
    assert [P.plan(c, 2, T).rb for T in (1, 128, 129, 512)] == [64, 64, 128, 128]


def test_refusals_and_refused_models():
    lib = _abi.load()
    v = [ctypes.c_int(0) for _ in range(8)]
    ptrs = [ctypes.byref(x) for x in v]
    name, reason = ctypes.create_string_buffer(32), ctypes.create_string_buffer(96)
    ok = (LL, 256, 4, 2, 64, 512, 0, 100, 0, 1)
    assert lib.sd_prefill_plan(*ok, *ptrs, name, 32, reason, 96) == 0 and name.value == b"mfma<rf2,bf16>" and reason.value == b""
    assert lib.sd_prefill_plan(*ok, *ptrs[:7], None, name, 32, reason, 96) != 0 and "NULL" in _abi.last_error()
    assert _abi.last_error().startswith("prefill_plan:")
    for cap in (0, 1, len(b"mfma<rf2,bf16>")):       # the name needs its NUL
        name.raw = b"\xaa" * 32
        assert lib.sd_prefill_plan(*ok, *ptrs, name, cap, reason, 96) != 0 and "too short" in _abi.last_error()
        assert name.raw == b"\xaa" * 32                # nothing written
    assert lib.sd_prefill_plan(*ok, *ptrs, name, 32, reason, 0) != 0 and "too short" in _abi.last_error()
    for bad, word in (((LL, 256, 4, 2, 64, 512, 4, 100, 0, 1), "which=4"), ((LL, 256, 4, 2, 64, 512, -1, 100, 0, 1), "which=-1"),
                      ((LL, 256, 4, 2, 64, 512, 0, 0, 0, 1), "T=0"), ((LL, 256, 4, 2, 64, 512, 0, 513, 0, 1), "T=513"),
                      ((LL, 0, 4, 2, 64, 512, 0, 100, 0, 1), "dimension")):
        assert lib.sd_prefill_plan(*bad, *ptrs, name, 32, reason, 96) != 0 and word in _abi.last_error(), bad
    # models the native backend refuses: answered, not an error, with the text sd_model_set_prefill_backend refuses them with
    gpt2 = prefill_plan(W.ARCH_GPT2, 768, 12, 12, 64, 3072, 0, 100)
    assert (gpt2.eligible, gpt2.name, gpt2.grid) == (False, "none", 0) and "Llama models only" in gpt2.reason
    rowmajor = prefill_plan(LL, 256, 4, 2, 64, 512, 0, 100, packed=False)
    assert (rowmajor.eligible, rowmajor.name) == (False, "none") and "packed weights" in rowmajor.reason
    for dims in ((LL, 224, 4, 2, 64, 512), (LL, 256, 3, 1, 32, 512), (LL, 256, 4, 2, 64, 500)):     # d_model, Hq*D, d_ff not in whole 64s
        p = prefill_plan(*dims, 0, 100)
        assert (p.eligible, p.name, p.blocks) == (False, "none", ()) and "multiples of 64" in p.reason, dims
    b, g = (ctypes.c_int * 16)(), (ctypes.c_int * 8)()
    assert lib.sd_prefill_plan_tables(*ok[:8], b, 8, g, 8) == 0
    assert lib.sd_prefill_plan_tables(*ok[:8], b, 7, g, 8) != 0 and "8 row blocks" in _abi.last_error()
    assert lib.sd_prefill_plan_tables(W.ARCH_GPT2, 768, 12, 12, 64, 3072, 0, 100, b, 8, g, 8) != 0 and "Llama models only" in _abi.last_error()


# ---- the pins ----------------------------------------------------------------------------------------------------------------------
def test_every_case_has_its_plan_pinned():
    ids = [c.id for c in P.ALL_CASES]
    assert len(ids) == len(set(ids))
    used = set()
    for c in P.ALL_CASES:
        assert c.L >= 96, c.id                                       # a prompt: the GEMM route (kPrefillMinTokens)
        assert sum(mc for _, mc in c.chunks()) == c.L
        for mc in c.chunk_sizes():
            used.add((c.model, mc))
            got = tuple(P.summary(P.plan(c.cfg, w, mc, c.wd)) for w in range(4))
            assert got == P.PINS[(c.model, mc)], (c.id, mc, got)
            for w in range(4):
                p = P.plan(c.cfg, w, mc, c.wd)
                assert p.eligible and p.name == f"mfma<rf{p.rb // 32},{c.wd}>" and p.grid == p.row_blocks * p.token_blocks
    assert used == set(P.PINS)                                      # no pin without a case


# ---- closure -----------------------------------------------------------------------------------------------------------------------
def _covered():
    out = set()
    for c in P.ALL_CASES:
        if c.backend == "native":
            out |= c.classes()
    return out


def test_cases_reach_every_class_the_models_can_produce():
    """R: every class a chunk of 1 .. 512 positions of Llama-3.2-1B / 3B, Llama-3-8B and of the case list's own models plans,
    bf16 and fp8; C: the classes of the native cases. R must be inside C."""
    C = _covered()
    R = {}
    for cfg in list(P.PRODUCTION) + list(P.MODELS.values()):
        for wd in ("bf16", "fp8"):
            for T in range(1, P.CHUNK + 1):
                for k in P.classes(cfg, T, wd):
                    R.setdefault(k, (cfg.name, wd, T))
    missing = {k: w for k, w in R.items() if k not in C}
    assert not missing, f"planned by a model (first at model, dtype, T) but run by no case: {missing}"
    assert len(R) >= 60           # the sweep really swept (71 when this was written)


def test_cases_reach_the_classes_by_name():
    """the same, spelled out per product: every class of the list below is reached on every product"""
    C = _covered()
    for w in range(4):
        for wd in ("bf16", "fp8"):
            assert ("height", w, 64, wd) in C and ("height", w, 128, wd) in C, (w, wd)
        for rb in (64, 128):
            assert ("swizzle", w, rb, True) in C, (w, rb)
        assert ("swizzle", w, 64, False) in C, w
        for n in (1, 2, 3, 4):
            assert ("token_blocks", w, n) in C, (w, n)
        for last in ("1", "127", "128", "other"):
            assert ("last_rows", w, last) in C, (w, last)
        assert ("short_block", w, True) in C and ("short_block", w, False) in C, w
    assert ("qkv_head_dim", 64) in C and ("qkv_head_dim", 128) in C
    # 128-row blocks on an unswizzled grid: gate / up of the 8B layer at 3 token blocks (228 x 3), the other three products of the
    # d_model 10240 shape at 3 token blocks (86 x 3)
    for w in range(4):
        assert ("swizzle", w, 128, False) in C, w


# ---- the tables --------------------------------------------------------------------------------------------------------------------
def _all_plans():
    seen = set()
    for cfg in list(P.PRODUCTION) + list(P.MODELS.values()):
        for T in (1, 128, 129, 257, 300, 385, 512):
            for w in range(4):
                key = (cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.d_ff, w, (T + 127) // 128)
                if key not in seen:
                    seen.add(key)
                    yield cfg, w, T, P.plan(cfg, w, T)


def test_row_blocks_cover_every_packed_row_exactly_once():
    """the tile list restated from stage_ref.gemv_geometry: every row block is a run of whole consecutive tiles of at most its
    height in rows, the blocks follow each other without a gap, and together they hold the 2 n_pairs packed rows"""
    n = 0
    for cfg, w, T, p in _all_plans():
        n_pairs, K = P.product_shape(cfg, w)
        tl = P.tiles(n_pairs, K)
        assert sum(np for _, np in tl) == n_pairs and [p0 for p0, _ in tl] == [sum(np for _, np in tl[:i]) for i in range(len(tl))][:len(tl)]
        starts = {p0: i for i, (p0, _) in enumerate(tl)}
        nxt = 0
        for first, rows in p.blocks:
            assert first == nxt and first in starts, (cfg.name, w, T, first, nxt)       # starts where the last one ended, on a tile edge
            assert 0 < rows <= p.rb and rows % 2 == 0, (cfg.name, w, T, rows)
            nxt = first + rows // 2
            assert nxt == n_pairs or nxt in starts, (cfg.name, w, T, nxt)               # ends on a tile edge
            # greedy: the next tile would not have fitted
            if nxt != n_pairs:
                assert rows + 2 * tl[starts[nxt]][1] > p.rb, (cfg.name, w, T, first)
        assert nxt == n_pairs and len(p.blocks) == p.row_blocks
        assert p.min_block_rows == min(r for _, r in p.blocks)
        assert p.k_stages * 64 == K
        n += 1
    assert n >= 100


def test_swizzle_is_a_bijection_for_every_grid():
    """every workgroup computes one (row block, token block) and every one is computed: for the grids of the case list and the
    production shapes, and for every grid size up to 1024 through the toy's shapes"""
    for cfg, w, T, p in _all_plans():
        assert sorted(p.wg_block) == list(range(p.grid)), (cfg.name, w, T)
        assert p.swizzled == (p.grid % 8 == 0)
        if not p.swizzled:
            assert list(p.wg_block) == list(range(p.grid))
        else:      # consecutive blocks (the token blocks of one row block) sit on one XCD: workgroups g, g + 8, g + 16, ...
            assert [p.wg_block[g] for g in range(0, p.grid, 8)] == list(range(p.grid // 8))
    grids = set()
    for ff in range(64, 64 * 130, 64):        # gate / up of a d 256 model: 2 ff / 64 row blocks of 64 rows, or ff / 64 of 128
        for T in (100, 200, 300, 400):
            p = prefill_plan(LL, 256, 4, 2, 64, ff, 2, T)
            assert sorted(p.wg_block) == list(range(p.grid)), (ff, T)
            grids.add(p.grid)
    assert len(grids) > 200 and any(g % 8 for g in grids) and any(g % 8 == 0 for g in grids)
