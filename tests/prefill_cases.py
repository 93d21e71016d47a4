"""The cases of tests/test_hip_prefill_rows_fp64_gpu.py, as data, with the host-only helpers that plan them.

A GEMM-prefilled prompt runs, per chunk of <= 512 positions and per layer, four products of the native MFMA GEMM
(csrc/prefill_mfma.hip). Which instantiation a product runs, over how many row blocks and token blocks, and whether its
workgroups are dealt to blocks through the XCD swizzle, is decided by the launcher; `sd_prefill_plan` answers from the same
functions. Every case below is one prompt into a one-layer `random_init` model; `PINS` holds the plan of every (model,
chunk size) the cases run, so tests/test_prefill_plan_cpu.py can prove on a machine without a GPU that the cases reach every
class the plan can produce, and the GPU test can refuse to run a case whose plan has drifted.

Nothing here touches a device."""

import dataclasses
import functools
from typing import Optional, Tuple

import stage_ref as R
from gemm_body_cases import S1B, S3B, S8B, TOY, llama
from specdec_hip import weights as W
from specdec_hip.ops import prefill_plan

CHUNK = 512                    # positions per GEMM chunk (kPrefillChunk, csrc/prefill_gemm.h)
PRODUCTS = ("qkv", "out", "gate_up", "down")

TOY128 = llama("toy-d128", 384, 3, 1, 128, 1024)          # (tests/test_hip_stage_fp64_gpu.py: the same name, the same weights)
# the smallest shapes that reach the classes the toys cannot:
# 128-row blocks need >= 256 workgroups, i.e. >= 64 blocks of 128 rows at 4 token blocks — gate / up of d_ff 4096 with four k-stages
WIDE = llama("wide-ff4096", 256, 4, 2, 64, 4096)
# ... and on the other three products N >= 8192; on a grid that is no multiple of 8 they need >= 86 row blocks of 128 at three token
# blocks. One constructed shape does both (no shipped model is this wide; a 70B layer is the nearest): d_model 10240 (out and down),
# 64 + 2 x 8 heads of 128 (QKV rows 10240), 86 row blocks each: 86 x 4 = 344 workgroups at 512 positions (swizzled), 86 x 3 = 258 at
# 300 (not). d_ff is the narrowest there is, which makes the down product a single k-stage.
TALL = llama("tall-d10240", 10240, 64, 8, 128, 64)
# a gate / up grid that is no multiple of 8 with 64-row blocks: 2 x 192 rows = 6 row blocks
ODD = llama("toy-ff192", 256, 4, 2, 64, 192)

MODELS = {c.name: c for c in (TOY, TOY128, WIDE, TALL, ODD, S1B, S3B, S8B)}
# the shapes the project runs (specdec_hip.weights), for the closure of the case list
PRODUCTION = (W.LLAMA_3_2_1B, W.LLAMA_3_2_3B, W.LLAMA_3_8B)


@functools.lru_cache(maxsize=None)
def _plan(key: Tuple, which: int, T: int, w8: bool):
    return prefill_plan(*key, which, T, w8)


def plan(cfg: W.ModelConfig, which: int, T: int, wd: str = "bf16"):
    """ops.prefill_plan of `cfg` (what HipModel.prefill_plan returns for a model of it)"""
    return _plan((cfg.arch, cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.d_ff), which, T, wd == "fp8")


def summary(p) -> Tuple:
    """what a pin holds of one product's plan: (block height, row blocks, token blocks, swizzled, fewest rows in a row block)"""
    return (p.rb, p.row_blocks, p.token_blocks, p.swizzled, p.min_block_rows)


def last_class(rows: int) -> str:
    return {1: "1", 127: "127", 128: "128"}.get(rows, "other")


def classes(cfg: W.ModelConfig, T: int, wd: str):
    """the classes one chunk of T positions of `cfg` puts under test, per product"""
    out = set()
    for which in range(4):
        p = plan(cfg, which, T, wd)
        out |= {("height", which, p.rb, wd), ("swizzle", which, p.rb, p.swizzled), ("token_blocks", which, p.token_blocks),
                ("last_rows", which, last_class(p.last_rows)), ("short_block", which, p.min_block_rows < p.rb)}
    out.add(("qkv_head_dim", cfg.head_dim))
    return out


@dataclasses.dataclass(frozen=True)
class Case:
    model: str                      # key of MODELS
    wd: str                         # "bf16" / "fp8"
    backend: str                    # "native" / "rocblas"
    L: int                          # positions of the prompt (per row)
    pos0: int = 0                   # first position (a continuation after a cached prefix)
    B: int = 1                      # rows of the call (the last one is checked)
    row: int = 0                    # first cache row
    batch: int = 1                  # rows of the bound cache
    page: Optional[int] = None      # page length of a paged cache

    @property
    def cfg(self) -> W.ModelConfig:
        return MODELS[self.model]

    @property
    def id(self) -> str:
        s = f"{self.backend}-{self.model}-{self.wd}-L{self.L}"
        if self.pos0:
            s += f"-p{self.pos0}"
        if self.B > 1 or self.row:
            s += f"-B{self.B}-row{self.row}"
        if self.page:
            s += f"-page{self.page}"
        return s

    def chunks(self):
        """[(first position of the chunk within the prompt, positions)]"""
        return [(m0, min(CHUNK, self.L - m0)) for m0 in range(0, self.L, CHUNK)]

    def chunk_sizes(self):
        return sorted({mc for _, mc in self.chunks()})

    def classes(self):
        out = set()
        for mc in self.chunk_sizes():
            out |= classes(self.cfg, mc, self.wd)
        return out


def _c(cfg, wd, backend, L, **kw):
    return Case(cfg.name, wd, backend, L, **kw)


# every position of the last chunk: a single partial block, the 127- and 128-row blocks, a 1-row block, 3 blocks, a full chunk, a
# 1-position second chunk, a partial and a full second chunk (positions 512-1023: over the split-KV boundary)
TOY_L = (96, 127, 128, 129, 300, 512, 513, 700, 1024)
CASES = (
    [_c(TOY, "bf16", "native", L) for L in TOY_L]
    + [_c(TOY, "fp8", "native", L) for L in (127, 129, 512, 513)]
    + [_c(TOY, "bf16", "rocblas", L) for L in (96, 129, 512, 700)]
    + [_c(TOY128, "bf16", "native", 333), _c(ODD, "bf16", "native", 100)]
    + [_c(WIDE, "bf16", "native", 512), _c(WIDE, "fp8", "native", 512)]
    + [_c(TALL, "bf16", "native", 512), _c(TALL, "fp8", "native", 512), _c(TALL, "bf16", "native", 300)]
    + [_c(S1B, "bf16", "native", 300), _c(S1B, "fp8", "native", 300)]
    + [_c(S3B, "bf16", "native", 300)]
    + [_c(S8B, "bf16", "native", 129), _c(S8B, "bf16", "native", 257)]
)
# a continuation at pos0 = 200 into row 1 of a 3-row batch, and a B = 2 prompt whose checked row is the second
CONTINUATION = [_c(TOY, "bf16", b, 512, pos0=200, row=1, batch=3) for b in ("native", "rocblas")]
BATCHED = [_c(TOY, "bf16", b, 300, B=2, row=1, batch=3) for b in ("native", "rocblas")]
PAGED = [_c(TOY, "bf16", "native", 300, page=64)]
TWO_LAYER = dataclasses.replace(TOY, n_layers=2, name="toy-d64-2l")
ALL_CASES = CASES + CONTINUATION + BATCHED + PAGED

# (model, chunk positions) -> per product (block height, row blocks, token blocks, swizzled, fewest rows in a row block); fp8 storage
# changes the kernel's name and nothing else of the plan
PINS = {
    ("toy-d64", 96): ((64, 8, 1, True, 64), (64, 4, 1, False, 64), (64, 16, 1, True, 64), (64, 4, 1, False, 64)),
    ("toy-d64", 127): ((64, 8, 1, True, 64), (64, 4, 1, False, 64), (64, 16, 1, True, 64), (64, 4, 1, False, 64)),
    ("toy-d64", 128): ((64, 8, 1, True, 64), (64, 4, 1, False, 64), (64, 16, 1, True, 64), (64, 4, 1, False, 64)),
    ("toy-d64", 129): ((64, 8, 2, True, 64), (64, 4, 2, True, 64), (64, 16, 2, True, 64), (64, 4, 2, True, 64)),
    ("toy-d64", 300): ((64, 8, 3, True, 64), (64, 4, 3, False, 64), (64, 16, 3, True, 64), (64, 4, 3, False, 64)),
    ("toy-d64", 512): ((64, 8, 4, True, 64), (64, 4, 4, True, 64), (64, 16, 4, True, 64), (64, 4, 4, True, 64)),
    ("toy-d64", 1): ((64, 8, 1, True, 64), (64, 4, 1, False, 64), (64, 16, 1, True, 64), (64, 4, 1, False, 64)),
    ("toy-d64", 188): ((64, 8, 2, True, 64), (64, 4, 2, True, 64), (64, 16, 2, True, 64), (64, 4, 2, True, 64)),
    ("toy-d128", 333): ((64, 10, 3, False, 64), (64, 6, 3, False, 64), (64, 32, 3, True, 64), (64, 6, 3, False, 64)),
    ("toy-ff192", 100): ((64, 8, 1, True, 64), (64, 4, 1, False, 64), (64, 6, 1, False, 64), (64, 4, 1, False, 64)),
    ("wide-ff4096", 512): ((64, 8, 4, True, 64), (64, 4, 4, True, 64), (128, 64, 4, True, 128), (64, 4, 4, True, 64)),
    ("tall-d10240", 512): ((128, 86, 4, True, 40), (128, 86, 4, True, 40), (64, 2, 4, True, 64), (128, 86, 4, True, 40)),
    ("tall-d10240", 300): ((128, 86, 3, False, 40), (128, 86, 3, False, 40), (64, 2, 3, False, 64), (128, 86, 3, False, 40)),
    ("1b-layer", 300): ((64, 52, 3, False, 12), (64, 32, 3, True, 64), (128, 128, 3, True, 128), (64, 32, 3, True, 64)),
    ("3b-layer", 300): ((64, 86, 3, False, 20), (64, 52, 3, False, 12), (128, 128, 3, True, 128), (64, 52, 3, False, 12)),
    ("8b-layer", 129): ((64, 103, 2, False, 24), (64, 64, 2, True, 64), (128, 228, 2, True, 70), (64, 64, 2, True, 64)),
    ("8b-layer", 257): ((64, 103, 3, False, 24), (64, 64, 3, True, 64), (128, 228, 3, False, 70), (64, 64, 3, True, 64)),
}


# ---- the spike token of the future-key cases -----------------------------------------------------------------------------------
SPIKE_TOKEN, SPIKE_CHANNEL, SPIKE_GAIN = 3, 5, 256.0


def spike_weights(mw: W.ModelWeights) -> W.ModelWeights:
    """A copy of one-layer Llama weights with one "spike" token whose V row is about SPIKE_GAIN times any other token's.
    RMSNorm keeps a row's direction, not its scale, so the spike comes from the direction: the spike token's embedding is one
    channel, no other token's embedding has that channel, and the V rows of wqkv are scaled by SPIKE_GAIN (a power of two: exact
    in bf16) on that column. Its K row and its q stay of ordinary size, so a query that saw a spike key would weigh it like any
    other key and move by about SPIKE_GAIN / (keys it sees) of the V scale."""
    c = mw.config
    tok = mw.tok_emb.clone()
    tok[:, SPIKE_CHANNEL] = 0
    tok[SPIKE_TOKEN] = 0
    tok[SPIKE_TOKEN, SPIKE_CHANNEL] = 1.0
    lw = mw.layers[0]
    wqkv = lw.wqkv.clone()
    v0 = (c.n_heads + c.n_kv_heads) * c.head_dim
    wqkv[v0:, SPIKE_CHANNEL] = (wqkv[v0:, SPIKE_CHANNEL].float() * SPIKE_GAIN).to(wqkv.dtype)
    layers = [dataclasses.replace(lw, wqkv=wqkv)] + list(mw.layers[1:])
    return dataclasses.replace(mw, tok_emb=tok, layers=layers, meta={})


# (prompt positions, first spike position): the spike token at every position >= s — in the second, third and fourth attention
# sub-pass of a 512-chunk, and in the second chunk of a 1024 prompt (every query before s has spike keys of its own future in the cache)
FUTURE = [(512, 130), (512, 300), (512, 400), (1024, 712)]


# ---- the tile list, restated -----------------------------------------------------------------------------------------------------
def tiles(n_pairs: int, K: int):
    """[(first pair, pairs)] of a matrix's packed stream, from the work split (stage_ref.gemv_geometry)"""
    g = R.gemv_geometry(n_pairs, K)
    out = []
    for lo in range(0, n_pairs, g["ppw"]):
        hi = min(lo + g["ppw"], n_pairs)
        out += [(p0, min(g["tile_pairs"], hi - p0)) for p0 in range(lo, hi, g["tile_pairs"])]
    return out


def product_shape(cfg: W.ModelConfig, which: int):
    """(row pairs, K) of a layer product of a Llama model"""
    d, HqD, ff = cfg.d_model, cfg.n_heads * cfg.head_dim, cfg.d_ff
    return (((cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim // 2, d), (d // 2, HqD), (ff, d), (d // 2, ff))[which]
