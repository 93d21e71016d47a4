"""The cases of tests/test_hip_persist_fp64_gpu.py, as data, with the host-only planner calls that name them.

The persistent forward (csrc/persist.hip) is one kernel in four instantiations that matter numerically, persist<D,HC>: D the head
dimension, HC the 1024-granule chunks of a d_model-wide row. Which one a pass runs, and how many tokens a pass of a model can
hold, is the library's decision (`sd_persist_plan`: the functions the bind and the launch ask). Every case below is one pass of
B rows x M tokens; tests/test_persist_plan_cpu.py proves on a machine without a GPU that the list reaches every instantiation at
every token count its model can hold, every (B, M) class and both parities of M >= 3, and the GPU test refuses to run a case
whose plan has drifted.

Nothing here touches a device."""

import dataclasses
from typing import Optional, Tuple

from gemm_body_cases import L3, S1B, S3B, TOY, llama
from specdec_hip import weights as W
from specdec_hip.ops import persist_plan

# one-layer models, vocab 512, random_init (un-damped) unless stated; names shared with the stage tests where the shape is theirs
# (one cache of weights serves the files). What each is for:
#   toy       out / down cut for 128 workgroups: half the CUs own no d_model-wide rows
#   toy128    QKV cut for 160 workgroups, a group of 3 q heads, an odd vocabulary: a last pair with one row
#   1b-layer  4 gate / up tiles; the two-wave sweep of the 4096-granule activation row
#   3b-layer  2 QKV tiles, two chunks
#   wide-d64  a wide model with 64-wide heads: the only way into persist<64,2>; a group of 9; QKV 235 and down 231 workgroups
#   widest    the d_model limit: two full 1024-granule chunks
#   heads64   64 q heads: 4 rows x 1 token are 256 attention units (every CU has one), and 5 rows exceed the CUs at T = 5
TOY128 = llama("toy-d128-v3001", 384, 3, 1, 128, 1024, vocab=3001)
WIDE64 = llama("wide-d64", 2304, 36, 4, 64, 6144)
WIDEST = llama("widest", 4096, 32, 8, 128, 12288)
HEADS64 = llama("heads64", 256, 64, 8, 64, 512)
S1B_TIED = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=1, d_model=2048, n_heads=32, n_kv_heads=8, head_dim=64, d_ff=8192, vocab=128256,
                         max_pos=4096, rope_theta=500000.0, rope_scaling=L3, tie_embeddings=True, name="1b-layer-fullvocab-tied")
TOY_3L = dataclasses.replace(TOY, n_layers=3, name="toy-d64-3l")
TOY128_2L = dataclasses.replace(TOY128, n_layers=2, name="toy-d128-v3001-2l")
TOY_60L = dataclasses.replace(TOY, n_layers=60, name="toy-d64-60l")
TOY_61L = dataclasses.replace(TOY, n_layers=61, name="toy-d64-61l")

MODELS = {c.name: c for c in (TOY, TOY128, S1B, S3B, WIDE64, WIDEST, HEADS64, S1B_TIED, TOY_3L, TOY128_2L, TOY_60L, TOY_61L)}
# the table of the models above: (instantiation, tokens per pass), pinned by tests/test_persist_plan_cpu.py against the library
TABLE = {"toy-d64": ("persist<64,1>", 8), "toy-d128-v3001": ("persist<128,1>", 8), "1b-layer": ("persist<64,1>", 5),
         "3b-layer": ("persist<128,2>", 4), "wide-d64": ("persist<64,2>", 6), "widest": ("persist<128,2>", 3)}
INSTANCES = ("persist<64,1>", "persist<64,2>", "persist<128,1>", "persist<128,2>")


def plan(cfg: W.ModelConfig, T: int = 1, **facts):
    """ops.persist_plan of a config (what HipModel.persist_plan returns for a bound bf16 packed model of it)"""
    return persist_plan(cfg.arch, cfg.n_layers, cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.d_ff, cfg.vocab, T, **facts)


@dataclasses.dataclass(frozen=True)
class Case:
    model: str                      # key of MODELS
    B: int                          # rows of the pass ...
    M: int                          # ... x tokens per row: T = B * M
    pos_base: Tuple[int, ...] = ()  # cached prefix length per row (default: 3 for the one row)
    row0: int = 0                   # first cache row of the pass (of a bound batch of row0 + B + 1)
    l_max: int = 1280               # cache rows bound (<= 1280: the length hint admits the launch)
    prefix: str = "spikes"          # "spikes" (x 256 V at pos0 - 1, 31, 32), "peaked" (K x 32), "stale" (spikes at every
                                    # position from pos0 to pos0 + M + 64: the in-pass causality construction)
    page_len: Optional[int] = None  # (dense KV only: the attribute the shared helpers of gemm_body_run.py read)

    @property
    def T(self):
        return self.B * self.M

    @property
    def cfg(self):
        return MODELS[self.model]

    @property
    def bases(self):
        return self.pos_base or tuple([3] * self.B)

    @property
    def id(self):
        s = f"{self.model}-{self.B}x{self.M}"
        if self.pos_base:
            s += "-p" + ".".join(str(p) for p in self.pos_base)
        if self.row0:
            s += f"-row{self.row0}"
        if self.l_max != 1280:
            s += f"-L{self.l_max}"
        if self.prefix != "spikes":
            s += f"-{self.prefix}"
        return s

    def name(self):
        """the instantiation the planner names for this pass ("none": not a persistent pass)"""
        return plan(self.cfg, self.T).name


def _ragged(B, seed):
    """B ragged prefix lengths around the attention's 32-key blocks, deterministic"""
    pool = [0, 1, 31, 32, 33, 63, 64, 65, 5, 17, 40, 95, 96, 2, 47, 70]
    return tuple(pool[(i * 7 + seed) % len(pool)] for i in range(B))


# ---- 1. tokens and rows ------------------------------------------------------------------------------------------------------------
# every (B, M) class: one row of 1..8 tokens, 2 / 3 / 5 / 8 rows of one token, and the five mixed shapes
CLASSES = [(1, M) for M in range(1, 9)] + [(B, 1) for B in (2, 3, 5, 8)] + [(2, 2), (2, 3), (3, 2), (2, 4), (4, 2)]
GRID_CASES = (
    [Case(m, B, M, _ragged(B, B + M) if B > 1 else (), row0=(1 if B > 1 and M > 1 else 0)) for m in ("toy-d64", "toy-d128-v3001") for (B, M) in CLASSES]
    # the three large models and the wide 64-head one: one row of 1..cap tokens (cap: TABLE; the CPU proof checks the sweep is whole)
    + [Case("1b-layer", 1, T) for T in range(1, 6)]
    + [Case("3b-layer", 1, T) for T in range(1, 5)]
    + [Case("wide-d64", 1, T) for T in range(1, 7)]
    + [Case("widest", 1, T) for T in range(1, 4)]
    # 1B dimensions: as many rows as a pass holds there (5: 160 attention units)
    + [Case("1b-layer", 5, 1, _ragged(5, 2), row0=2)]
    # 256 attention units: every CU has one
    + [Case("heads64", 4, 1, _ragged(4, 1), row0=1)]
)
# passes the engine must NOT run persistently, and must still get right on the launch path: more attention units than CUs at a
# token count the model holds (B * Hq <= 256), and 8 / 9 rows at 1B dimensions (above its 5 tokens per pass)
LAUNCH_CASES = [Case("heads64", 5, 1, _ragged(5, 3)), Case("1b-layer", 8, 1, _ragged(8, 4)), Case("1b-layer", 9, 1, _ragged(9, 5))]

# ---- 2. attention edges ------------------------------------------------------------------------------------------------------------
EDGE_LENGTHS = (0, 1, 31, 32, 33, 95, 96, 97, 511, 512)
EDGE_SHAPES = [("toy-d64", 1), ("toy-d64", 3), ("toy-d64", 8), ("toy-d128-v3001", 2), ("toy-d128-v3001", 5)]
EDGE_CASES = [Case(m, 1, M, (p,), prefix=kind) for (m, M) in EDGE_SHAPES for kind in ("spikes", "peaked") for p in EDGE_LENGTHS]
# the end of the cache: the last positions of a 1280-row cache; the smallest legal cache (8 rows: every K row of the first block
# beyond 7 is clamped to row 7, the V^T vectors to keys 0..7); and a cache that ends inside a 32-key block (40 rows) behind a
# cached block whose visible keys stop at 34
END_CASES = (
    [Case(m, 1, M, (1280 - M,), prefix=kind) for (m, M) in EDGE_SHAPES for kind in ("spikes", "peaked")]
    + [Case("toy-d64", 1, 8, (0,), l_max=8), Case("toy-d64", 1, 1, (7,), l_max=8), Case("toy-d128-v3001", 1, 1, (7,), l_max=8, prefix="peaked"),
       Case("toy-d64", 1, 5, (35,), l_max=40), Case("toy-d128-v3001", 1, 8, (32,), l_max=40)]
)
# ---- 3. in-pass causality ----------------------------------------------------------------------------------------------------------
CAUSAL_CASES = [Case("toy-d64", 1, M, (p,), l_max=256, prefix="stale") for (M, p) in ((3, 0), (5, 27), (8, 30), (8, 0))]

# ---- 4. depth: the last layer of a deep model, from the hidden rows of its first n - 1 layers (tests/persist_run.py: run_deep) ----
DEPTH_CASES = (
    [Case("toy-d64-3l", 1, T, (33,)) for T in (1, 3, 8)] + [Case("toy-d128-v3001-2l", 1, T, (31,)) for T in (1, 3, 8)]
    + [Case("toy-d64-3l", 2, 3, (5, 40), row0=1)]
    + [Case("toy-d64-60l", 1, 2, (17,), l_max=64)]
)
DEPTH_LAUNCH_CASE = Case("toy-d64-61l", 1, 2, (17,), l_max=64)

# ---- 5. the production instance (no stage-row stores) -------------------------------------------------------------------------------
NOTAPS_CASES = [Case(m, 1, T, (34,)) for m in ("toy-d64-3l", "toy-d128-v3001", "1b-layer") for T in (1, 2, 5)]

# ---- 6. full vocabulary --------------------------------------------------------------------------------------------------------------
VOCAB_CASE = Case("1b-layer-fullvocab-tied", 1, 5, (9,), l_max=64)

# ---- 7. a run of launches on one engine: M cycles, positions advance -------------------------------------------------------------------
RUN_MODEL, RUN_MS, RUN_LAUNCHES = "toy-d64-3l", (1, 3, 8, 2, 5), 20

ONE_PASS_CASES = GRID_CASES + EDGE_CASES + END_CASES + CAUSAL_CASES
PERSIST_CASES = ONE_PASS_CASES + DEPTH_CASES + NOTAPS_CASES + [VOCAB_CASE]   # every case that must run the persistent launch
