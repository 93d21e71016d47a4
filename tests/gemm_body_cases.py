"""The cases of tests/test_hip_gemm_bodies_gpu.py, as data, with the host-only helpers that plan them.

The multi-token weight-streaming kernels (csrc/gemm_skinny.hip, csrc/gemm_pipe.hip) are one family of template instantiations;
which one a launch runs depends on the token count, the matrix and the work split. `sd_gemm_plan` names it from the
launchers' own decision. Every case below is one pass of a one-layer (or two-layer) `random_init` model; its `names` are
filled in from the plan, so tests/test_gemm_plan_cpu.py can prove on a machine without a GPU that the cases reach every
instantiation the models the project runs can reach, and the GPU test can refuse to run a case whose plan has drifted.

Nothing here touches a device: models are created over placeholder addresses and never bound."""

import ctypes
import dataclasses
import functools
from typing import Optional, Tuple

from specdec_hip import _abi
from specdec_hip import weights as W
from specdec_hip.engine import _LayerWeights, _ModelConfig
from specdec_hip.ops import PLAN_NO_DIRECT, PLAN_NO_PIPE, gemm_plan

LL = W.ARCH_LLAMA
L3 = {"factor": 32.0, "low_freq_factor": 1.0, "high_freq_factor": 4.0, "original_max_position_embeddings": 8192, "rope_type": "llama3"}


def llama(name, d, hq, hkv, D, ff, vocab=512, max_pos=4096, scaling=None, n_layers=1):
    return W.ModelConfig(arch=LL, n_layers=n_layers, d_model=d, n_heads=hq, n_kv_heads=hkv, head_dim=D, d_ff=ff, vocab=vocab,
                         max_pos=max_pos, rope_theta=500000.0, rope_scaling=scaling, tie_embeddings=False, name=name)


# the one-layer models of tests/test_hip_stage_fp64_gpu.py (same names: one cache of weights serves both files) ...
TOY = llama("toy-d64", 256, 4, 2, 64, 512)
S1B = llama("1b-layer", 2048, 32, 8, 64, 8192, scaling=L3)
S1B_V = llama("1b-layer-fullvocab", 2048, 32, 8, 64, 8192, vocab=128256, scaling=L3)
S3B = llama("3b-layer", 3072, 24, 8, 128, 8192, scaling=L3)
S8B = llama("8b-layer", 4096, 32, 8, 128, 14336)
# ... and the smallest shape where every matrix takes the chunk pipeline up to 64 tokens (K >= 1024) and the one-step-per-batch
# chunked kernels above; the odd vocabulary leaves a zero second row in the last pair. MID_V: more than 32768 row pairs, so the
# head's work split has no K slices (ksplit = 1) and a wave owns 8 steps of a chunk: the small stand-in for a full vocabulary
MID = llama("mid-d1024", 1024, 8, 2, 128, 2048, vocab=515)
MID_V = llama("mid-d1024-v65539", 1024, 8, 2, 128, 2048, vocab=65539)
# two-layer models for the statistics a down-projection hands to the next layer's QKV launch
MID_2L = dataclasses.replace(MID, n_layers=2, name="mid-d1024-2l")
S1B_2L = dataclasses.replace(S1B, n_layers=2, name="1b-2l")
S3B_2L = dataclasses.replace(S3B, n_layers=2, name="3b-2l")

MODELS = {c.name: c for c in (TOY, S1B, S1B_V, S3B, S8B, MID, MID_V, MID_2L, S1B_2L, S3B_2L)}
# the shapes the project runs (specdec_hip.weights), for the closure of the case list
PRODUCTION = (W.LLAMA_3_2_1B, W.LLAMA_3_2_3B, W.LLAMA_3_8B, W.GPT2_SMALL, S1B_V)


class _Unbound:
    """an sd_model over placeholder addresses (sd_model_create only records them): the matrix table and the pass size"""

    def __init__(self, cfg: W.ModelConfig, wd: str):
        self.lib = _abi.load()
        self._buf = ctypes.create_string_buffer(64)
        p = ctypes.addressof(self._buf)
        self._layers = (_LayerWeights * cfg.n_layers)()
        for layer in self._layers:
            for f, _ in _LayerWeights._fields_:
                setattr(layer, f, p)
        mc = _ModelConfig(arch=cfg.arch, n_layers=cfg.n_layers, d_model=cfg.d_model, n_heads=cfg.n_heads, n_kv_heads=cfg.n_kv_heads,
                          head_dim=cfg.head_dim, d_ff=cfg.d_ff, vocab=cfg.vocab, max_pos=cfg.max_pos, norm_eps=cfg.norm_eps,
                          weight_dtype=_abi.SD_FP8_E4M3 if wd == "fp8" else _abi.SD_BF16, tok_emb=p, pos_emb=p, final_norm_w=p,
                          final_norm_b=p, lm_head=p, rope_cos=p, rope_sin=p, layers=self._layers, packed=p)
        self.handle = ctypes.c_void_p()
        self.created = self.lib.sd_model_create(ctypes.byref(mc), ctypes.byref(self.handle)) == 0

    def shapes(self):
        out = []
        for which in range(5):
            v = [ctypes.c_int(0) for _ in range(5)]
            _abi.check(self.lib.sd_model_matrix_shape(self.handle, which, *[ctypes.byref(x) for x in v]), "sd_model_matrix_shape")
            out.append(tuple(int(x.value) for x in v))
        return out

    def close(self):
        if self.created:
            self.lib.sd_model_destroy(self.handle)
            self.created = False


@functools.lru_cache(maxsize=None)
def _model_facts(name: str, wd: str, key: Tuple):
    """-> (created, pass_tokens, ((N, K, n_pairs, epi, prologue) x 5)); `key`: the geometry, so that a name is not trusted alone"""
    arch, d, hq, hkv, D, ff, vocab = key
    cfg = W.ModelConfig(arch=arch, n_layers=1, d_model=d, n_heads=hq, n_kv_heads=hkv, head_dim=D, d_ff=ff, vocab=vocab, name=name)
    m = _Unbound(cfg, wd)
    try:
        if not m.created:
            return (False, 0, ())
        return (True, int(m.lib.sd_model_pass_tokens(m.handle)), tuple(m.shapes()))
    finally:
        m.close()


def model_facts(cfg: W.ModelConfig, wd: str):
    return _model_facts(cfg.name, wd, (cfg.arch, cfg.d_model, cfg.n_heads, cfg.n_kv_heads, cfg.head_dim, cfg.d_ff, cfg.vocab))


def pass_plan(cfg: W.ModelConfig, wd: str, T: int, flags: int = 0):
    """the five instantiation names of a T-token pass of `cfg` (what HipModel.pass_plan returns for a bound model)"""
    created, _, shapes = model_facts(cfg, wd)
    assert created, (cfg.name, wd)
    return [gemm_plan(T, n_pairs, K, wd == "fp8", prologue, epi, flags) for (_, K, n_pairs, epi, prologue) in shapes]


@dataclasses.dataclass(frozen=True)
class Case:
    model: str                      # key of MODELS
    wd: str                         # "bf16" | "fp8"
    B: int                          # rows of the pass ...
    M: int                          # ... x tokens per row: T = B * M
    pos_base: Tuple[int, ...] = ()  # cached prefix length per row (default: 3 for the one row)
    row0: int = 0                   # first cache row of the pass
    page_len: Optional[int] = None  # paged KV
    flags: int = 0                  # PLAN_NO_DIRECT | PLAN_NO_PIPE: a case of the knob children
    two_layer: bool = False         # cross-layer statistics case

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
        s = f"{self.model}-{self.wd}-{self.B}x{self.M}"
        if self.row0:
            s += f"-row{self.row0}"
        if self.page_len:
            s += f"-page{self.page_len}"
        if self.flags:
            s += f"-flags{self.flags}"
        return s

    def names(self):
        return pass_plan(self.cfg, self.wd, self.T, self.flags)


def _one_row(model, wd, T, **kw):
    return Case(model, wd, 1, T, **kw)


def _ragged(B, seed):
    """B ragged prefix lengths around the attention's 32-key blocks, deterministic"""
    pool = [0, 1, 31, 32, 33, 63, 64, 65, 5, 17, 40, 95, 96, 2, 47, 70]
    return tuple(pool[(i * 7 + seed) % len(pool)] for i in range(B))


# ---- the GPU case list (flags = 0) ---------------------------------------------------------------------------------------------
# One row of T tokens. T leaves 6, 15, 15, 15, 0 padded token columns below 64 and 15, 0, 15, 0, 15, 0, 15, 0 above. Left out
# because the plan names the same five kernels as a neighbour that stays: T = 64 of the three large models (= T = 49; MID keeps
# it, and two batched cases are 63- and 64-token passes), T = 96 and 128 of the toy (= 65 and 97; MID keeps both).
GPU_CASES = (
    [_one_row("mid-d1024", wd, T) for wd in ("bf16", "fp8") for T in (10, 17, 33, 49, 64)]
    + [_one_row(m, wd, T) for m in ("1b-layer", "3b-layer", "8b-layer") for wd in ("bf16", "fp8") for T in (10, 17, 33, 49)]
    + [_one_row("toy-d64", wd, T) for wd in ("bf16", "fp8") for T in (10, 33, 65, 97)]
    + [_one_row("mid-d1024", "bf16", T) for T in (65, 80, 81, 96, 97, 112, 113, 128)]
    + [_one_row("mid-d1024-v65539", wd, T) for wd in ("bf16", "fp8") for T in (10, 17, 33, 49)]
    + [_one_row("1b-layer-fullvocab", "bf16", 17)]
)

# batched: B x M with ragged prefix lengths and row0 > 0 (the t -> (b, m) mapping of the QKV and ARGMAX epilogues); two on a
# paged cache. 2 x 8 and 16 x 3 are the 16- and 48-token sides of the 16 / 17 and 48 / 49 edges.
BATCHED_CASES = [
    Case("mid-d1024", "bf16", 16, 5, _ragged(16, 0), row0=1),
    Case("mid-d1024", "bf16", 14, 9, _ragged(14, 3), row0=2),
    Case("mid-d1024", "bf16", 3, 33, _ragged(3, 5), row0=1),
    Case("mid-d1024", "fp8", 9, 7, _ragged(9, 1), row0=3),
    Case("mid-d1024", "bf16", 2, 5, _ragged(2, 2), row0=1),
    Case("mid-d1024", "bf16", 2, 8, _ragged(2, 9), row0=2),
    Case("mid-d1024", "bf16", 16, 3, _ragged(16, 10), row0=1),
    Case("toy-d64", "bf16", 16, 5, _ragged(16, 4), row0=1, page_len=32),
    Case("1b-layer", "bf16", 9, 7, _ragged(9, 6), row0=2, page_len=32),
    Case("3b-layer", "fp8", 4, 16, _ragged(4, 7), row0=1),
]

TWO_LAYER_CASES = [
    Case("mid-d1024-2l", "bf16", 1, 33, (0,), two_layer=True),
    Case("1b-2l", "bf16", 1, 17, (0,), two_layer=True),
    Case("3b-2l", "fp8", 1, 64, (0,), two_layer=True),
]

# ---- the bodies only a knob reaches, run in child processes (one per flags value) ----------------------------------------------------
KNOB_CASES = (
    [_one_row(m, wd, T, flags=PLAN_NO_PIPE) for m in ("mid-d1024", "1b-layer", "8b-layer") for wd in ("bf16", "fp8") for T in (10, 17, 49)]
    + [_one_row(m, "bf16", 10, flags=PLAN_NO_DIRECT) for m in ("toy-d64", "mid-d1024")]
    + [_one_row("mid-d1024", "bf16", 10, flags=PLAN_NO_DIRECT | PLAN_NO_PIPE)]
    # what the closure (tests/test_gemm_plan_cpu.py) reported missing beyond those: the fp8 gate / up of the 1B at three token
    # groups, and a full-vocabulary fp8 head in the chunked body (16 steps of a 1024-column chunk per wave)
    + [_one_row("1b-layer", "fp8", 33, flags=PLAN_NO_PIPE)]
    + [_one_row("mid-d1024-v65539", "fp8", T, flags=PLAN_NO_PIPE) for T in (10, 49)]
)


def planned_names(cases):
    out = set()
    for c in cases:
        out.update(c.names())
    return out


def production_names(flags: int = 0, lo: int = 10):
    """every name a pass of lo..pass_tokens tokens of a model the project runs plans, bf16 and fp8 -> {name: (model, wd, T)}"""
    out = {}
    for cfg in PRODUCTION:
        for wd in ("bf16", "fp8"):
            created, pass_tokens, _ = model_facts(cfg, wd)
            if not created:
                continue
            for T in range(lo, pass_tokens + 1):
                for n in pass_plan(cfg, wd, T, flags):
                    out.setdefault(n, (cfg.name, wd, T))
    return out
