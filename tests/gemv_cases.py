"""The cases of tests/test_hip_gemv_instances_gpu.py, as data, with the host-only helpers that name their kernels.

A launch of 1..9 tokens (csrc/gemv.hip) runs one of three things: a fixed-geometry instance, an instantiation of the generic
kernel (EPI x whole / mask x token bound x storage x batch depth), or — rows too long to stage — a csrc/gemm_skinny.hip body.
`sd_gemv_instance` names it from the choice the launcher itself consumes. Every case below is one pass of a one-layer
`random_init` model; its `names` are the five instance names of that pass, so tests/test_gemv_instance_cpu.py can prove on a
machine without a GPU that the cases reach every kernel the models the project runs can reach at 1..9 tokens, and the GPU test
can refuse to run a case whose names have drifted.

Shaped like tests/gemm_body_cases.py, whose Case, models and helpers are reused. Nothing here touches a device."""

import contextlib
import dataclasses
import os

import gemm_body_cases as G
from specdec_hip import weights as W
from specdec_hip.ops import gemv_instance

SWITCH = "SPECDEC_GEMV_GENERIC"      # read by the library at every launch and every query

# the one-layer models of tests/test_hip_stage_fp64_gpu.py that gemm_body_cases.py does not have (same names and dimensions: one
# cache of weights serves the files; the GPU test checks that they are equal) ...
TOY128 = G.llama("toy-d128", 384, 3, 1, 128, 1024)          # K = 384: slices that are not whole 32-k steps, a MASK shape
GPT2 = W.ModelConfig(arch=W.ARCH_GPT2, n_layers=1, d_model=768, n_heads=12, n_kv_heads=12, head_dim=64, d_ff=3072, vocab=512,
                     max_pos=1024, tie_embeddings=False, name="gpt2-small-layer")
# ... and the "short-last" geometry of tests/test_hip_gemv_fixed_gpu.py: the LAST workgroup of the QKV, out and gate / up launches
# owns fewer pairs than the others while the class is still a fixed one; its down-projection (K = 8184) is a MASK shape
SHORT = G.llama("short-last-layer", 2816, 28, 7, 128, 8184)

MODELS = dict(G.MODELS)
MODELS.update({c.name: c for c in (TOY128, GPT2, SHORT)})


@contextlib.contextmanager
def switch(generic: bool):
    """the process environment with SPECDEC_GEMV_GENERIC set (generic) or absent, restored on exit"""
    old = os.environ.get(SWITCH)
    if generic:
        os.environ[SWITCH] = "1"
    else:
        os.environ.pop(SWITCH, None)
    try:
        yield
    finally:
        if old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = old


def pass_instances(cfg: W.ModelConfig, wd: str, T: int, generic: bool = False):
    """the five kernel names of a T-token launch-path pass of `cfg` (what HipModel.small_pass_instances returns for a bound
    model in a process whose switch is `generic`)"""
    created, _, shapes = G.model_facts(cfg, wd)
    assert created, (cfg.name, wd)
    with switch(generic):
        return [gemv_instance(T, n_pairs, K, wd == "fp8", prologue, epi) for (_, K, n_pairs, epi, prologue) in shapes]


@dataclasses.dataclass(frozen=True)
class Case(G.Case):
    generic: bool = False            # a switch case: runs (and is named) under SPECDEC_GEMV_GENERIC=1

    @property
    def cfg(self):
        return MODELS[self.model]

    @property
    def id(self):
        return G.Case.id.fget(self) + ("-generic" if self.generic else "")

    def names(self):
        return pass_instances(self.cfg, self.wd, self.T, self.generic)


def _one_row(model, wd, T, **kw):
    return Case(model, wd, 1, T, **kw)


# ---- one row of T tokens ---------------------------------------------------------------------------------------------------------
# T = 4 and 6 put one and three padded token columns under the tt5 and tt9 bounds, 5 and 9 fill them. 8B: the down-projection
# (K = 14336) is the generic MASK kernel up to 5 tokens and the `skinny:` hand-over at 6, 7, 8 and 9 (10 .. 7 padded columns of
# a 16-token group), next to three gemv.hip launches in the same pass.
# Left out because a neighbour that stays runs the same five names: of the full-vocabulary head (a 0.5 GB stream and a
# [T][128256] fp64 reference per case) T = 5 and 6 in bf16 (= 4 and 9) and T = 4 and 9 in fp8 (= 5 and 6): each dtype keeps a
# padded and a full case between them at both bounds; of toy-d64 in fp8 all but T = 1, 4 and 9 (its fp8 names are not ones a
# production shape plans). No full-vocabulary 3B / 8B head: ksplit = 1 and the deep batch at every K, the 1B head's names.
TOKENS = (1, 2, 3, 4, 5, 6, 9)
ONE_ROW_CASES = (
    [_one_row(m, wd, T) for m in ("1b-layer", "3b-layer") for wd in ("bf16", "fp8") for T in TOKENS]
    + [_one_row("8b-layer", wd, T) for wd in ("bf16", "fp8") for T in (1, 2, 3, 4, 5, 6, 7, 8, 9)]
    + [_one_row("1b-layer-fullvocab", "bf16", T) for T in (1, 2, 3, 4, 9)]
    + [_one_row("1b-layer-fullvocab", "fp8", T) for T in (1, 2, 3, 5, 6)]
    + [_one_row(m, "bf16", T) for m in ("gpt2-small-layer", "toy-d64", "toy-d128") for T in TOKENS]
    + [_one_row("toy-d64", "fp8", T) for T in (1, 4, 9)]
    + [_one_row("short-last-layer", "bf16", 5)]
)

# ---- batched: B rows x M tokens, B * M <= 9, ragged prefix lengths, row0 > 0 ------------------------------------------------------
# the t -> (row, position) map (m_magic) of the QKV and ARGMAX epilogues: on fixed instances (1B, 3B in bf16) and on the generic
# kernel (1B in fp8, the toy); two on a paged cache
_BM = ((2, 4), (3, 3), (4, 2), (9, 1), (2, 1))
BATCHED_CASES = (
    [Case(m, wd, B, M, G._ragged(B, 2 * i + j), row0=1 + (i + j) % 3)
     for j, (m, wd) in enumerate((("1b-layer", "bf16"), ("3b-layer", "bf16"), ("1b-layer", "fp8"), ("toy-d64", "bf16")))
     for i, (B, M) in enumerate(_BM)]
    + [Case("1b-layer", "bf16", 4, 2, G._ragged(4, 11), row0=2, page_len=32),
       Case("toy-d64", "bf16", 3, 3, G._ragged(3, 12), row0=1, page_len=32)]
)

# ---- the switch: the generic kernel at the shapes where it is the bitwise reference of the fixed instances ---------------------------
SWITCH_CASES = [_one_row(m, "bf16", T, generic=True) for m in ("1b-layer", "3b-layer", "8b-layer") for T in (1, 2, 3, 5, 9)]

GPU_CASES = ONE_ROW_CASES + BATCHED_CASES


def planned_names(cases):
    out = set()
    for c in cases:
        out.update(c.names())
    return out


def production_names(generic: bool = False):
    """every name a launch-path pass of 1..9 tokens of a model the project runs plans, bf16 and fp8 -> {name: (model, wd, T)}"""
    out = {}
    for cfg in G.PRODUCTION:
        for wd in ("bf16", "fp8"):
            if not G.model_facts(cfg, wd)[0]:        # GPT-2 has no fp8 storage (K = 768 is not whole 64-k steps per slice)
                continue
            for T in range(1, 10):
                for n in pass_instances(cfg, wd, T, generic):
                    out.setdefault(n, (cfg.name, wd, T))
    return out
