"""sd_gemm_plan on a machine without a GPU: the plan query itself, the closure of the GPU case list over every instantiation
the models the project runs can reach, and the choosers' edges.

The closure is the point. tests/test_hip_gemm_bodies_gpu.py checks kernels by name; a new body, threshold or template value
that its case list (tests/gemm_body_cases.py) does not reach fails here, before any GPU time is spent."""

import ctypes

import pytest

import gemm_body_cases as G
from specdec_hip import _abi
from specdec_hip import weights as W
from specdec_hip.ops import EPI_ARGMAX, EPI_QKV_ROPE, EPI_RESID, EPI_SWIGLU, PLAN_NO_DIRECT, PLAN_NO_PIPE, PRO_NONE, PRO_RMSNORM, gemm_plan


@pytest.fixture(autouse=True)
def _no_knobs(monkeypatch):
    """the library reads the two knobs once per process: this file's expectations are those of a process without them"""
    import os
    if "SPECDEC_NO_DIRECT" in os.environ or "SPECDEC_NO_PIPE" in os.environ:
        pytest.skip("SPECDEC_NO_DIRECT / SPECDEC_NO_PIPE are set in this process")
    monkeypatch.delenv("SPECDEC_MAX_PASS_TOKENS", raising=False)


# ---- the entry ---------------------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_additive():
    lib = _abi.load()
    for name in ("sd_gemm_plan", "sd_model_matrix_shape"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
    assert lib.sd_abi_version() == _abi.SD_ABI_VERSION == 1


def test_plan_names():
    assert gemm_plan(9, 1024, 2048, False, PRO_RMSNORM, EPI_QKV_ROPE) == "gemv"
    assert gemm_plan(1, 1024, 2048) == "gemv"
    assert gemm_plan(20, 8192, 2048, False, PRO_RMSNORM, EPI_SWIGLU) == "pipe<swiglu,tg2,bf16,sc4>"
    assert gemm_plan(80, 768, 1024, False, PRO_RMSNORM, EPI_QKV_ROPE) == "chunked<qkv,tg6,bf16,nb1>"
    assert gemm_plan(65, 256, 256, True, PRO_RMSNORM, EPI_QKV_ROPE) == "chunked<qkv,tg6,fp8,nb1>"
    assert gemm_plan(80, 768, 1024, True, PRO_RMSNORM, EPI_QKV_ROPE) == "none"      # fp8 chunk of 1024 columns x 80 rows: no LDS
    assert gemm_plan(40, 1024, 2048, False, PRO_NONE, EPI_RESID) == "slice<tg3>"
    assert gemm_plan(12, 1024, 2048, False, PRO_NONE, EPI_RESID) == "direct<tg1>"
    assert gemm_plan(12, 1024, 2048, False, PRO_NONE, EPI_RESID, PLAN_NO_DIRECT) == "pipe<resid,tg1,bf16,sc1>"
    assert gemm_plan(12, 1024, 2048, False, PRO_NONE, EPI_RESID, PLAN_NO_DIRECT | PLAN_NO_PIPE) == "chunked<resid,tg1,bf16,nb4>"
    # uncovered: K not in whole weight steps, more tokens than a launch takes, no rows
    assert gemm_plan(16, 384, 776) == "none"
    assert gemm_plan(129, 1024, 2048) == "none"
    assert gemm_plan(16, 0, 2048) == "none"
    assert gemm_plan(16, 1024, 2080, True) == "none"       # fp8: K in whole 64-k steps


def test_plan_refusals():
    lib = _abi.load()
    buf = ctypes.create_string_buffer(64)
    assert lib.sd_gemm_plan(16, 1024, 2048, 0, 0, 1, 0, None, 64) != 0 and "NULL out" in _abi.last_error()
    assert _abi.last_error().startswith("gemm_plan:")
    name = b"pipe<swiglu,tg2,bf16,sc4>"
    for cap in (0, 1, len(name)):         # the name needs its NUL
        buf.raw = b"\xaa" * 64
        assert lib.sd_gemm_plan(20, 8192, 2048, 0, 1, 2, 0, buf, cap) != 0 and "too short" in _abi.last_error()
        assert buf.raw == b"\xaa" * 64    # nothing written
    assert lib.sd_gemm_plan(20, 8192, 2048, 0, 1, 2, 0, buf, len(name) + 1) == 0 and buf.value == name
    assert lib.sd_gemm_plan(0, 1024, 2048, 0, 0, 1, 0, buf, 64) != 0 and "T=0" in _abi.last_error()
    for bad in ((16, 1024, 2048, 0, 3, 1, 0), (16, 1024, 2048, 0, 0, 5, 0), (16, 1024, 2048, 0, 0, -1, 0), (16, 1024, 2048, 0, 0, 1, 4)):
        assert lib.sd_gemm_plan(*bad, buf, 64) != 0 and "out of range" in _abi.last_error()
    v = [ctypes.c_int(0) for _ in range(5)]
    assert lib.sd_model_matrix_shape(None, 0, *[ctypes.byref(x) for x in v]) != 0 and "NULL" in _abi.last_error()


def test_matrix_shapes_of_a_model():
    """sd_model_matrix_shape against the shapes written out by hand for Llama-3.2-1B and GPT-2"""
    _, _, sh = G.model_facts(W.LLAMA_3_2_1B, "bf16")
    assert sh == ((3072, 2048, 1536, EPI_QKV_ROPE, 1), (2048, 2048, 1024, EPI_RESID, 0), (16384, 2048, 8192, EPI_SWIGLU, 1),
                  (2048, 8192, 1024, EPI_RESID, 0), (128256, 2048, 64128, EPI_ARGMAX, 1))
    _, _, sh = G.model_facts(W.GPT2_SMALL, "bf16")
    assert sh == ((2304, 768, 1152, EPI_QKV_ROPE, 2), (768, 768, 384, EPI_RESID, 0), (3072, 768, 1536, 3, 2),
                  (768, 3072, 384, EPI_RESID, 0), (50257, 768, 25129, EPI_ARGMAX, 2))


# ---- closure -----------------------------------------------------------------------------------------------------------------------
_GPU = G.GPU_CASES + G.BATCHED_CASES + G.TWO_LAYER_CASES


def test_case_ids_are_unique_and_cases_are_single_passes():
    ids = [c.id for c in _GPU + G.KNOB_CASES]
    assert len(ids) == len(set(ids))
    for c in _GPU + G.KNOB_CASES:
        created, pass_tokens, _ = G.model_facts(c.cfg, c.wd)
        assert created and 10 <= c.T <= pass_tokens, c.id
        assert len(c.bases) == c.B and "none" not in c.names() and "gemv" not in c.names(), c.id


def test_gpu_cases_reach_every_production_instantiation():
    """R: every name a pass of 10 .. pass_tokens tokens of Llama-3.2-1B / 3B, Llama-3-8B, GPT-2 small and the one-layer 1B with
    the full vocabulary plans, bf16 and fp8; C: the names of the GPU cases. R must be inside C."""
    R, C = G.production_names(0), G.planned_names(_GPU)
    missing = {n: w for n, w in R.items() if n not in C}
    assert not missing, f"planned by a production shape (first at model, dtype, T) but run by no GPU case: {missing}"
    assert len(R) >= 60           # the sweep really swept (63 when this was written)


@pytest.mark.parametrize("flags", [PLAN_NO_DIRECT, PLAN_NO_PIPE, PLAN_NO_DIRECT | PLAN_NO_PIPE])
def test_knob_cases_reach_every_production_instantiation(flags):
    """the same under each knob setting: what a production shape then plans is run by a knob case (in its own child process,
    under its own knobs) or already by a GPU case — a name is one kernel, whichever knobs led to it"""
    R, C = G.production_names(flags), G.planned_names(_GPU + G.KNOB_CASES)
    missing = {n: w for n, w in R.items() if n not in C}
    assert not missing, f"planned under flags={flags} (first at model, dtype, T) but run by no case: {missing}"
    assert any(c.flags == flags for c in G.KNOB_CASES)


def test_batched_and_edge_cases_are_present():
    batched = [c for c in _GPU if c.B > 1]
    assert len(batched) >= 8 and all(c.row0 > 0 and len(set(c.bases)) > 1 for c in batched)
    assert sum(1 for c in batched if c.page_len == 32) >= 2
    assert {(c.model, c.wd, c.T) for c in G.TWO_LAYER_CASES} == {("mid-d1024-2l", "bf16", 33), ("1b-2l", "bf16", 17), ("3b-2l", "fp8", 64)}
    Ts = {c.T for c in _GPU}
    assert {10, 16, 17, 48, 49, 64, 65, 80, 81, 96, 97, 112, 113, 128} <= Ts      # both sides of every token-count edge (9 is gemv.hip's)


# ---- the choosers' edges -------------------------------------------------------------------------------------------------------------
def _tg(name):
    return int(name.split("tg")[1].split(",")[0].rstrip(">"))


# (T, token groups of the instantiation): 16 tokens per group, 5 and 7 groups round up to the 6- and 8-group templates
TG_EDGES = [(10, 1), (16, 1), (17, 2), (48, 3), (49, 4), (64, 4), (65, 6), (80, 6), (81, 6), (96, 6), (97, 8), (112, 8), (113, 8), (128, 8)]


@pytest.mark.parametrize("T,tg", TG_EDGES)
def test_token_group_edges(T, tg):
    for cfg in (G.MID, G.TOY, G.S1B, G.S8B):
        names = G.pass_plan(cfg, "bf16", T)
        assert [_tg(n) for n in names] == [tg] * 5, (cfg.name, T, names)
        bodies = {n.split("<")[0] for n in names}
        if T > 64:
            assert bodies == {"chunked"}, (cfg.name, T, names)          # no other body takes more than 64 tokens


def test_body_edges_in_T():
    for cfg in (G.MID, G.S1B, G.S3B, G.S8B):
        shapes = G.model_facts(cfg, "bf16")[2]
        for which in (1, 3):                                              # out and down projections: plain residual
            _, K, n_pairs, epi, pro = shapes[which]
            body = lambda T, f=0: gemm_plan(T, n_pairs, K, False, pro, epi, f).split("<")[0]
            assert gemm_plan(9, n_pairs, K, False, pro, epi) == "gemv"
            assert [body(T) for T in (10, 16, 17, 48, 49, 64, 65)] == ["direct", "direct", "slice", "slice", "pipe", "pipe", "chunked"], cfg.name
            assert [body(T, PLAN_NO_DIRECT) for T in (10, 16, 17)] == ["pipe", "pipe", "slice"]
            assert [body(T, PLAN_NO_PIPE) for T in (16, 49, 64)] == ["direct", "chunked", "chunked"]
            assert body(16, PLAN_NO_DIRECT | PLAN_NO_PIPE) == "chunked"
            # the same matrix behind a norm, or in fp8, is never direct or slice
            assert gemm_plan(16, n_pairs, K, False, PRO_RMSNORM, epi).startswith("pipe<")
            assert gemm_plan(40, n_pairs, K, True, pro, epi).split("<")[0] in ("pipe", "chunked")


def test_pipe_needs_k_1024():
    """K = 992 / 1024: the pipeline's statistics segments need 1024 columns. Below: the chunked body where K splits into whole
    slices of weight steps (512 over 16 slices; 992 only without K slices, i.e. more than 32768 row pairs), else nothing"""
    assert gemm_plan(40, 512, 1024, False, PRO_RMSNORM, EPI_SWIGLU) == "pipe<swiglu,tg3,bf16,sc1>"
    assert gemm_plan(40, 512, 992, False, PRO_RMSNORM, EPI_SWIGLU) == "none"
    assert gemm_plan(40, 512, 512, False, PRO_RMSNORM, EPI_SWIGLU) == "chunked<swiglu,tg3,bf16,nb2>"
    assert gemm_plan(40, 40000, 1024, False, PRO_RMSNORM, EPI_ARGMAX) == "pipe<argmax,tg3,bf16,sc8>"
    assert gemm_plan(40, 40000, 992, False, PRO_RMSNORM, EPI_ARGMAX) == "chunked<argmax,tg3,bf16,nb1>"


def test_full_vocabulary_head_has_no_k_slices():
    """more than 32768 row pairs: ksplit = 1, a wave owns 8 steps of a 256-column chunk"""
    for vocab, K in ((128256, 2048), (128256, 4096), (65539, 1024)):
        for T, tg in ((10, 1), (17, 2), (33, 3), (64, 4)):
            assert gemm_plan(T, (vocab + 1) // 2, K, False, PRO_RMSNORM, EPI_ARGMAX) == f"pipe<argmax,tg{tg},bf16,sc8>"


@pytest.mark.parametrize("cfg", list(G.PRODUCTION) + [G.TOY, G.MID, G.MID_V, G.S3B, G.S8B], ids=lambda c: c.name)
@pytest.mark.parametrize("wd", ["bf16", "fp8"])
def test_pass_tokens_is_what_the_plan_covers(cfg, wd):
    """sd_model_pass_tokens = the largest pass size (128, 64, 32 or 16) at which the plan names a kernel for all five matrices;
    every smaller T is then covered too, and the next pass size is not. 9 or fewer: gemv.hip's rows, no multi-token pass."""
    created, pass_tokens, _ = G.model_facts(cfg, wd)
    if not created:       # sd_model_create refuses fp8 storage where a matrix does not split into whole 64-k steps: GPT-2's K = 768
        assert (cfg.name, wd) == ("gpt2", "fp8")
        return
    covered = [T for T in range(10, 129) if "none" not in G.pass_plan(cfg, wd, T)]
    if pass_tokens <= 9:
        assert not any(T in covered for T in (16, 32, 64, 128)), (pass_tokens, covered)
        return
    assert pass_tokens in (16, 32, 64, 128)
    assert set(range(10, pass_tokens + 1)) <= set(covered)
    assert pass_tokens == 128 or 2 * pass_tokens not in covered


# ---- m_magic ---------------------------------------------------------------------------------------------------------------------
def test_m_magic_divides_exactly():
    """gemv_derive: t / M == (t * ceil(65536 / M)) >> 16 for every M in 1..128 and t < 512 (the QKV and ARGMAX epilogues map a
    token column t to (row b, position m) with it; padded columns reach t = 127)"""
    for M in range(1, 129):
        magic = (65536 + M - 1) // M
        assert magic < 1 << 17
        for t in range(512):
            assert (t * magic) >> 16 == t // M, (M, t)
