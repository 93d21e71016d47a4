"""sd_gemv_instance on a machine without a GPU: the query itself, hand-written expectations at the choosers' edges, and the
closure of the GPU case list (tests/gemv_cases.py) over every kernel a pass of 1..9 tokens of the models the project runs
can reach.

The closure is the point. tests/test_hip_gemv_instances_gpu.py checks kernels by name against fp64; a new fixed class, token
bound, batch depth or hand-over that its case list does not reach fails here, before any GPU time is spent."""

import ctypes

import pytest

import gemm_body_cases as G
import gemv_cases as V
from specdec_hip import _abi
from specdec_hip import weights as W
from specdec_hip.ops import (EPI_ARGMAX, EPI_GELU, EPI_QKV_ROPE, EPI_RESID, EPI_SWIGLU, PRO_LAYERNORM, PRO_NONE, PRO_RMSNORM,
                             gemm_plan, gemv_instance, gemv_variant)
from test_gemv_variant_cpu import MODELS, layer_matrices


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    """the expectations are those of a process without the switch and without the multi-token knobs (the `skinny:` names are
    gemm_plan's, which reads its knobs once per process)"""
    import os
    if "SPECDEC_NO_DIRECT" in os.environ or "SPECDEC_NO_PIPE" in os.environ:
        pytest.skip("SPECDEC_NO_DIRECT / SPECDEC_NO_PIPE are set in this process")
    monkeypatch.delenv(V.SWITCH, raising=False)
    monkeypatch.delenv("SPECDEC_MAX_PASS_TOKENS", raising=False)


# ---- the entry ---------------------------------------------------------------------------------------------------------------------
def test_symbol_is_exported_and_additive():
    lib = _abi.load()
    assert "sd_gemv_instance" in _abi.SIGNATURES and hasattr(lib, "sd_gemv_instance")
    assert _abi.SIGNATURES["sd_gemv_instance"] == _abi.SIGNATURES["sd_gemv_variant"]
    assert lib.sd_abi_version() == _abi.SD_ABI_VERSION == 1
    # the two older queries keep their answers: they name the launcher that is asked
    assert gemm_plan(9, 2048, 14336, False, PRO_NONE, EPI_RESID) == "gemv"
    assert gemv_variant(9, 2048, 14336, False, PRO_NONE, EPI_RESID) == "generic"


def test_refusals_in_form():
    lib = _abi.load()
    buf = ctypes.create_string_buffer(64)
    assert lib.sd_gemv_instance(5, 1536, 3072, 0, 0, 1, None, 64) != 0 and "NULL out" in _abi.last_error()
    assert _abi.last_error().startswith("gemv_instance:")
    name = b"fixed<resid,ks16,tp6,none,tt5,kb6>"
    for cap in (0, 1, len(name)):         # the name needs its NUL
        buf.raw = b"\xaa" * 64
        assert lib.sd_gemv_instance(5, 1536, 3072, 0, 0, 1, buf, cap) != 0 and "too short" in _abi.last_error()
        assert buf.raw == b"\xaa" * 64    # nothing written
    assert lib.sd_gemv_instance(5, 1536, 3072, 0, 0, 1, buf, len(name) + 1) == 0 and buf.value == name


@pytest.mark.parametrize("bad", [dict(T=0), dict(T=10), dict(prologue=3), dict(prologue=-1), dict(epi=5), dict(epi=-1), dict(n_pairs=0),
                                 dict(K=0), dict(K=3076)])
def test_refuses_what_the_variant_query_refuses(bad):
    args = dict(T=5, n_pairs=1536, K=3072, w8=False, prologue=PRO_NONE, epi=EPI_RESID)
    args.update(bad)
    with pytest.raises(_abi.HipLibraryError):
        gemv_variant(**args)
    with pytest.raises(_abi.HipLibraryError):
        gemv_instance(**args)


def test_refuses_what_the_launcher_refuses():
    """launch_gemv's own refusals, in its words: fp8 storage whose K slices are not whole 64-k steps (the 384-wide toy, GPT-2),
    and rows that fit neither the LDS nor a multi-token chunk (K = 14344: 6 rows do not fit, and no body has a chunk for it)"""
    with pytest.raises(_abi.HipLibraryError, match="whole 64-k steps"):
        gemv_instance(2, 256, 384, True, PRO_RMSNORM, EPI_QKV_ROPE)
    with pytest.raises(_abi.HipLibraryError, match="whole 64-k steps"):
        gemv_instance(2, 1152, 768, True, PRO_LAYERNORM, EPI_QKV_ROPE)
    assert gemv_instance(5, 2048, 14344, False, PRO_NONE, EPI_RESID) == "generic<resid,mask,tt9,bf16,kb12>"
    assert gemm_plan(16, 2048, 14344, False, PRO_NONE, EPI_RESID) == "none"
    with pytest.raises(_abi.HipLibraryError, match="does not fit LDS"):
        gemv_instance(6, 2048, 14344, False, PRO_NONE, EPI_RESID)
    assert gemv_variant(6, 2048, 14344, False, PRO_NONE, EPI_RESID) == "generic"       # the older query names the launcher it asked


_SHAPES = [(n, K, pro, epi) for c in MODELS.values() for _, n, K, pro, epi in layer_matrices(c)] + [
    (64128, 2048, PRO_RMSNORM, EPI_ARGMAX), (25129, 768, PRO_LAYERNORM, EPI_ARGMAX), (1152, 768, PRO_LAYERNORM, EPI_QKV_ROPE),
    (1536, 768, PRO_LAYERNORM, EPI_GELU), (384, 3072, PRO_NONE, EPI_RESID), (96, 256, PRO_RMSNORM, EPI_QKV_ROPE), (1536, 3080, PRO_NONE, EPI_RESID),
    (8184, 2816, PRO_RMSNORM, EPI_SWIGLU), (1408, 8184, PRO_NONE, EPI_RESID)]


@pytest.mark.parametrize("generic", [False, True])
def test_agrees_with_the_variant_query(generic):
    """fixed<...> wherever sd_gemv_variant says so, the very string; generic<...> or skinny:... wherever it says "generic" """
    n_fixed = n_other = 0
    with V.switch(generic):
        for n_pairs, K, pro, epi in _SHAPES:
            for w8 in (False, True):
                for T in range(1, 10):
                    v = gemv_variant(T, n_pairs, K, w8, pro, epi)
                    try:
                        i = gemv_instance(T, n_pairs, K, w8, pro, epi)
                    except _abi.HipLibraryError:
                        assert v == "generic" and w8, (T, n_pairs, K, w8)      # a launch the launcher refuses
                        continue
                    if v.startswith("fixed<"):
                        assert i == v
                        n_fixed += 1
                    else:
                        assert v == "generic" and (i.startswith("generic<") or i.startswith("skinny:")), (T, n_pairs, K, w8, v, i)
                        n_other += 1
    assert n_other > 0 and (n_fixed > 0) != generic


# ---- hand-written expectations -----------------------------------------------------------------------------------------------------
def test_the_3b_verify_pass():
    got = [gemv_instance(5, n, K, False, pro, epi) for _, n, K, pro, epi in layer_matrices(W.LLAMA_3_2_3B)]
    assert got == ["fixed<qkv,ks8,tp5,rmsnorm,tt5,kb6>", "fixed<resid,ks16,tp6,none,tt5,kb6>",
                   "fixed<swiglu,ks4,tp8,rmsnorm,tt5,kb12>", "fixed<resid,ks16,tp6,none,tt5,kb12>"]
    with V.switch(True):
        got = [gemv_instance(5, n, K, False, pro, epi) for _, n, K, pro, epi in layer_matrices(W.LLAMA_3_2_3B)]
    assert got == ["generic<qkv,whole,tt5,bf16,kb6>", "generic<resid,whole,tt5,bf16,kb6>",
                   "generic<swiglu,whole,tt5,bf16,kb12>", "generic<resid,whole,tt5,bf16,kb12>"]


@pytest.mark.parametrize("generic", [False, True])
def test_8b_down_projection_hands_over_past_what_the_lds_stages(generic):
    """K = 14336: the MASK variant of the generic kernel while T rows fit the LDS, a gemm_skinny.hip body above — on both sides of
    the switch, which only chooses between gemv.hip's two families. The boundary is gemv_max_tokens(14336)."""
    with V.switch(generic):
        names = {T: gemv_instance(T, 2048, 14336, False, PRO_NONE, EPI_RESID) for T in range(1, 10)}
        names8 = {T: gemv_instance(T, 2048, 14336, True, PRO_NONE, EPI_RESID) for T in range(1, 10)}
    # gemv_max_tokens by hand: T bf16 rows of K + 8 (padding) elements, the partials aliased onto them, and 4 * (9 * 16 * 2 + 64)
    # bytes of norm sums must fit the CU's 160 KiB
    edge = max(T for T in range(1, 10) if T * (14336 + 8) * 2 + 1408 <= 160 * 1024)
    assert edge == 5
    # ... and gemv_max_tokens itself, as sd_model_create records it: a model whose other matrices no multi-token body covers
    # (the 384-wide toy's) takes passes of gemv_max_tokens(its widest row) tokens and no more
    assert G.model_facts(G.llama("toy-d128-ff14336", 384, 3, 1, 128, 14336), "bf16")[:2] == (True, edge)
    assert all(names[T] == "generic<resid,mask,tt9,bf16,kb12>" for T in range(1, edge + 1)), names
    assert all(names[T] == "skinny:direct<tg1>" for T in range(edge + 1, 10)), names
    assert all(names8[T] == "generic<resid,mask,tt9,fp8,kb6>" for T in range(1, edge + 1)), names8
    assert all(names8[T] == "skinny:chunked<resid,tg1,fp8,nb2>" for T in range(edge + 1, 10)), names8


def _field(name, i):
    return name[name.index("<") + 1:-1].split(",")[i]


@pytest.mark.parametrize("generic", [False, True])
def test_token_bound_edges(generic):
    """tt: 1 | 2 | 3 | 4-5 | 6-9, in both families; a MASK instantiation is tt9 at every T"""
    want = {1: "tt1", 2: "tt2", 3: "tt3", 4: "tt5", 5: "tt5", 6: "tt9", 7: "tt9", 8: "tt9", 9: "tt9"}
    with V.switch(generic):
        for T, tt in want.items():
            for _, n, K, pro, epi in layer_matrices(W.LLAMA_3_2_1B):
                assert _field(gemv_instance(T, n, K, False, pro, epi), 2 if generic else 4) == tt
                assert _field(gemv_instance(T, n, K, True, pro, epi), 2) == tt
            assert gemv_instance(T, 64128, 2048, False, PRO_RMSNORM, EPI_ARGMAX) == f"generic<argmax,whole,{tt},bf16,kb12>"
            assert gemv_instance(T, 1152, 768, False, PRO_LAYERNORM, EPI_QKV_ROPE) == "generic<qkv,mask,tt9,bf16,kb6>"
            assert gemv_instance(T, 1536, 3080, False, PRO_NONE, EPI_RESID) == "generic<resid,mask,tt9,bf16,kb6>"      # 16 slices of 224: 7 loads


def test_batch_depth_edges():
    """kb: 12 from kDeepSteps = 24 loads per wave over the K slice, from kDeepStepsVerify = 16 at 3 tokens and more (an fp8 load
    covers 64 k). 1B out (K = 2048 over 16 slices: 4 loads), down (8192: 16) and gate / up (2048 over 4: 16); 3B gate / up (3072
    over 4: 24); 8B qkv (4096 over 8: 16)."""
    kb = lambda *a: _field(gemv_instance(*a), -1)
    assert [kb(T, 1024, 2048, False, PRO_NONE, EPI_RESID) for T in (2, 3)] == ["kb6", "kb6"]
    assert [kb(T, 1024, 8192, False, PRO_NONE, EPI_RESID) for T in (2, 3)] == ["kb6", "kb12"]        # 16 loads: deep from 3 tokens
    assert [kb(T, 8192, 2048, False, PRO_RMSNORM, EPI_SWIGLU) for T in (2, 3)] == ["kb6", "kb12"]
    assert [kb(T, 8192, 3072, False, PRO_RMSNORM, EPI_SWIGLU) for T in (1, 2, 3)] == ["kb12"] * 3      # 24 loads: deep at every T
    assert [kb(T, 3072, 4096, False, PRO_RMSNORM, EPI_QKV_ROPE) for T in (2, 3)] == ["kb6", "kb12"]
    assert [kb(T, 1024, 8192, True, PRO_NONE, EPI_RESID) for T in (2, 3, 9)] == ["kb6"] * 3            # fp8: 8 loads
    assert [kb(T, 8192, 3072, True, PRO_RMSNORM, EPI_SWIGLU) for T in (2, 3)] == ["kb6", "kb6"]          # fp8: 12 loads
    assert [kb(T, 14336, 4096, True, PRO_RMSNORM, EPI_SWIGLU) for T in (2, 3)] == ["kb12", "kb12"]       # 8B gate / up, 2 slices: 32 loads
    with V.switch(True):
        assert [kb(T, 1024, 8192, False, PRO_NONE, EPI_RESID) for T in (2, 3)] == ["kb6", "kb12"]    # the same edge in the generic kernel


# ---- closure -----------------------------------------------------------------------------------------------------------------------
_ALL = V.GPU_CASES + V.SWITCH_CASES


def test_case_ids_are_unique_and_cases_are_single_small_passes():
    ids = [c.id for c in _ALL]
    assert len(ids) == len(set(ids))
    for c in _ALL:
        created, pass_tokens, _ = G.model_facts(c.cfg, c.wd)
        assert created and 1 <= c.T <= 9 and c.T <= max(pass_tokens, 9), c.id
        names = c.names()
        assert len(c.bases) == c.B and len(names) == 5, c.id
        assert all(n.startswith(("fixed<", "generic<", "skinny:")) and not n.endswith("none") for n in names), (c.id, names)
    assert all(c.generic for c in V.SWITCH_CASES) and not any(c.generic for c in V.GPU_CASES)
    assert not any(n.startswith("fixed<") for c in V.SWITCH_CASES for n in c.names())


def test_gpu_cases_reach_every_production_instantiation():
    """R: every name a pass of 1..9 tokens of Llama-3.2-1B / 3B, Llama-3-8B, GPT-2 small and the one-layer 1B with the full
    vocabulary runs, bf16 and fp8; C: the names of the GPU cases. R must be inside C."""
    R, C = V.production_names(False), V.planned_names(V.GPU_CASES)
    missing = {n: w for n, w in R.items() if n not in C}
    assert not missing, f"run by a production shape (first at model, dtype, T) but by no GPU case: {missing}"
    assert len(R) >= 90           # the sweep really swept (90 when this was written: 48 fixed, 40 generic, 2 skinny)


def test_switch_cases_reach_every_production_instantiation_under_the_switch():
    """the same with SPECDEC_GEMV_GENERIC set: what a production shape then runs is run by a switch case or already by a GPU
    case — a name is one kernel, whichever setting led to it"""
    R, C = V.production_names(True), V.planned_names(_ALL)
    missing = {n: w for n, w in R.items() if n not in C}
    assert not missing, f"run under the switch (first at model, dtype, T) but by no case: {missing}"
    assert len(R) >= 60 and not any(n.startswith("fixed<") for n in R)         # (60 when this was written)


def test_batched_paged_and_hand_over_cases_are_present():
    batched = [c for c in V.GPU_CASES if c.B > 1]
    assert len(batched) >= 8 and all(c.row0 > 0 and len(set(c.bases)) > 1 and c.T <= 9 for c in batched)
    assert sum(1 for c in batched if c.page_len == 32) >= 2
    assert {(c.B, c.M) for c in batched} >= {(2, 4), (3, 3), (4, 2), (9, 1), (2, 1)}
    # batched passes on fixed instances and on the generic kernel
    assert any(all(n.startswith("fixed<") for n in c.names()[:4]) for c in batched)
    assert any(all(n.startswith("generic<") for n in c.names()) for c in batched)
    # every 8B pass of 6..9 tokens: exactly one hand-over (the down-projection), bf16 and fp8, next to gemv.hip launches
    big = [c for c in _ALL if c.model == "8b-layer" and c.T >= 6]
    assert {(c.wd, c.T) for c in big if not c.generic} == {(wd, T) for wd in ("bf16", "fp8") for T in (6, 7, 8, 9)}
    for c in big:
        names = c.names()
        assert [n.startswith("skinny:") for n in names] == [False, False, False, True, False], (c.id, names)
    assert not any(n.startswith("skinny:") for c in _ALL if not (c.model == "8b-layer" and c.T >= 6) for n in c.names())
    Ts = {(c.model, c.wd, c.T) for c in V.ONE_ROW_CASES}
    for m in ("1b-layer", "3b-layer", "8b-layer"):
        assert {(m, wd, T) for wd in ("bf16", "fp8") for T in (1, 2, 3, 4, 5, 6, 9)} <= Ts         # padded and full under tt5 and tt9
    assert ("short-last-layer", "bf16", 5) in Ts and ("toy-d128", "bf16", 4) in Ts and ("gpt2-small-layer", "bf16", 6) in Ts
