"""sd_gemv_variant on a machine without a GPU: which csrc/gemv.hip instance a launch of T <= 9 tokens takes.

The fixed-geometry instances exist for the bf16 layer matrices of Llama models at 1B / 3B / 8B dimensions; everything else runs
the generic kernel. The query and launch_gemv ask the same function, so what is named here is what a forward runs
(tests/test_hip_gemv_fixed_gpu.py compares the two paths bit for bit).

The one layer matrix of the three models that is NOT served by a fixed instance is the 8B down-projection: its K = 14336 is
beyond the one-chunk-per-thread staging (K / 8 > 1024 threads), i.e. a MASK shape, and MASK shapes stay generic."""

import pytest

from specdec_hip import _abi
from specdec_hip import weights as W
from specdec_hip.ops import (EPI_ARGMAX, EPI_GELU, EPI_QKV_ROPE, EPI_RESID, EPI_SWIGLU, PRO_LAYERNORM, PRO_NONE, PRO_RMSNORM,
                             gemm_plan, gemv_variant)

TOKENS = (1, 2, 3, 5, 9)
MODELS = {"1b": W.LLAMA_3_2_1B, "3b": W.LLAMA_3_2_3B, "8b": W.LLAMA_3_8B}


def layer_matrices(c):
    """(name, n_pairs, K, prologue, epilogue) of the four layer matrices, the numbers sd_model_matrix_shape gives"""
    hq_d = c.n_heads * c.head_dim
    return [("qkv", (c.n_heads + 2 * c.n_kv_heads) * c.head_dim // 2, c.d_model, PRO_RMSNORM, EPI_QKV_ROPE),
            ("out", c.d_model // 2, hq_d, PRO_NONE, EPI_RESID),
            ("gate_up", c.d_ff, c.d_model, PRO_RMSNORM, EPI_SWIGLU),
            ("down", c.d_model // 2, c.d_ff, PRO_NONE, EPI_RESID)]


@pytest.fixture(autouse=True)
def _no_switch(monkeypatch):
    monkeypatch.delenv("SPECDEC_GEMV_GENERIC", raising=False)


def test_symbol_is_exported_and_additive():
    lib = _abi.load()
    assert "sd_gemv_variant" in _abi.SIGNATURES and hasattr(lib, "sd_gemv_variant")
    assert lib.sd_abi_version() == _abi.SD_ABI_VERSION == 1
    assert gemm_plan(5, 2560, 3072, False, PRO_RMSNORM, EPI_QKV_ROPE) == "gemv"     # the plan query keeps its answer


@pytest.mark.parametrize("model", list(MODELS))
@pytest.mark.parametrize("T", TOKENS)
def test_layer_matrices_take_fixed_instances(model, T):
    tt = {1: 1, 2: 2, 3: 3, 5: 5, 9: 9}[T]
    for name, n_pairs, K, pro, epi in layer_matrices(MODELS[model]):
        got = gemv_variant(T, n_pairs, K, False, pro, epi)
        if K // 8 > 1024:      # 8B down: MASK shape
            assert (model, name) == ("8b", "down") and got == "generic"
            continue
        assert got.startswith("fixed<") and got.endswith(">"), (model, name, T, got)
        fields = got[len("fixed<"):-1].split(",")
        assert fields[0] == {EPI_QKV_ROPE: "qkv", EPI_RESID: "resid", EPI_SWIGLU: "swiglu"}[epi]
        assert fields[3] == ("rmsnorm" if pro == PRO_RMSNORM else "none") and fields[4] == f"tt{tt}", (model, name, T, got)


def test_named_geometry_is_the_work_split():
    """the 3B verify pass (5 tokens): K slices x pairs per tile of the four launches, and the batch depth"""
    got = [gemv_variant(5, n, K, False, pro, epi) for _, n, K, pro, epi in layer_matrices(W.LLAMA_3_2_3B)]
    assert got == ["fixed<qkv,ks8,tp5,rmsnorm,tt5,kb6>", "fixed<resid,ks16,tp6,none,tt5,kb6>",
                   "fixed<swiglu,ks4,tp8,rmsnorm,tt5,kb12>", "fixed<resid,ks16,tp6,none,tt5,kb12>"]
    assert gemv_variant(4, 2560, 3072, False, PRO_RMSNORM, EPI_QKV_ROPE) == "fixed<qkv,ks8,tp5,rmsnorm,tt5,kb6>"   # 4 tokens: the 5-token bound
    # a last workgroup with fewer pairs is still the same class
    assert gemv_variant(5, 8184, 2816, False, PRO_RMSNORM, EPI_SWIGLU) == "fixed<swiglu,ks4,tp8,rmsnorm,tt5,kb12>"


@pytest.mark.parametrize("T", TOKENS)
def test_everything_else_is_generic(T):
    for c in MODELS.values():
        assert gemv_variant(T, c.vocab // 2, c.d_model, False, PRO_RMSNORM, EPI_ARGMAX) == "generic"      # lm_head, a (batched) Medusa head
        for _, n_pairs, K, pro, epi in layer_matrices(c):
            assert gemv_variant(T, n_pairs, K, True, pro, epi) == "generic"                              # fp8
    assert gemv_variant(T, 2048, 14336, False, PRO_NONE, EPI_RESID) == "generic"          # MASK: rows longer than the register staging
    assert gemv_variant(T, 1536, 3080, False, PRO_NONE, EPI_RESID) == "generic"           # MASK: slices that are not whole 32-k steps
    g = W.GPT2_SMALL
    assert gemv_variant(T, 3 * g.d_model // 2, g.d_model, False, PRO_LAYERNORM, EPI_QKV_ROPE) == "generic"
    assert gemv_variant(T, g.d_ff // 2, g.d_model, False, PRO_LAYERNORM, EPI_GELU) == "generic"
    assert gemv_variant(T, 96, 256, False, PRO_RMSNORM, EPI_QKV_ROPE) == "generic"        # a toy model: another work split


def test_the_switch_forces_generic(monkeypatch):
    assert gemv_variant(5, 1536, 3072).startswith("fixed<")
    monkeypatch.setenv("SPECDEC_GEMV_GENERIC", "1")       # read at every call, as at every launch
    assert gemv_variant(5, 1536, 3072) == "generic"
    monkeypatch.delenv("SPECDEC_GEMV_GENERIC")
    assert gemv_variant(5, 1536, 3072).startswith("fixed<")


@pytest.mark.parametrize("bad", [dict(T=0), dict(prologue=3), dict(prologue=-1), dict(epi=5), dict(epi=-1)])
def test_refuses_what_the_plan_query_refuses(bad):
    args = dict(T=5, n_pairs=1536, K=3072, w8=False, prologue=PRO_NONE, epi=EPI_RESID)
    args.update(bad)
    with pytest.raises(_abi.HipLibraryError):
        gemm_plan(**args)
    with pytest.raises(_abi.HipLibraryError):
        gemv_variant(**args)


def test_refuses_what_is_no_gemv_launch():
    for bad in (dict(T=10), dict(n_pairs=0), dict(K=0), dict(K=3076)):
        args = dict(T=5, n_pairs=1536, K=3072)
        args.update(bad)
        with pytest.raises(_abi.HipLibraryError):
            gemv_variant(**args)
