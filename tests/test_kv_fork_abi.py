"""sd_model_kv_fork / sd_model_kv_copy_pages through the C-ABI on a host without a GPU: both symbols are exported and bound, and
the refusals are returned with a message before any device work. Binding a cache needs a device, so the refusals that compare an
index with the bound geometry (a row >= B, n_pos > Lmax or page_len, a page >= n_pages, the dense entry on a paged model and the
reverse) are asserted on bound models in tests/test_hip_kv_fork_gpu.py; everything a NULL or unbound model can show is here."""

import ctypes

import pytest

from specdec_hip import _abi
from specdec_hip.engine import _LayerWeights, _ModelConfig


def _unbound_model():
    """an sd_model over placeholder addresses, never bound (sd_model_create only records them)"""
    lib = _abi.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    layers = (_LayerWeights * 1)()
    for f, _ in _LayerWeights._fields_:
        setattr(layers[0], f, p)
    mc = _ModelConfig(arch=0, n_layers=1, d_model=128, n_heads=2, n_kv_heads=1, head_dim=64, d_ff=256, vocab=1000, max_pos=512,
                      norm_eps=1e-5, weight_dtype=_abi.SD_BF16, tok_emb=p, pos_emb=None, final_norm_w=p, final_norm_b=None, lm_head=p,
                      rope_cos=p, rope_sin=p, layers=layers, packed=None)
    h = ctypes.c_void_p()
    _abi.check(lib.sd_model_create(ctypes.byref(mc), ctypes.byref(h)), "sd_model_create")
    return lib, h, (buf, layers)


def _i32(*xs):
    return (ctypes.c_int32 * len(xs))(*xs)


def test_both_symbols_are_exported_and_bound():
    lib = _abi.load()
    for name in ("sd_model_kv_fork", "sd_model_kv_copy_pages"):
        assert name in _abi.SIGNATURES and hasattr(lib, name)
        assert getattr(lib, name).argtypes == _abi.SIGNATURES[name][1]
    assert lib.sd_abi_version() == _abi.SD_ABI_VERSION == 1      # additive: the version stays


# (src_row, dst_rows, n_dst, n_pos) -> message; the model is NULL: these are refused on the arguments alone
FORK_CASES = {
    "null_list": ((0, None, 2, 4), "NULL dst_rows"),
    "negative_count": ((0, _i32(1), -1, 4), "n_dst=-1"),
    "negative_n_pos": ((0, _i32(1), 1, -1), "n_pos=-1"),
    "negative_src": ((-1, _i32(1), 1, 4), "src_row -1"),
    "negative_dst": ((0, _i32(1, -2), 2, 4), "destination row -2"),
    "dst_is_src": ((1, _i32(0, 1), 2, 4), "is the source row"),
    "null_model": ((0, _i32(1), 1, 4), "NULL model"),
    "null_model_empty": ((0, None, 0, 0), "NULL model"),
}


@pytest.mark.parametrize("case", sorted(FORK_CASES))
def test_kv_fork_refusals(case):
    (src, dsts, n, n_pos), msg = FORK_CASES[case]
    rc = _abi.load().sd_model_kv_fork(None, src, dsts, n, n_pos, None)
    assert rc != 0
    assert msg in _abi.last_error() and _abi.last_error().startswith("kv_fork:"), _abi.last_error()


PAGE_CASES = {
    "null_src_list": ((None, _i32(1), 1, 4), "NULL page list"),
    "null_dst_list": ((_i32(1), None, 1, 4), "NULL page list"),
    "negative_count": ((_i32(0), _i32(1), -3, 4), "n_pairs=-3"),
    "negative_n_pos": ((_i32(0), _i32(1), 1, -5), "n_pos=-5"),
    "negative_src_page": ((_i32(-1), _i32(1), 1, 4), "negative page index"),
    "negative_dst_page": ((_i32(0, 2), _i32(1, -1), 2, 4), "negative page index"),
    "page_onto_itself": ((_i32(0, 3), _i32(1, 3), 2, 4), "page 3 onto itself"),
    "null_model": ((_i32(0), _i32(1), 1, 4), "NULL model"),
}


@pytest.mark.parametrize("case", sorted(PAGE_CASES))
def test_kv_copy_pages_refusals(case):
    (src, dst, n, n_pos), msg = PAGE_CASES[case]
    rc = _abi.load().sd_model_kv_copy_pages(None, src, dst, n, n_pos, None)
    assert rc != 0
    assert msg in _abi.last_error() and _abi.last_error().startswith("kv_copy_pages:"), _abi.last_error()


def test_unbound_model_is_refused_by_both():
    lib, h, keep = _unbound_model()
    try:
        assert lib.sd_model_kv_fork(h, 0, _i32(1), 1, 4, None) != 0
        assert "not bound" in _abi.last_error() and _abi.last_error().startswith("kv_fork:")
        assert lib.sd_model_kv_copy_pages(h, _i32(0), _i32(1), 1, 4, None) != 0
        assert "not bound" in _abi.last_error() and _abi.last_error().startswith("kv_copy_pages:")
        # even the calls that would launch nothing need a bound model
        assert lib.sd_model_kv_fork(h, 0, None, 0, 0, None) != 0 and "not bound" in _abi.last_error()
        assert lib.sd_model_kv_copy_pages(h, None, None, 0, 0, None) != 0 and "not bound" in _abi.last_error()
    finally:
        lib.sd_model_destroy(h)
