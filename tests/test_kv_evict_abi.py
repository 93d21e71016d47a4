"""sd_model_kv_evict through the C-ABI on a host without a GPU: the symbol is exported and bound, and what a NULL or unbound model
can show is refused with a message before any device work. The refusals that need a bound geometry (a paged or GPT-2 model, a row
>= B, drop >= max_pos, n_pos > Lmax) are asserted in tests/test_hip_kv_evict_gpu.py."""

import pytest

from specdec_hip import _abi
from test_kv_fork_abi import _unbound_model


def test_the_symbol_is_exported_and_bound():
    lib = _abi.load()
    assert "sd_model_kv_evict" in _abi.SIGNATURES and hasattr(lib, "sd_model_kv_evict")
    assert lib.sd_model_kv_evict.argtypes == _abi.SIGNATURES["sd_model_kv_evict"][1]
    assert lib.sd_abi_version() == _abi.SD_ABI_VERSION == 1      # additive: the version stays


# (row, keep, drop, n_pos) -> message; the model is NULL: refused on the arguments alone, in this order
CASES = {
    "negative_row": ((-1, 4, 8, 40), "row -1 is negative"),
    "negative_keep": ((1, -4, 8, 40), "keep=-4 is negative"),
    "zero_drop": ((1, 4, 0, 40), "drop=0 must be a positive multiple of 8"),
    "negative_drop": ((1, 4, -8, 40), "drop=-8 must be a positive multiple of 8"),
    "odd_drop": ((1, 4, 20, 40), "drop=20 must be a positive multiple of 8"),
    "block_past_n_pos": ((1, 4, 40, 43), "keep=4 + drop=40 exceed n_pos=43"),
    "null_model": ((1, 4, 8, 40), "NULL model"),
    "null_model_empty_move": ((1, 4, 8, 12), "NULL model"),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_kv_evict_refusals(case):
    args, msg = CASES[case]
    assert _abi.load().sd_model_kv_evict(None, *args, None) != 0
    assert msg in _abi.last_error() and _abi.last_error().startswith("kv_evict:"), _abi.last_error()


def test_an_unbound_model_is_refused_even_for_an_empty_move():
    lib, h, keep = _unbound_model()
    try:
        for args in ((0, 4, 8, 40), (0, 4, 8, 12)):
            assert lib.sd_model_kv_evict(h, *args, None) != 0
            assert "not bound" in _abi.last_error() and _abi.last_error().startswith("kv_evict:")
    finally:
        lib.sd_model_destroy(h)
