"""sd_model_set_kv_dtype and the refusals of an fp8-KV model that need no device: a model created over dummy pointers (create
and the refused calls never dereference them). The Python layers' refusals are in tests/test_hip_kv_fp8_generate_gpu.py."""

import ctypes

from specdec_hip import _abi
from specdec_hip.engine import _LayerWeights, _ModelConfig

P = 1 << 20   # a 16-byte-aligned non-null "pointer"


def _model(lib, head_dim=64):
    layers = (_LayerWeights * 1)()
    for f, _ in _LayerWeights._fields_:
        setattr(layers[0], f, P)
    mc = _ModelConfig(arch=0, n_layers=1, d_model=256, n_heads=4, n_kv_heads=2, head_dim=head_dim, d_ff=512, vocab=512, max_pos=4096,
                      norm_eps=1e-5, weight_dtype=_abi.SD_BF16, tok_emb=P, pos_emb=None, final_norm_w=P, final_norm_b=None, lm_head=P,
                      rope_cos=P, rope_sin=P, layers=layers, packed=None)
    h = ctypes.c_void_p()
    _abi.check(lib.sd_model_create(ctypes.byref(mc), ctypes.byref(h)), "sd_model_create")
    return h, (mc, layers)


def test_setter_sizes_and_refusals_before_device_work():
    lib = _abi.load()
    h, keep = _model(lib)
    bf16 = lib.sd_model_kv_bytes(h, 2, 64)
    for args, word in (((_abi.SD_F32, 1.0, 1.0), "kv dtype"), ((_abi.SD_FP8_E4M3, 0.0, 1.0), "positive"),
                       ((_abi.SD_FP8_E4M3, 1.0, float("inf")), "positive"), ((_abi.SD_FP8_E4M3, float("nan"), 1.0), "positive")):
        assert lib.sd_model_set_kv_dtype(h, *args) != 0 and word in _abi.last_error(), args
    assert lib.sd_model_set_kv_dtype(None, _abi.SD_FP8_E4M3, 1.0, 1.0) != 0
    assert lib.sd_model_kv_bytes(h, 2, 64) == bf16                       # a refused call changes nothing
    assert lib.sd_model_set_kv_dtype(h, _abi.SD_FP8_E4M3, 0.25, 2.0) == 0
    assert lib.sd_model_kv_bytes(h, 2, 64) * 2 == bf16 == 1 * 2 * 2 * 64 * 64 * 2
    assert lib.sd_model_persist_active(h, 1) == 0
    one = (ctypes.c_int32 * 1)(1)
    for rc in (lib.sd_model_bind_paged(h, P, P, 4, 32, P, 2, 1, P, 1 << 40), lib.sd_model_kv_fork(h, 0, one, 1, 8, None),
               lib.sd_model_kv_copy_pages(h, one, (ctypes.c_int32 * 1)(2), 1, 8, None), lib.sd_model_kv_evict(h, 0, 4, 8, 64, None),
               lib.sd_model_bind(h, P, P, 1, 72, P, 1 << 40)):               # Lmax % 16 != 0
        assert rc != 0 and "kv dtype" in _abi.last_error(), _abi.last_error()
    assert lib.sd_model_set_kv_dtype(h, _abi.SD_BF16, 3.0, 3.0) == 0 and lib.sd_model_kv_bytes(h, 2, 64) == bf16
    lib.sd_model_destroy(h)
    h32, keep32 = _model(lib, head_dim=32)
    assert lib.sd_model_set_kv_dtype(h32, _abi.SD_FP8_E4M3, 1.0, 1.0) == 0
    assert lib.sd_model_bind(h32, P, P, 1, 64, P, 1 << 40) != 0 and "kv dtype" in _abi.last_error() and "head_dim" in _abi.last_error()
    lib.sd_model_destroy(h32)
