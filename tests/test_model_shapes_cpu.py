"""Host-only results of the model's matrix table (csrc/pack.hip) through the C-ABI: packed sizes, the pass size, the workspace and
whether sd_model_create accepts a geometry in bf16 and fp8. Models are created over placeholder pointers and never bound
(sd_model_create does no device work). The expected values were recorded before the table had a single owner."""

import ctypes

import pytest

from specdec_hip import _abi
from specdec_hip.engine import _LayerWeights, _ModelConfig

# name: (arch, n_layers, d_model, n_heads, n_kv_heads, head_dim, d_ff, vocab, max_pos)
GEOMETRIES = {
    "llama-3.2-1b": (0, 16, 2048, 32, 8, 64, 8192, 128256, 8192),
    "llama-3.2-3b": (0, 28, 3072, 24, 8, 128, 8192, 128256, 8192),
    "llama-3-8b": (0, 32, 4096, 32, 8, 128, 14336, 128256, 8192),
    "gpt2": (1, 12, 768, 12, 12, 64, 3072, 50257, 1024),
}

# (name, dtype): (sd_packed_bytes, sd_packed_head_bytes, created, sd_model_pass_tokens, sd_model_workspace_bytes)
EXPECTED = {
    ("llama-3.2-1b", "bf16"): (2471493632, 525336576, True, 128, 45598720),
    ("llama-3.2-1b", "fp8"): (1237767168, 263181312, True, 64, 45598720),
    ("llama-3.2-3b", "bf16"): (6425149440, 788004864, True, 128, 61395968),
    ("llama-3.2-3b", "fp8"): (3216184320, 394515456, True, 64, 61395968),
    ("llama-3-8b", "bf16"): (15009316864, 1050673152, True, 128, 85383168),
    ("llama-3-8b", "fp8"): (7510676480, 525849600, True, 64, 85383168),
    ("gpt2", "bf16"): (247065600, 77196288, True, 9, 22758400),
    ("gpt2", "fp8"): (124065792, 38799360, False, None, None),
}


def _measure(name, dtype):
    lib = _abi.load()
    arch, n_layers, d, hq, hkv, hd, ff, vocab, max_pos = GEOMETRIES[name]
    wd = _abi.SD_BF16 if dtype == "bf16" else _abi.SD_FP8_E4M3
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    layers = (_LayerWeights * n_layers)()
    for layer in layers:
        for f, _ in _LayerWeights._fields_:
            setattr(layer, f, p)
    mc = _ModelConfig(arch=arch, n_layers=n_layers, d_model=d, n_heads=hq, n_kv_heads=hkv, head_dim=hd, d_ff=ff, vocab=vocab,
                      max_pos=max_pos, norm_eps=1e-5, weight_dtype=wd, tok_emb=p, pos_emb=p, final_norm_w=p, final_norm_b=p, lm_head=p,
                      rope_cos=p, rope_sin=p, layers=layers, packed=p)
    packed = lib.sd_packed_bytes(ctypes.byref(mc))
    head = lib.sd_packed_head_bytes(vocab, d, wd)
    h = ctypes.c_void_p()
    if lib.sd_model_create(ctypes.byref(mc), ctypes.byref(h)) != 0:
        return (packed, head, False, None, None)
    try:
        return (packed, head, True, lib.sd_model_pass_tokens(h), lib.sd_model_workspace_bytes(h))
    finally:
        lib.sd_model_destroy(h)


@pytest.mark.parametrize("name,dtype", sorted(EXPECTED))
def test_model_shapes(name, dtype, monkeypatch):
    monkeypatch.delenv("SPECDEC_MAX_PASS_TOKENS", raising=False)   # read by sd_model_create
    assert _measure(name, dtype) == EXPECTED[(name, dtype)]
