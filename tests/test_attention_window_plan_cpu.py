"""Sliding-window attention, host side: the launch plan (sd_attention_window_plan), the refusals of sd_model_set_sliding_window and
its neighbours by message (a model over dummy pointers, as tests/test_kv_fp8_refusals_cpu.py builds one; the refusal of a BOUND
model needs a bind and is in tests/test_hip_attention_window_gpu.py), the command-line option and a checkpoint directory's config."""

import ctypes
import json
import types

import pytest

from specdec_hip import _abi
from specdec_hip import weights as W
from specdec_hip.ops import attention_plan, attention_prefill_plan, attention_window_plan
from test_kv_fp8_refusals_cpu import P, _model


@pytest.mark.parametrize("Wn", [1, 40, 100, 511, 1100, 4096, 40000])
@pytest.mark.parametrize("M", [1, 5, 17, 128])
@pytest.mark.parametrize("l_max", [512, 8192, 32768])
def test_plan_follows_the_span(Wn, M, l_max):
    hq, hkv, B = 24, 8, 1
    plan, plain = attention_window_plan(hq, hkv, 128, B, M, l_max, Wn), attention_plan(hq, hkv, 128, B, M, l_max)
    base = hkv * B * plan.tiles
    assert plan.tiles == plain.tiles and plan.grid == (hkv, B, plan.tiles * plan.n_split)
    assert plan.n_split == max(1, min(min(l_max, Wn + M) // 512, 32, 1024 // base, 512 // base)) <= plain.n_split
    assert 1 <= plan.max_blocks <= (Wn + M) // 32 + 2 and plan.max_blocks <= -(-l_max // 32)
    pf = attention_prefill_plan(hq, hkv, 128, min(4 * M, 512), l_max, window=Wn)
    assert pf[:6] == attention_prefill_plan(hq, hkv, 128, min(4 * M, 512), l_max)[:6] and 1 <= pf.max_blocks <= (Wn + pf.pt) // 64 + 2


def test_a_32k_cache_under_a_4k_window_launches_8_way(monkeypatch):
    assert attention_window_plan(24, 8, 128, 1, 5, 32768, 4096).n_split == 8 and attention_plan(24, 8, 128, 1, 5, 32768).n_split == 32
    monkeypatch.setenv("SPECDEC_NO_ATTN_SPLIT", "1")
    assert attention_window_plan(24, 8, 128, 1, 5, 32768, 4096).n_split == 1
    for args in ((24, 8, 128, 1, 5, 32768, 0), (24, 8, 32, 1, 5, 32768, 64), (24, 8, 128, 1, 129, 32768, 64)):
        with pytest.raises(_abi.HipLibraryError, match="sliding_window|M="):
            attention_window_plan(*args)


def test_refusals_by_message():
    lib = _abi.load()
    err = lambda rc: rc != 0 and "sliding_window" in _abi.last_error()     # noqa: E731
    h, keep = _model(lib)
    assert lib.sd_model_sliding_window(h) == 0 and lib.sd_model_sliding_window(None) == -1
    assert err(lib.sd_model_set_sliding_window(h, -1)) and lib.sd_model_set_sliding_window(None, 64) != 0
    assert lib.sd_model_set_sliding_window(h, 4096) == 0 and lib.sd_model_sliding_window(h) == 4096
    assert lib.sd_model_persist_active(h, 1) == 0
    assert err(lib.sd_model_set_kv_dtype(h, _abi.SD_FP8_E4M3, 1.0, 1.0)) and err(lib.sd_model_set_cascade(h, 1))      # fp8, cascade after
    assert err(lib.sd_model_kv_evict(h, 0, 4, 8, 64, None))
    assert lib.sd_model_set_kv_dtype(h, _abi.SD_BF16, 1.0, 1.0) == 0 and lib.sd_model_set_cascade(h, 0) == 0
    assert lib.sd_model_set_sliding_window(h, 0) == 0
    assert lib.sd_model_set_kv_dtype(h, _abi.SD_FP8_E4M3, 1.0, 1.0) == 0 and err(lib.sd_model_set_sliding_window(h, 64))   # fp8 before
    assert lib.sd_model_set_kv_dtype(h, _abi.SD_BF16, 1.0, 1.0) == 0 and lib.sd_model_set_cascade(h, 1) == 0
    assert err(lib.sd_model_set_sliding_window(h, 64)) and lib.sd_model_sliding_window(h) == 0                          # cascade before
    assert lib.sd_model_set_sliding_window(h, 0) == 0                                                                    # off is always accepted
    lib.sd_model_destroy(h)
    h32, keep32 = _model(lib, head_dim=32)
    assert err(lib.sd_model_set_sliding_window(h32, 64)) and "head_dim" in _abi.last_error()
    lib.sd_model_destroy(h32)
    hg, keepg = _model(lib)
    keepg[0].arch, keepg[0].pos_emb, keepg[0].final_norm_b = 1, P, P          # the same dimensions as a GPT-2 model
    h2 = ctypes.c_void_p()
    _abi.check(lib.sd_model_create(ctypes.byref(keepg[0]), ctypes.byref(h2)), "sd_model_create")
    assert err(lib.sd_model_set_sliding_window(h2, 64)) and "GPT-2" in _abi.last_error()
    lib.sd_model_destroy(h2)
    lib.sd_model_destroy(hg)


def test_option_reaches_the_models():
    import src.specdec.run_specdec as rs
    from specdec_hip.engine import HipModel
    from src.specdec import HipLM
    from src.specdec.core.pipeline import SpeculativePipeline
    from src.specdec_cli import main as cli

    mw = W.synthetic_llama(W.ModelConfig(), seed=1)      # CPU tensors: the Python layers refuse before any device work
    for make in (lambda **kw: HipModel(mw, batch=1, l_max=64, **kw), lambda **kw: HipLM(mw, **kw)):
        for kw in (dict(sliding_window=-1), dict(sliding_window=64, kv_dtype="fp8")):
            with pytest.raises(ValueError, match="sliding_window"):
                make(**kw)
    assert rs.parse_args(["--prompt", "1 2 3"]).sliding_window is None
    assert rs.parse_args(["--prompt", "1 2 3", "--sliding-window", "4096"]).sliding_window == 4096
    assert cli.build_parser().parse_args(["run", "--sliding-window", "4096", "hi"]).sliding_window == 4096
    lms = [HipLM.__new__(HipLM), HipLM.__new__(HipLM)]
    for lm, own in zip(lms, (0, 512)):                    # the second model's own config carries a window: it keeps it
        lm.sliding_window, lm.config, lm.kv_cache_dtype, lm.cascade_attention = own, W.ModelConfig(sliding_window=own), "bf16", False
    pipe = types.SimpleNamespace(base_lm=lms[0], draft_lm=lms[1])
    SpeculativePipeline.set_sliding_window(pipe, 4096)    # what both CLIs call with the parsed option
    assert [lm.sliding_window for lm in lms] == [4096, 512]
    with pytest.raises(ValueError, match="sliding_window"):
        SpeculativePipeline.set_sliding_window(pipe, -4)


@pytest.mark.parametrize("value,want", [(4096, 4096), (None, 0), ("absent", 0)])
def test_checkpoint_config_carries_the_window(tmp_path, value, want):
    from test_checkpoint_dir import _tiny_llama

    _tiny_llama(False).save_pretrained(tmp_path, safe_serialization=True)
    raw = json.loads((tmp_path / "config.json").read_text())
    raw.update(model_type="mistral", architectures=["MistralForCausalLM"])
    if value != "absent":
        raw["sliding_window"] = value
    (tmp_path / "config.json").write_text(json.dumps(raw))
    got = W.load_checkpoint_dir(str(tmp_path), device="cpu").config
    assert got.arch == W.ARCH_LLAMA and got.sliding_window == want and got.n_layers == raw["num_hidden_layers"]
