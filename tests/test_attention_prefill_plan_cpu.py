"""The tiled prompt-attention mode without a device: its plan query (sd_attention_prefill_plan, the function the launch consults),
the refusals of the setter, and the option's way from the command line to HipLM.prefill_attention."""

import ctypes
import itertools
import types

import pytest

from specdec_hip import _abi
from specdec_hip import weights as W
from specdec_hip.ops import attention_prefill_plan
from test_kv_fp8_refusals_cpu import P, _model

HEADS = {"3b": (24, 8, 128), "1b": (32, 8, 64)}


@pytest.mark.parametrize("geo,Mc,l_max,paged", list(itertools.product(HEADS, (96, 128, 512), (1024, 32768), (0, 64))))
def test_plan_covers_every_row_once(geo, Mc, l_max, paged):
    hq, hkv, D = HEADS[geo]
    G = hq // hkv
    p = attention_prefill_plan(hq, hkv, D, Mc, l_max, paged)
    # row r of tile t is (head r // pt, position t * pt + r % pt): every (position, head) of the chunk exactly once
    seen = [(t * p.pt + r % p.pt, r // p.pt) for t in range(p.tiles) for r in range(p.rows_per_wg)
            if r // p.pt < G and t * p.pt + r % p.pt < Mc]
    assert sorted(seen) == sorted(itertools.product(range(Mc), range(G)))
    assert p.rows_per_wg % 16 == 0 and p.rows_per_wg == p.waves * 16 and p.rows_per_wg - 16 < p.pt * G <= p.rows_per_wg
    assert 0 < p.lds_bytes <= 160 * 1024 and p.lds_bytes == 2 * 2 * (64 * (D + 8) + D * 72)
    assert p.n_split == 1
    if Mc == 512:
        assert p.tiles * p.n_split * hkv >= 256, p


def test_refusals_by_message():
    for args, word in (((4, 2, 32, 128, 1024), "head_dim"), ((5, 2, 64, 128, 1024), "query heads per kv head"),
                       ((32, 2, 64, 128, 1024), "query heads per kv head"), ((4, 2, 64, 0, 1024), "Mc=0"),
                       ((4, 2, 64, 513, 1024), "Mc=513"), ((4, 2, 64, 128, 1020), "multiple of 8"), ((4, 2, 64, 128, 1024, 48), "pages")):
        with pytest.raises(RuntimeError, match=word):
            attention_prefill_plan(*args)
    lib = _abi.load()
    assert lib.sd_model_set_prefill_attention(None, 1) != 0 and "NULL" in _abi.last_error()
    assert lib.sd_model_prefill_attention(None) == -1 and lib.sd_model_prefill_tiled_launches(None) == -1
    h, keep = _model(lib)
    assert lib.sd_model_set_prefill_attention(h, 2) != 0 and "unknown mode" in _abi.last_error()
    assert lib.sd_model_set_prefill_attention(h, _abi.SD_PREFILL_ATTN_TILED) == 0 and lib.sd_model_prefill_attention(h) == 1
    assert lib.sd_model_set_kv_dtype(h, _abi.SD_FP8_E4M3, 1.0, 1.0) != 0 and "fp8" in _abi.last_error()
    assert lib.sd_model_set_prefill_attention(h, _abi.SD_PREFILL_ATTN_PASSES) == 0
    assert lib.sd_model_set_kv_dtype(h, _abi.SD_FP8_E4M3, 1.0, 1.0) == 0
    assert lib.sd_model_set_prefill_attention(h, _abi.SD_PREFILL_ATTN_TILED) != 0 and "fp8" in _abi.last_error()
    lib.sd_model_destroy(h)
    h32, keep32 = _model(lib, head_dim=32)
    assert lib.sd_model_set_prefill_attention(h32, _abi.SD_PREFILL_ATTN_TILED) != 0 and "head_dim" in _abi.last_error()
    lib.sd_model_destroy(h32)
    hg, keepg = _model(lib)
    keepg[0].arch, keepg[0].pos_emb, keepg[0].final_norm_b = 1, P, P          # the same dimensions as a GPT-2 model
    h2 = ctypes.c_void_p()
    _abi.check(lib.sd_model_create(ctypes.byref(keepg[0]), ctypes.byref(h2)), "sd_model_create")
    assert lib.sd_model_set_prefill_attention(h2, _abi.SD_PREFILL_ATTN_TILED) != 0 and "Llama" in _abi.last_error()
    lib.sd_model_destroy(h2)
    lib.sd_model_destroy(hg)


def test_option_reaches_the_models(monkeypatch):
    from specdec_hip.engine import HipModel
    from src.specdec import HipLM
    from src.specdec.core.pipeline import SpeculativePipeline
    from src.specdec.run_specdec import parse_args

    assert parse_args(["--prompt", "1 2 3"]).prefill_attention is None
    assert parse_args(["--prompt", "1 2 3", "--prefill-attention", "tiled"]).prefill_attention == "tiled"
    with pytest.raises(SystemExit):
        parse_args(["--prompt", "1 2 3", "--prefill-attention", "flash"])
    mw = W.synthetic_llama(W.ModelConfig(), seed=1)      # CPU tensors: any device work would fail differently
    with pytest.raises(ValueError, match="prefill_attention"):
        HipModel(mw, batch=1, l_max=64, prefill_attention="flash")
    with pytest.raises(ValueError, match="prefill_attention"):
        HipLM(mw, prefill_attention="flash")
    lms = [HipLM.__new__(HipLM), HipLM.__new__(HipLM)]
    for lm in lms:
        lm.prefill_attention = "passes"
    pipe = types.SimpleNamespace(base_lm=lms[0], draft_lm=lms[1])
    SpeculativePipeline.set_prefill_attention(pipe, "tiled")             # what both CLIs call with the parsed option
    assert [lm.prefill_attention for lm in lms] == ["tiled", "tiled"]
    with pytest.raises(ValueError, match="prefill_attention"):
        SpeculativePipeline.set_prefill_attention(pipe, "flash")
    # both command lines hand the parsed option to the pipeline they create (a stand-in that stops there)
    import src.specdec.run_specdec as rs
    from src.specdec_cli import main as cli

    assert cli.build_parser().parse_args(["run", "--prefill-attention", "tiled", "hi"]).prefill_attention == "tiled"
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["run", "--prefill-attention", "flash", "hi"])
    seen = []

    class Stop(Exception):
        pass

    class Pipe:
        base_lm = draft_lm = None

        def __init__(self, *a, **kw):
            pass

        def set_prefill_attention(self, name):
            seen.append(name)
            raise Stop()

    monkeypatch.setattr(rs, "SpeculativePipeline", Pipe)
    monkeypatch.setattr(cli, "SpeculativePipeline", Pipe)
    for run in (lambda: rs.main(["--prompt", "1 2 3", "--prefill-attention", "tiled"]),
                lambda: cli.main(["run", "--prefill-attention", "tiled", "hi"])):
        try:
            run()
        except (Stop, SystemExit):
            pass
    assert seen == ["tiled", "tiled"]
    import src.kernels as sk

    assert sk.get_kernel_info()["prefill_attention"] == ["passes", "tiled"]
