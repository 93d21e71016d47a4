"""The prompt-prefill backend option of the command line and of the Python surface: names are checked before any device work
(these run on a host without a GPU)."""

import pytest

from specdec_hip import _abi
from specdec_hip import weights as W


def test_run_specdec_parses_the_prefill_backend():
    from src.specdec.run_specdec import parse_args

    assert parse_args(["--prompt", "1 2 3"]).prefill_backend == "auto"
    for name in ("auto", "passes", "rocblas", "native"):
        assert parse_args(["--prompt", "1 2 3", "--prefill-backend", name]).prefill_backend == name
    with pytest.raises(SystemExit):
        parse_args(["--prompt", "1 2 3", "--prefill-backend", "cublas"])


def test_unknown_backend_name_raises_before_device_work():
    from specdec_hip.engine import HipModel
    from src.specdec import HipLM

    mw = W.synthetic_llama(W.ModelConfig(), seed=1)      # CPU tensors: any device work would fail differently
    with pytest.raises(ValueError, match="prefill_backend"):
        HipModel(mw, batch=1, l_max=64, prefill_backend="cublas")
    with pytest.raises(ValueError, match="prefill_backend"):
        HipLM(mw, prefill_backend="fast")


def test_backend_enum_and_availability():
    lib = _abi.load()
    assert _abi.PREFILL_BACKENDS == {"auto": 0, "passes": 1, "rocblas": 2, "native": 3}
    for v in (_abi.SD_PREFILL_AUTO, _abi.SD_PREFILL_PASSES, _abi.SD_PREFILL_NATIVE):
        assert lib.sd_prefill_backend_available(v) == 1
    assert lib.sd_prefill_backend_available(4) == 0 and lib.sd_prefill_backend_available(-1) == 0
    assert lib.sd_model_set_prefill_backend(None, _abi.SD_PREFILL_NATIVE) != 0 and "NULL" in _abi.last_error()
    assert lib.sd_model_prefill_count(None, _abi.SD_PREFILL_NATIVE) == -1
    import src.kernels as sk

    info = sk.get_kernel_info()
    assert {"passes", "native"} <= set(info["prefill_backends"])
    assert ("rocblas" in info["prefill_backends"]) == bool(lib.sd_prefill_backend_available(_abi.SD_PREFILL_ROCBLAS))
