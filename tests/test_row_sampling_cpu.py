"""Per-request sampling parameters without a GPU: the record's size against the library, the host-side refusals of the four
new entry points (they return before any launch), SamplingParams validation and packing, and --sampling-params on both
command lines."""

import ctypes
import json
import struct

import pytest

from specdec_hip import _abi
from specdec_hip.sampling_params import (ROW_BYTES, RowSampling, SamplingParams, load_file, load_for_cli, pack, pack_bytes, unpack)


def test_record_is_32_bytes_on_both_sides():
    lib = _abi.load()
    assert lib.sd_row_sampling_bytes() == 32 == ctypes.sizeof(RowSampling) == ROW_BYTES
    assert lib.sd_abi_version() == 1


def _err(rc):
    assert rc != 0
    return _abi.last_error()


def test_host_side_refusals_without_a_device():
    """NULL table, B < 1 and a misaligned table are refused by the host code of every entry point, ahead of any launch; the
    pointers below are never dereferenced."""
    lib = _abi.load()
    fake, odd = 0x10000, 0x10008      # 16-byte aligned / only 8-byte aligned
    sample = lambda table, B: lib.sd_sample_token_rows(fake, _abi.SD_BF16, 64, B, 64, None, 1, None, table, None, 0, None, fake, None)  # noqa: E731
    spec = lambda table, B: lib.sd_spec_sample_accept_rows(fake, fake, fake, B, 2, 64, table, None, 0, None, None, fake, fake, None,  # noqa: E731
                                                           fake, 1 << 20, None)
    proc = lambda table, B: lib.sd_logit_process_rows(fake, 64, B, 1, 64, fake, None, None, 0, 0, None, table, None, 0, None, 0,  # noqa: E731
                                                      None, None, 0, None, 0, None)
    for name, fn in (("sample_token_rows", sample), ("spec_sample_accept_rows", spec), ("logit_process_rows", proc)):
        assert "NULL table" in _err(fn(None, 2)), name
        assert "B=0" in _err(fn(fake, 0)), name
        assert "B=-3" in _err(fn(fake, -3)), name
        assert "16-byte aligned" in _err(fn(odd, 2)), name
        assert name in _abi.last_error()
    assert "NULL" in _err(lib.sd_specdec_set_row_sampling(None, fake))
    assert "NULL" in _err(lib.sd_specdec_set_row_sampling(None, None))


def test_sampling_params_validation():
    SamplingParams()                                           # the defaults: whole-vocabulary sampling at T = 1
    assert SamplingParams(temperature=0).greedy and not SamplingParams(temperature=0.7).greedy
    assert SamplingParams(presence_penalty=0.5).has_penalties and not SamplingParams(top_k=5).has_penalties
    for kw, msg in (({"temperature": float("nan")}, "temperature"), ({"temperature": -1.0}, "temperature"),
                    ({"temperature": float("inf")}, "temperature"), ({"top_k": -2}, "top_k"), ({"top_k": 2.5}, "top_k"),
                    ({"top_p": 0.0}, r"top_p=0.0 \(must be > 0\)"), ({"top_p": float("nan")}, "top_p"),
                    ({"repetition_penalty": 0.0}, r"repetition_penalty=0.0 \(must be > 0\)"),
                    ({"repetition_penalty": float("nan")}, "repetition_penalty"),
                    ({"presence_penalty": float("inf")}, "must be finite"), ({"frequency_penalty": float("nan")}, "must be finite"),
                    ({"seed": 1.5}, "seed")):
        with pytest.raises(ValueError, match=msg):
            SamplingParams(**kw)
    # what the device would only turn into a greedy row: refused with the messages of the scalar paths
    with pytest.raises(NotImplementedError, match=r"do_sample=True: top_k=2000 > 1024 is not on the HIP path"):
        SamplingParams(top_k=2000).check(vocab=128256)
    SamplingParams(top_k=2000).check(vocab=1000)              # clamped to the vocabulary: 1000 <= 1024
    with pytest.raises(NotImplementedError, match=r"top_k=2000 is outside 1..1024"):
        SamplingParams(top_k=2000).check(vocab=128256, spec=True)
    with pytest.raises(NotImplementedError, match="without top_k"):
        SamplingParams(top_p=0.9).check(vocab=1000, spec=True)
    SamplingParams(top_p=0.9).check(vocab=1000)               # the full-vocabulary nucleus is a path of the sampled-bonus mode
    SamplingParams(temperature=0, top_p=0.9).check(vocab=1000, spec=True)    # a greedy request: nothing to refuse


def test_normalised_scalars_follow_the_device_rule():
    assert SamplingParams(temperature=0.0, top_k=50, top_p=0.5, seed=3).scalars() == {"temperature": 1.0, "top_k": 1, "top_p": None, "seed": 3}
    assert SamplingParams(temperature=0.7, top_k=50, top_p=0.9).scalars() == {"temperature": 0.7, "top_k": 50, "top_p": 0.9, "seed": 0}
    assert SamplingParams(temperature=1.5, top_p=1.0).scalars() == {"temperature": 1.5, "top_k": None, "top_p": None, "seed": 0}
    assert SamplingParams(top_p=0.9).scalars() == {"temperature": 1.0, "top_k": None, "top_p": 0.9, "seed": 0}
    assert SamplingParams(top_p=0.9).scalars(spec=True)["top_k"] == 1                 # the spec kernels: a greedy row
    assert SamplingParams(top_k=2000).scalars(vocab=128256)["top_k"] == 1 and SamplingParams(top_k=2000).scalars(vocab=1000)["top_k"] == 2000


def test_packing():
    ps = [SamplingParams(temperature=0.7, top_k=50, top_p=0.9, seed=(5 << 32) | 7, repetition_penalty=1.25, presence_penalty=-0.5,
                         frequency_penalty=0.125),
          SamplingParams(temperature=0.0), SamplingParams(seed=None)]
    raw = pack_bytes(ps, default_seed=99)
    assert len(raw) == 3 * 32
    assert struct.unpack("<fifIIfff", raw[:32]) == (struct.unpack("<f", struct.pack("<f", 0.7))[0], 50, struct.unpack("<f", struct.pack("<f", 0.9))[0],
                                                    7, 5, 1.25, -0.5, 0.125)
    assert struct.unpack("<fifIIfff", raw[32:64]) == (0.0, 0, 1.0, 99, 0, 1.0, 0.0, 0.0)      # the entry's own seed, else the call's
    assert struct.unpack("<fifIIfff", raw[64:]) == (1.0, 0, 1.0, 99, 0, 1.0, 0.0, 0.0)
    t = pack(ps, "cpu", default_seed=99)
    assert tuple(t.shape) == (3, 32) and bytes(t.view(-1).tolist()) == raw and t.data_ptr() % 16 == 0
    back = unpack(t)
    assert [(r.top_k, r.seed_lo, r.seed_hi) for r in back] == [(50, 7, 5), (0, 99, 0), (0, 99, 0)]
    assert ps[2].with_seed(4).seed == 4 and ps[0].with_seed(4).seed == (5 << 32) | 7
    with pytest.raises(ValueError, match="empty"):
        pack([], "cpu")


# --------------------------------------------------------------------------------------------------------- command lines
def _file(tmp_path, data, name="sp.json"):
    p = tmp_path / name
    p.write_text(data if isinstance(data, str) else json.dumps(data))
    return str(p)


def test_sampling_params_file(tmp_path):
    good = _file(tmp_path, [{"temperature": 0.7, "top_k": 50, "top_p": 0.9, "seed": 3}, {"temperature": 0, "presence_penalty": 0.5}])
    ps = load_file(good, 2)
    assert ps == [SamplingParams(0.7, 50, 0.9, 3), SamplingParams(temperature=0, presence_penalty=0.5)]
    for data, n, msg in ((good, 3, "2 entries for 3 prompt"), (_file(tmp_path, {"temperature": 1}, "a"), 1, "JSON list"),
                         (_file(tmp_path, "[{", "b"), 1, "not JSON"), (_file(tmp_path, [{"temp": 1}], "c"), 1, "unknown key"),
                         (_file(tmp_path, [3], "d"), 1, "expected an object"), (_file(tmp_path, [{"top_p": 0}], "e"), 1, "top_p")):
        with pytest.raises(ValueError, match=msg):
            load_file(data, n)
    with pytest.raises(OSError):
        load_file(str(tmp_path / "missing.json"), 1)
    assert load_for_cli(None, 1, {"--x": 1.0}) is None
    with pytest.raises(ValueError, match="--a, --b"):
        load_for_cli(good, 2, {"--b": 1.0, "--a": True, "--c": None, "--d": False})


def test_run_specdec_option(tmp_path):
    from src.specdec import run_specdec as cli

    one = _file(tmp_path, [{"temperature": 0.7, "top_k": 40, "seed": 11}])
    base = ["--prompt", "5 6 7", "--sampling-params", one]
    args = cli.parse_args(base + ["--n", "2", "--spec-sampling"])
    assert cli.cli_sampling_params(args) == [SamplingParams(temperature=0.7, top_k=40, seed=11)]
    assert cli.cli_sampling_params(cli.parse_args(["--prompt", "5 6 7"])) is None
    for extra, msg in ((["--repetition-penalty", "1.2"], "--repetition-penalty"), (["--presence-penalty", "0.1"], "--presence-penalty"),
                       (["--frequency-penalty", "0.1"], "--frequency-penalty"), (["--spec-sampling", "--spec-top-k", "5"], "--spec-top-k"),
                       (["--spec-sampling", "--spec-top-k", "5", "--spec-top-p", "0.5"], "--spec-top-p"), (["--adaptive-K"], "--adaptive-K"),
                       (["--controller", "adaptive"], "--controller adaptive"), (["--draft-mode", "eagle"], "--draft-mode eagle"),
                       (["--policy", "typical"], "--policy typical")):
        with pytest.raises(ValueError, match=msg):
            cli.cli_sampling_params(cli.parse_args(base + extra))
    # main() reports and exits 1 before it builds a pipeline
    assert cli.main(base + ["--presence-penalty", "0.1"]) == 1
    assert cli.main(["--prompt", "5 6 7", "--sampling-params", _file(tmp_path, [{}, {}], "two.json")]) == 1
    assert cli.main(["--prompt", "5 6 7", "--sampling-params", str(tmp_path / "missing.json")]) == 1


def test_specdec_cli_option(tmp_path):
    from src.specdec_cli import main as cli

    one = _file(tmp_path, [{"temperature": 0.0}])
    parse = cli.build_parser().parse_args
    assert cli.cli_sampling_params(parse(["run", "--sampling-params", one, "5 6 7"])) == [SamplingParams(temperature=0.0)]
    assert cli.cli_sampling_params(parse(["run", "5 6 7"])) is None
    for extra, msg in ((["--do-sample"], "--do-sample"), (["--repetition-penalty", "1.2"], "--repetition-penalty"),
                       (["--presence-penalty", "0.3"], "--presence-penalty"), (["--frequency-penalty", "0.3"], "--frequency-penalty"),
                       (["--spec-top-k", "5"], "--spec-top-k"), (["--spec-top-p", "0.5"], "--spec-top-p")):
        with pytest.raises(ValueError, match=msg):
            cli.cli_sampling_params(parse(["run", "--sampling-params", one] + extra + ["5 6 7"]))
    with pytest.raises(SystemExit, match="--sampling-params"):
        cli.cmd_run(parse(["run", "--sampling-params", one, "--do-sample", "5 6 7"]))
    with pytest.raises(SystemExit, match="2 entries for 1 prompt"):
        cli.cmd_run(parse(["run", "--sampling-params", _file(tmp_path, [{}, {}], "two.json"), "5 6 7"]))
