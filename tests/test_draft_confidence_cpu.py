"""Confidence-gated draft length without a device: the float64 restatement (tests/draft_confidence_ref.py) on hand-made rows, the stop
rule's edges, every refusal and route of the call resolution with its message (the stand-in pipelines of tests/call_route_cases.py),
the config key, the command-line flags, and the C ABI's symbols and argument checks."""

import math

import numpy as np
import pytest

import call_route_cases as C
import draft_confidence_ref as R

NEG, NAN = float("-inf"), float("nan")


# ---------------------------------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("V", [1, 7, 160, 4099])
def test_conf_on_planted_rows(V):
    one = np.full(V, NEG)
    one[V // 2] = -3.25
    assert R.conf(one) == 1.0                                        # one-hot
    assert R.conf(np.full(V, 0.75)) == pytest.approx(1.0 / V, rel=1e-13)   # flat
    for n in (1, 2, 5):
        if V >= 2 * n:
            r = np.full(V, -30.0)
            r[:n] = 0.0
            assert R.conf(r) == pytest.approx(1.0 / n, rel=1e-9)     # n equal maxima over a -30 floor: (V - n) e^-30 < 4e-10
    if V >= 4:
        half = np.full(V, 2.0)
        half[::2] = NEG                                              # -inf entries add 0
        assert R.conf(half) == pytest.approx(1.0 / (V // 2), rel=1e-13)
    for bad in (NAN, float("inf")):
        r = np.zeros(V)
        r[V - 1] = bad
        assert math.isnan(R.conf(r))
    assert math.isnan(R.conf(np.full(V, NEG)))
    for name, row, want in R.planted_rows(V):
        got = R.conf(row)
        assert (math.isnan(got) and math.isnan(want)) or got == pytest.approx(want, rel=1e-12), name


def test_k_rule_edges():
    K = 4
    hi, lo = 0.9, 0.1
    assert R.k_rule([hi] * K, 0.5, 1) == K                           # no stop
    assert R.k_rule([lo, hi, hi, hi], 0.5, 1) == 1                   # the first judged forward
    assert R.k_rule([lo, lo, hi, hi], 0.5, 2) == 2                   # min_k: forward 0 is not judged
    assert R.k_rule([lo, hi, lo, hi], 0.5, 2) == 3
    assert R.k_rule([lo, lo, lo, hi], 0.5, 4) == K                   # min_k = K: nothing is judged
    assert R.k_rule([hi, hi, hi, lo], 0.5, 1) == K                   # forward K - 1 needs no judgement
    assert R.k_rule([hi, NAN, hi, hi], 0.5, 1) == 2                  # a NaN stops the row
    assert R.k_rule([0.5, 0.5, 0.5, 0.5], 0.5, 1) == K               # c == tau continues
    assert R.k_rule([hi], 0.5, 1) == 1                               # K = 1
    assert R.margins([hi, lo, hi, hi], 0.5, 1) == pytest.approx([0.4, 0.4])
    assert R.margins([hi, hi, hi, hi], 0.5, 2) == pytest.approx([0.4, 0.4])
    assert R.margins([hi, NAN, hi, hi], 0.5, 1)[-1] == float("inf")


# ---------------------------------------------------------------------------------------------------- refusals and routes
def _resolve(stand_in, single=False, policy_routes=True, **kw):
    from src.specdec.core.step_options import resolve

    pipe = C.STAND_INS[stand_in]()
    tau, min_k = kw.pop("draft_confidence", None), kw.pop("draft_min_k", None)
    grammar = C._grammar(kw.pop("grammar")) if "grammar" in kw else None
    rows = C._ROWS[kw.pop("sampling_params")]() if "sampling_params" in kw else None
    prompts = [C.PROMPTS[-1]] if single else C.PROMPTS
    return pipe, resolve(pipe, prompts, None, None, kw.pop("do_sample", None), kw, grammar=grammar, sampling_params=rows, single=single,
                         policy_routes=policy_routes, draft_confidence=tau, draft_min_k=min_k)


def test_routes():
    for many in (False, True):
        _, call = _resolve("longest_prefix", policy_routes=not many, draft_confidence=0.4)
        assert call.route == "step" and (call.options.draft_confidence, call.options.draft_min_k) == (0.4, 1) and call.options.mode == "greedy"
    _, call = _resolve("longest_prefix", draft_confidence=1, draft_min_k=3, do_sample=True)        # the sampled bonus token stays allowed
    assert (call.options.mode, call.options.draft_confidence, call.options.draft_min_k) == ("sampled", 1.0, 3)
    _, call = _resolve("longest_prefix")
    assert call.options.draft_confidence is None and call.options.draft_min_k == 1


REFUSALS = [
    ("longest_prefix", dict(draft_confidence=0.0), ValueError, "draft_confidence=0.0 (a threshold in (0, 1])"),
    ("longest_prefix", dict(draft_confidence=1.5), ValueError, "draft_confidence=1.5"),
    ("longest_prefix", dict(draft_confidence=NAN), ValueError, "draft_confidence=nan"),
    ("longest_prefix", dict(draft_confidence="0.5"), ValueError, "draft_confidence='0.5'"),
    ("longest_prefix", dict(draft_confidence=0.5, draft_min_k=0), ValueError, "draft_min_k=0 (an integer in 1..K)"),
    ("longest_prefix", dict(draft_confidence=0.5, draft_min_k=1.5), ValueError, "draft_min_k=1.5"),
    ("longest_prefix", dict(draft_min_k=2), ValueError, "draft_min_k belongs to draft_confidence"),
    ("longest_prefix/adaptive", dict(draft_confidence=0.5), NotImplementedError, "needs a fixed shape K (controller='fixed')"),
    ("longest_prefix/adaptive_per_row", dict(draft_confidence=0.5), NotImplementedError, "adaptive K is not supported with it"),
    ("medusa_heads", dict(draft_confidence=0.5), NotImplementedError, "needs the draft-model mode (draft_mode='vanilla')"),
    ("typical", dict(draft_confidence=0.5), NotImplementedError,
     "draft_confidence is decided inside the captured device step: policy='typical' on the host loop is not supported with it"),
    ("rejection/host", dict(draft_confidence=0.5), NotImplementedError, "policy='rejection' on the host loop is not supported with it"),
    ("rejection/device", dict(draft_confidence=0.5), NotImplementedError, "not supported with speculative sampling"),
    ("fake", dict(draft_confidence=0.5), NotImplementedError, "implementation='fake' is not supported with it"),
    ("longest_prefix", dict(draft_confidence=0.5, repetition_penalty=1.2), NotImplementedError, "not supported with logit processors"),
    ("longest_prefix", dict(draft_confidence=0.5, bad_token_ids=[7]), NotImplementedError, "not supported with logit processors"),
    ("longest_prefix", dict(draft_confidence=0.5, grammar="A"), NotImplementedError, "not supported with a grammar"),
    ("longest_prefix", dict(draft_confidence=0.5, sampling_params="plain"), NotImplementedError, "not supported with sampling_params"),
]


@pytest.mark.parametrize("stand_in,kw,exc,message", REFUSALS, ids=[f"{s}-{i}" for i, (s, *_) in enumerate(REFUSALS)])
def test_refusals_of_a_call(stand_in, kw, exc, message):
    with pytest.raises(exc) as e:
        _resolve(stand_in, **dict(kw))
    assert message in str(e.value)


def test_generate_refuses_it():
    with pytest.raises(NotImplementedError, match="belongs to generate_batch, generate_many and start_session"):
        _resolve("longest_prefix", single=True, draft_confidence=0.5)
    pipe = C.STAND_INS["longest_prefix"]()
    with pytest.raises(NotImplementedError, match="generate\\(\\) emits the draft's own tokens"):
        pipe.generate(C.PROMPTS[0], draft_confidence=0.5)


def test_device_rule_and_session_refusals():
    from src.specdec.core import draft_confidence as D
    from src.specdec.core.acceptance import DeviceRule
    from src.specdec.core.step_options import Processors, StepOptions

    pipe = C.STAND_INS["longest_prefix"]()
    pipe.accept_device = DeviceRule("typical")
    from src.specdec.core.step_options import resolve
    with pytest.raises(NotImplementedError, match="not supported with policy 'typical' / 'topk_agree' on the device"):
        resolve(pipe, C.PROMPTS, None, None, None, {}, draft_confidence=0.5)
    # start_session: the mode, then the same refusals
    pipe = C.STAND_INS["longest_prefix"]()
    with pytest.raises(NotImplementedError, match="needs the bonus-token emit mode"):
        D.session_confidence(pipe, StepOptions(), 1, False, 0.5, None, 0)
    with pytest.raises(NotImplementedError, match="needs the draft-model mode"):
        D.session_confidence(pipe, StepOptions(), 0, True, 0.5, None, 0)
    with pytest.raises(NotImplementedError, match="speculative sampling"):
        D.session_confidence(pipe, StepOptions("spec"), 0, False, 0.5, None, 0)
    assert D.session_confidence(pipe, StepOptions(), 1, False, None, None, 0) == StepOptions()
    got = D.session_confidence(pipe, StepOptions("sampled", 0.8, 20, None, 3), 0, False, 0.25, 2, 0)
    assert (got.draft_confidence, got.draft_min_k, got.mode, got.top_k) == (0.25, 2, "sampled", 20)
    with pytest.raises(NotImplementedError, match="draft_confidence needs"):
        pipe.start_session(C.PROMPTS, 16, 1, None, draft_confidence=0.5)
    # the session's own checks
    on = StepOptions(draft_confidence=0.5, draft_min_k=3)
    assert D.check_session(StepOptions(), True, False, 1) is False
    assert D.check_session(on, False, True, 4) is True
    with pytest.raises(ValueError, match="draft_min_k=3 exceeds the step's K \\(2\\)"):
        D.check_session(on, False, True, 2)
    for other_step, bonus, o in ((True, True, on), (False, False, on), (False, True, StepOptions("spec", draft_confidence=0.5)),
                                 (False, True, StepOptions(draft_confidence=0.5, processors=Processors.IDENTITY))):
        with pytest.raises(NotImplementedError, match="needs the bonus-token HIP step with a draft model and a fixed K"):
            D.check_session(o, other_step, bonus, 4)


# ---------------------------------------------------------------------------------------------------- config key and flags
def test_config_key(tmp_path):
    from src.specdec.core import pipeline as P
    from src.specdec.core.step_options import resolve

    assert "draft_confidence_threshold" not in P._DEFAULTS                   # absent = off
    cfg = tmp_path / "c.yaml"
    cfg.write_text("draft_confidence_threshold: 0.35\ndraft_min_k: 2\n")
    pipe = C.STAND_INS["longest_prefix"]()
    pipe.config = dict(pipe._load_config(str(cfg)), implementation="hip")
    call = resolve(pipe, C.PROMPTS, None, None, None, {})
    assert (call.options.draft_confidence, call.options.draft_min_k) == (0.35, 2)
    call = resolve(pipe, C.PROMPTS, None, None, None, {}, draft_confidence=0.6)      # the call's threshold over the config's
    assert (call.options.draft_confidence, call.options.draft_min_k) == (0.6, 1)
    call = resolve(pipe, [C.PROMPTS[0]], None, None, None, {}, single=True)          # generate() does not read the key
    assert call.options.draft_confidence is None
    shipped = pipe._load_config(str(C.PKG / "configs" / "specdec.yaml"))
    assert "draft_confidence_threshold" not in shipped


def test_cli_flags():
    from src.specdec import run_specdec
    from src.specdec_cli.main import build_parser

    a = run_specdec.parse_args(["--prompt", "1 2 3", "--draft-confidence", "0.4", "--draft-min-k", "2"])
    assert (a.draft_confidence, a.draft_min_k) == (0.4, 2)
    a = run_specdec.parse_args(["--prompt", "1 2 3"])
    assert (a.draft_confidence, a.draft_min_k) == (None, None)
    assert run_specdec.main(["--prompt", "1 2 3", "--draft-min-k", "2"]) == 1        # belongs to --draft-confidence
    a = build_parser().parse_args(["run", "--draft-confidence", "0.4", "--draft-min-k", "3", "1 2 3"])
    assert (a.draft_confidence, a.draft_min_k) == (0.4, 3)
    a = build_parser().parse_args(["run", "1 2 3"])
    assert (a.draft_confidence, a.draft_min_k) == (None, None)


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_symbols_are_declared_bound_and_check_their_arguments():
    from specdec_hip import _abi, ops

    lib = _abi.load()
    header = (C.ROOT / "include" / "specdec_hip.h").read_text()
    for name in ("sd_draft_confidence", "sd_specdec_draft_confidence_bytes", "sd_specdec_set_draft_confidence"):
        assert name in _abi.SIGNATURES and hasattr(lib, name) and f"{name}(" in header
        assert getattr(lib, name).argtypes == _abi.SIGNATURES[name][1]
    assert lib.sd_abi_version() == _abi.SD_ABI_VERSION == 1                  # additive: the version stays
    assert lib.sd_specdec_draft_confidence_bytes(3, 160) == 3 * 2 * 160 * 2
    assert lib.sd_specdec_draft_confidence_bytes(0, 160) == 0
    assert lib.sd_draft_confidence(None, _abi.SD_BF16, 8, 1, 8, None, None) != 0 and "NULL" in _abi.last_error()
    buf = (16 * 4) * b"\0"
    import ctypes
    p = ctypes.cast(ctypes.create_string_buffer(buf), ctypes.c_void_p)
    for args, word in (((_abi.SD_I32, 8, 1, 8), "dtype"), ((_abi.SD_BF16, 8, 0, 8), "B=0"), ((_abi.SD_BF16, 8, 1, 0), "V=0"),
                       ((_abi.SD_BF16, 7, 2, 8), "row_stride 7 below V")):
        assert lib.sd_draft_confidence(p, args[0], args[1], args[2], args[3], p, None) != 0
        assert word in _abi.last_error(), (args, _abi.last_error())
    assert lib.sd_specdec_set_draft_confidence(None, 1, 0.5, 1, None, 0, None) != 0 and "NULL" in _abi.last_error()
    assert callable(ops.draft_confidence)
    from specdec_hip.engine import HipSpecDec
    assert callable(HipSpecDec.set_draft_confidence)
