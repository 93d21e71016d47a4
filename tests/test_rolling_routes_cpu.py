"""context_window / attention_sinks through generate, generate_batch, generate_many and start_session on the stand-in pipeline of
tests/call_route_cases.py (no device): every refusal of the rolling context window with its message, the Window that reaches
DecodeSession where the feature is allowed, and nothing changed where it is not asked."""

from types import SimpleNamespace

import pytest

import call_route_cases as C
from src.specdec.core import pipeline as P
from src.specdec.core import rolling

PROMPTS = [list(range(10, 22)), list(range(30, 54))]


class _Reached(Exception):
    pass


def _pipe(name="longest_prefix", **kw):
    pipe = C.STAND_INS[name]() if not kw else C._stand_in(**kw)
    got = {}

    def runtime(*a, **k):
        got["runtime"] = (a, k)
        raise _Reached
    pipe._runtime = runtime
    return pipe, got


def _call(pipe, entry, **kw):
    if entry == "generate":
        return pipe.generate(PROMPTS[0], max_tokens=300, **kw)
    if entry == "generate_batch":
        return pipe.generate_batch(PROMPTS, max_tokens=300, **kw)
    if entry == "generate_many":
        return pipe.generate_many(PROMPTS, max_tokens=300, batch_size=1, **kw)
    return pipe.start_session(PROMPTS, 300, 1 if entry.endswith("/draft") else 0, **kw)


BATCH = ("generate_batch", "generate_many", "start_session")


@pytest.mark.parametrize("entry", BATCH)
def test_the_window_reaches_the_session_and_sizes_the_caches(entry):
    pipe, got = _pipe()
    with pytest.raises(_Reached):
        _call(pipe, entry, context_window=96)
    (batch, need, k, *_), kw = got["runtime"]
    w = rolling.plan(96, 4, 4)
    assert need == w.l_max == 96 + 17 and kw.get("windowed") is True and k == 4       # sized by the window, not by 300 tokens
    pipe, got = _pipe()
    with pytest.raises(_Reached):
        _call(pipe, entry)
    (batch, need, *_), kw = got["runtime"]
    assert need == 24 + 300 + 8 + 8 and "windowed" not in kw                            # not asked: as before


@pytest.mark.parametrize("entry", BATCH)
def test_config_keys_and_attention_sinks(entry):
    pipe, got = _pipe()
    pipe.config.update(context_window=128, attention_sinks=8)
    seen = {}
    real = P.DecodeSession.__init__

    def init(self, *a, **kw):
        seen["window"] = kw.get("window")
        return real(self, *a, **kw)
    P.DecodeSession.__init__ = init
    try:
        with pytest.raises(_Reached):
            _call(pipe, entry)
        assert seen["window"] == rolling.plan(128, 8, 4) and seen["window"].drop == 56
        with pytest.raises(_Reached):
            _call(pipe, entry, context_window=96, attention_sinks=0)                    # the call's over the config's
        assert seen["window"] == rolling.plan(96, 0, 4)
    finally:
        P.DecodeSession.__init__ = real


ALLOWED = {
    "greedy": ({}, {}),
    "do_sample": ({}, {"do_sample": True}),
    "rejection/device": ({"name": "rejection/device"}, {}),
    "typical/device": ({"kw": dict(policy="typical", policy_params={"backend": "device"})}, {}),
    "processors": ({}, {"repetition_penalty": 1.2, "bad_token_ids": [3]}),
    "grammar": ({}, {"grammar": "A"}),
    "sampling_params": ({}, {"sampling_params": "two"}),
    "logprobs": ({}, {"logprobs": 2}),
    "draft_confidence": ({}, {"draft_confidence": 0.4}),
}


@pytest.mark.parametrize("mode", sorted(ALLOWED))
def test_allowed_next_to_the_other_modes_of_the_step(mode):
    how, kw = ALLOWED[mode]
    kw = dict(kw)
    pipe, got = _pipe(how.get("name", "longest_prefix"), **how.get("kw", {}))
    if "accept_device" not in vars(pipe):
        from src.specdec.core.acceptance import device_rule
        pipe.accept_device = device_rule(pipe.policy_name, how.get("kw", {}).get("policy_params"), False, C.V_SMALL)
    if "grammar" in kw:
        kw["grammar"] = C.automata()[kw["grammar"]]
    if "sampling_params" in kw:
        kw["sampling_params"] = C._ROWS[kw["sampling_params"]]()
    with pytest.raises(_Reached):
        pipe.generate_batch(PROMPTS, max_tokens=300, context_window=96, **kw)
    assert got["runtime"][1].get("windowed") is True


def _refused(pipe, entry, exc, msg, **kw):
    kw.setdefault("context_window", 96)
    with pytest.raises(exc, match=msg):
        _call(pipe, entry, **kw)


def test_generate_is_refused():
    pipe, _ = _pipe()
    _refused(pipe, "generate", NotImplementedError, "generate\\(\\) decodes one row within its cache")
    pipe.config["context_window"] = 96                                                  # the config key alike
    with pytest.raises(NotImplementedError, match="generate\\(\\) decodes one row"):
        pipe.generate(PROMPTS[0], max_tokens=8)
    pipe, _ = _pipe()
    _refused(pipe, "start_session/draft", NotImplementedError, "bonus-token emit mode")


@pytest.mark.parametrize("entry", BATCH)
def test_refusals_of_models_and_modes(entry):
    pipe, _ = _pipe()
    pipe.base_lm.kv_page_len = 32
    _refused(pipe, entry, NotImplementedError, "paged KV")
    pipe, _ = _pipe()
    pipe.draft_lm.config = SimpleNamespace(max_pos=1024, arch=1)
    _refused(pipe, entry, NotImplementedError, "GPT-2 model has learned positions")
    pipe, _ = _pipe("longest_prefix/adaptive")
    _refused(pipe, entry, NotImplementedError, "context_window keeps a fixed K")
    pipe, _ = _pipe("longest_prefix/adaptive_per_row")
    _refused(pipe, entry, NotImplementedError, "context_window keeps a fixed K")
    pipe, _ = _pipe()
    _refused(pipe, entry, NotImplementedError, "share_prefix / n are not supported with context_window", share_prefix=True)
    pipe, _ = _pipe()
    pipe.draft_lm.config = SimpleNamespace(max_pos=64)
    _refused(pipe, entry, ValueError, "exceeds the 64 positions of the smaller model")
    pipe, _ = _pipe()
    _refused(pipe, entry, ValueError, "too small for steps of K=4", context_window=40)
    pipe, _ = _pipe()
    _refused(pipe, entry, ValueError, "attention_sinks=-2", attention_sinks=-2)
    pipe, _ = _pipe(controller_params={"k": 1})                                          # K = 1: 8 positions of room, the window is a valid one
    _refused(pipe, entry, ValueError, "prompt of 24 tokens does not fit context_window=30", context_window=30, attention_sinks=0)


def test_refusals_of_the_other_routes():
    for name in ("typical", "rejection/host"):                                          # host-loop policies
        pipe, _ = _pipe(name)
        _refused(pipe, "generate_batch", NotImplementedError, "on the host loop is not supported with it")
    pipe, _ = _pipe("fake")
    _refused(pipe, "generate_batch", NotImplementedError, "implementation='fake' is not supported with it")
    pipe, _ = _pipe("fake")
    _refused(pipe, "start_session", NotImplementedError, "implementation='fake' is not supported with it")
    pipe, _ = _pipe("medusa_heads")                                                     # persistent heads draft from the target itself
    _refused(pipe, "generate_batch", NotImplementedError, "medusa / eagle / self-draft")
    pipe, _ = _pipe("eagle")
    with pytest.raises(NotImplementedError, match="medusa / eagle / self-draft"):
        pipe.start_session(PROMPTS, 300, 0, self_draft=True, context_window=96)
    pipe, _ = _pipe()
    _refused(pipe, "generate_batch", NotImplementedError, "share_prefix / n are not supported", n=2)
    with pytest.raises(NotImplementedError, match="needs the bonus-token HIP step"):    # a session made by hand, past the call's checks
        P.DecodeSession(pipe, PROMPTS, 300, 0, share_prefix=True, window=rolling.plan(96, 4, 4))


def test_admit_judges_a_prompt_by_the_window_not_the_budget():
    pipe, _ = _pipe()
    sess = object.__new__(P.DecodeSession)
    sess.window, sess.k, sess.max_tokens, sess.rt, sess.pos_limit = rolling.plan(96, 4, 4), 4, 10 ** 6, {"l_max": 128}, 128
    sess.rows = [SimpleNamespace(active=False)]
    with pytest.raises(ValueError, match="does not fit this session"):
        sess.admit(0, list(range(80)))
