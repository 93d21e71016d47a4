"""logprobs= / best_of= on the host, before anything touches the device: every refusal with its message, every allowed combination
resolved with options.logprobs set, and the best_of validations — with the stand-in pipelines of tests/call_route_cases.py."""

import pytest

import call_route_cases as C


def _resolve(pipe, prompts=None, do_sample=None, kwargs=None, **kw):
    from src.specdec.core.step_options import resolve

    return resolve(pipe, C.PROMPTS if prompts is None else prompts, None, None, do_sample, dict(kwargs or {}), **kw)


def _device_rule_stand_in(policy="typical", params=None):
    from src.specdec.core.acceptance import device_rule

    params = {"backend": "device", "p": 0.09, "delta": 0.3, "temperature": 0.7} if params is None else params
    pipe = C._stand_in(policy, dict(params))
    pipe.accept_device = device_rule(policy, params, False, pipe.base_lm.vocab_size)
    return pipe


def test_the_argument():
    from src.specdec.core.logprobs import check_logprobs

    assert check_logprobs(None) is None and check_logprobs(False) is None
    assert check_logprobs(True) == 0 and check_logprobs(0) == 0 and check_logprobs(1) == 1 and check_logprobs(20) == 20
    for bad in (-1, 21, 2.0, "5", [5]):
        with pytest.raises(ValueError, match="logprobs="):
            check_logprobs(bad)
    from src.specdec.core.step_options import _GATE, StepOptions

    assert StepOptions().logprobs is None and "logprobs" in _GATE


@pytest.mark.parametrize("entry", ["generate_batch", "generate_many"])
def test_allowed_combinations_resolve_with_the_option(entry):
    routes = {"policy_routes": entry == "generate_batch"}
    A = C.automata()["A"]
    o = _resolve(C._stand_in(), logprobs=5, **routes)
    assert o.route == "step" and (o.options.mode, o.options.logprobs) == ("greedy", 5)
    assert _resolve(C._stand_in(), logprobs=True, **routes).options.logprobs == 0
    assert _resolve(C._stand_in(), logprobs=0, **routes).options.logprobs == 0
    assert _resolve(C._stand_in(), **routes).options.logprobs is None
    assert _resolve(C._stand_in(), logprobs=False, **routes).options.logprobs is None
    o = _resolve(C._stand_in(), do_sample=True, kwargs={"top_k": 20, "seed": 3}, logprobs=20, **routes).options
    assert (o.mode, o.top_k, o.logprobs) == ("sampled", 20, 20)
    o = _resolve(C._stand_in(), kwargs={"bad_token_ids": [3, 9], "repetition_penalty": 1.2}, grammar=A, logprobs=2, **routes).options
    assert o.processors is not None and o.fsm is A and o.logprobs == 2
    o = _resolve(C._stand_in(), sampling_params=C._ROWS["penalties"](), logprobs=1, **routes).options
    assert o.row_params is not None and o.logprobs == 1
    call = _resolve(C._stand_in(), do_sample=True, share_prefix=True, n=2, logprobs=3, **routes)
    assert call.share_prefix and len(call.prompts) == 2 * len(C.PROMPTS) and call.options.logprobs == 3
    # the device acceptance rules, greedy and with the sampled token after the accepted prefix
    o = _resolve(_device_rule_stand_in(), logprobs=5, **routes).options
    assert (o.accept_rule, o.mode, o.logprobs) == ("typical", "greedy", 5)
    o = _resolve(_device_rule_stand_in("topk_agree", {"backend": "device", "k": 2}), do_sample=True, logprobs=5, **routes).options
    assert (o.accept_rule, o.mode, o.logprobs) == ("topk_agree", "sampled", 5)


def test_rejection_on_the_device_resolves_with_the_option():
    for name in ("rejection/device", "rejection/device_shaped"):
        o = _resolve(C.STAND_INS[name](), logprobs=4).options
        assert (o.mode, o.logprobs) == ("spec", 4)
    o = _resolve(C.STAND_INS["rejection/device"](), sampling_params=C._ROWS["plain"](), logprobs=4).options
    assert o.mode == "spec" and o.row_params is not None and o.logprobs == 4


def test_every_refusal_fires_with_its_message():
    # the host loops
    for name in ("typical", "rejection/host"):
        with pytest.raises(NotImplementedError, match="logprobs are computed inside the captured device step: policy=.* on the host loop"):
            _resolve(C.STAND_INS[name](), logprobs=5)
    # the fake double: generate_batch (which falls back to generate() per prompt) and generate_many
    with pytest.raises(NotImplementedError, match="logprobs are computed inside the captured device step: implementation='fake'"):
        _resolve(C.STAND_INS["fake"](), logprobs=5)
    with pytest.raises(NotImplementedError, match="implementation='fake' is not supported"):
        _resolve(C.STAND_INS["fake"](), logprobs=5, policy_routes=False)
    # medusa heads (a loop without a draft model)
    with pytest.raises(NotImplementedError, match="logprobs need the draft-model mode"):
        _resolve(C.STAND_INS["medusa_heads"](), logprobs=5)
    # adaptive K, both kinds
    for name, routes in (("longest_prefix/adaptive", True), ("longest_prefix/adaptive_per_row", True), ("longest_prefix/adaptive_per_row", False),
                         ("rejection/device_adaptive", True)):
        with pytest.raises(NotImplementedError, match="adaptive K is not supported"):
            _resolve(C.STAND_INS[name](), logprobs=5, policy_routes=routes)
    # generate()
    with pytest.raises(NotImplementedError, match=r"logprobs belong to generate_batch, generate_many and start_session: generate\(\)"):
        _resolve(C._stand_in(), prompts=[C.PROMPTS[0]], single=True, logprobs=5)
    with pytest.raises(NotImplementedError, match=r"generate\(\)"):
        C._stand_in().generate(C.PROMPTS[0], logprobs=5)
    # draft_confidence, from the call and from the config
    with pytest.raises(NotImplementedError, match="logprobs are not supported with draft_confidence"):
        _resolve(C._stand_in(), draft_confidence=0.5, logprobs=5)
    pipe = C._stand_in()
    pipe.config["draft_confidence_threshold"] = 0.5
    with pytest.raises(NotImplementedError, match="logprobs are not supported with draft_confidence"):
        _resolve(pipe, logprobs=5)
    # a value that is no top_n
    with pytest.raises(ValueError, match="logprobs=21"):
        _resolve(C._stand_in(), logprobs=21)


def test_start_session(monkeypatch):
    from src.specdec.core import pipeline as P

    seen = []
    monkeypatch.setattr(P, "DecodeSession", lambda *a, **kw: seen.append(a) or "session")
    pipe = C._stand_in()
    assert pipe.start_session(C.PROMPTS, 16, 0, logprobs=5) == "session" and seen[-1][4].logprobs == 5
    pipe.start_session(C.PROMPTS, 16, 0, {"temperature": 0.9, "top_k": 20, "top_p": None, "seed": 3}, bad_token_ids=[4], logprobs=True)
    assert (seen[-1][4].mode, seen[-1][4].logprobs) == ("sampled", 0) and seen[-1][4].processors is not None
    pipe.start_session(C.PROMPTS, 16, 0)
    assert seen[-1][4].logprobs is None
    with pytest.raises(NotImplementedError, match=r"EMIT_DRAFT"):
        pipe.start_session(C.PROMPTS, 16, 1, logprobs=5)
    pipe.start_session(C.PROMPTS, 16, 1)                                   # the draft-emit mode without it is what it was
    with pytest.raises(NotImplementedError, match="logprobs need the draft-model mode"):
        C.STAND_INS["eagle"]().start_session(C.PROMPTS, 16, 0, self_draft=True, logprobs=5)
    with pytest.raises(NotImplementedError, match="logprobs need the draft-model mode"):
        pipe.start_session(C.PROMPTS, 16, 0, self_draft=True, logprobs=5)
    with pytest.raises(NotImplementedError, match="implementation='fake'"):
        C.STAND_INS["fake"]().start_session(C.PROMPTS, 16, 0, logprobs=5)
    with pytest.raises(NotImplementedError, match="draft_confidence"):
        pipe.start_session(C.PROMPTS, 16, 0, draft_confidence=0.5, logprobs=5)


def test_a_session_refuses_what_it_cannot_give():
    """DecodeSession's own check, for options built by hand"""
    from src.specdec.core.logprobs import check_session
    from src.specdec.core.step_options import StepOptions

    assert check_session(StepOptions(), False, True) is None
    assert check_session(StepOptions(logprobs=0), False, True) == 0 and check_session(StepOptions(logprobs=7), False, True) == 7
    for other_step, bonus, o in ((True, True, StepOptions(logprobs=5)), (False, False, StepOptions(logprobs=5)),
                                 (False, True, StepOptions(logprobs=5, draft_confidence=0.5))):
        with pytest.raises(NotImplementedError, match="logprobs need the bonus-token HIP step"):
            check_session(o, other_step, bonus)


def test_best_of_validations(monkeypatch):
    pipe = C._stand_in()
    seen = []

    def decode(ids, *a, **kw):
        seen.append((ids, kw["options"]))
        raise C._Handoff
    pipe._decode = decode
    with pytest.raises(ValueError, match="best_of=1 .*>= n = 2"):
        pipe.generate_batch(C.PROMPTS, do_sample=True, n=2, best_of=1)
    for bad in (0, 2.5, True, "4"):
        with pytest.raises(ValueError, match="best_of="):
            pipe.generate_batch(C.PROMPTS, do_sample=True, best_of=bad)
    with pytest.raises(ValueError, match="best_of needs a sampling mode"):
        pipe.generate_batch(C.PROMPTS, n=2, best_of=4)
    with pytest.raises(NotImplementedError, match="best_of belongs to generate_batch"):
        pipe.generate_many(C.PROMPTS, do_sample=True, best_of=4)
    assert not seen
    # allowed: m rows per prompt through the n machinery, logprobs implied (0) or kept as asked
    with pytest.raises(C._Handoff):
        pipe.generate_batch(C.PROMPTS, do_sample=True, n=2, best_of=4)
    assert len(seen[-1][0]) == 4 * len(C.PROMPTS) and seen[-1][1].logprobs == 0 and seen[-1][1].mode == "sampled"
    with pytest.raises(C._Handoff):
        pipe.generate_batch(C.PROMPTS, do_sample=True, best_of=3, logprobs=5)
    assert len(seen[-1][0]) == 3 * len(C.PROMPTS) and seen[-1][1].logprobs == 5
    # and refused where logprobs are: the host loops
    with pytest.raises(NotImplementedError, match="logprobs are computed inside the captured device step"):
        C.STAND_INS["rejection/host"]().generate_batch(C.PROMPTS, best_of=1)
    with pytest.raises(NotImplementedError, match="share_prefix / n need the captured device step"):      # (m rows are n rows)
        C.STAND_INS["rejection/host"]().generate_batch(C.PROMPTS, best_of=2)


def test_pick_best_orders_by_cumulative_logprob_then_row():
    from src.specdec.core.logprobs import pick_best

    rows = [{"cumulative_logprob": x, "row": i} for i, x in enumerate([-3.0, -1.0, -1.0, -2.0, -9.0, -8.0, -8.5, -7.0])]
    got = pick_best(rows, 4, 2)
    assert [r["row"] for r in got] == [1, 2, 7, 5]
    assert [r["row"] for r in pick_best(rows, 4, 4)] == [1, 2, 3, 0, 7, 5, 6, 4]


def test_result_fields():
    from types import SimpleNamespace

    from src.specdec.core.logprobs import TokenInfo, result_fields

    row = SimpleNamespace(generated=[7, 8], token_info=[TokenInfo(7, -0.5, 0, [(7, -0.5), (1, -2.0)]), TokenInfo(8, -1.25, 1, [(3, -0.75), (8, -1.25)])])
    assert result_fields(row, None) == {}
    got = result_fields(row, 0)
    assert got == {"logprobs": [-0.5, -1.25], "token_ranks": [0, 1], "cumulative_logprob": -1.75}
    got = result_fields(row, 2)
    assert got["top_logprobs"] == [[(7, -0.5), (1, -2.0)], [(3, -0.75), (8, -1.25)]]
    row.generated = [7, 9]
    with pytest.raises(RuntimeError, match="out of step"):
        result_fields(row, 0)
