"""policy "typical" / "topk_agree" with backend "device": what a call resolves to (the captured step, with the rule in its
StepOptions) and every refusal, over the stand-in pipeline of tests/call_route_cases.py; the flags of both CLIs. No device."""

import argparse

import pytest

import call_route_cases as C


def _stand_in(policy="typical", params=None, **kw):
    from src.specdec.core.acceptance import device_rule

    params = {"backend": "device", "p": 0.09, "delta": 0.3, "temperature": 0.7} if params is None else params
    pipe = C._stand_in(policy, dict(params), **kw)
    pipe.accept_device = device_rule(policy, params, kw.get("fake", False), pipe.base_lm.vocab_size)
    return pipe


def _resolve(pipe, prompts=None, do_sample=None, kwargs=None, **kw):
    from src.specdec.core.step_options import resolve

    return resolve(pipe, C.PROMPTS if prompts is None else prompts, None, None, do_sample, dict(kwargs or {}), **kw)


def test_the_rule_of_a_pipeline():
    from src.specdec.core.acceptance import DeviceRule, device_rule

    assert device_rule("typical", {"backend": "device", "p": 0.09, "delta": 0.3, "temperature": 0.7}, False) == DeviceRule("typical", 0.7, 0.09, 0.3)
    assert device_rule("typical", {"backend": "device"}, False) == DeviceRule("typical", 1.0, 0.9, None)          # the policy's p, T = 1, fixed threshold
    assert device_rule("typical", {"backend": "device", "delta": float("inf")}, False).delta is None
    assert device_rule("topk_agree", {"backend": "device", "k": 3}, False, 1000) == DeviceRule("topk_agree", k=3)
    assert device_rule("topk_agree", {"backend": "device"}, False).k == 5
    # without the backend, and for the policies whose device backend is somebody else's business: nothing
    for policy, params in (("typical", {"p": 0.5}), ("typical", None), ("topk_agree", {"backend": "host"}), ("rejection", {"backend": "device"}),
                           ("longest_prefix", {"backend": "device"})):
        assert device_rule(policy, params, False) is None
    with pytest.raises(NotImplementedError, match="not verification"):
        device_rule("conf_threshold", {"backend": "device"}, False)
    with pytest.raises(NotImplementedError, match="HIP engine"):
        device_rule("typical", {"backend": "device"}, True)
    for params, word in (({"p": 0.0}, "p="), ({"p": 1.5}, "p="), ({"delta": 0.0}, "delta"), ({"delta": -1}, "delta"), ({"temperature": 0}, "temperature"),
                         ({"temperature": float("nan")}, "temperature")):
        with pytest.raises(ValueError, match=word):
            device_rule("typical", dict(params, backend="device"), False)
    for k in (0, -2, 2.5, 1001):
        with pytest.raises(ValueError, match="k="):
            device_rule("topk_agree", {"backend": "device", "k": k}, False, 1000)


@pytest.mark.parametrize("entry", ["generate_batch", "generate_many"])
def test_calls_take_the_step_route_with_the_rule(entry):
    routes = {"policy_routes": entry == "generate_batch"}
    call = _resolve(_stand_in(), **routes)
    o = call.options
    assert call.route == "step" and not call.self_draft
    assert (o.mode, o.accept_rule, o.accept_temperature, o.accept_epsilon, o.accept_delta) == ("greedy", "typical", 0.7, 0.09, 0.3)
    assert o.processors is None and o.fsm is None and o.row_params is None
    # do_sample chooses how the token after the accepted prefix is drawn; the rule stays
    o = _resolve(_stand_in(), do_sample=True, kwargs={"top_k": 20, "top_p": 0.9, "seed": 5}, **routes).options
    assert (o.mode, o.top_k, o.top_p, o.seed, o.accept_rule) == ("sampled", 20, 0.9, 5, "typical")
    o = _resolve(_stand_in("topk_agree", {"backend": "device", "k": 2}), **routes).options
    assert (o.mode, o.accept_rule, o.accept_k) == ("greedy", "topk_agree", 2)
    # what only needs the captured step keeps working: share_prefix / n, logit processors, grammars
    call = _resolve(_stand_in(), share_prefix=True, n=2, **routes)
    assert call.share_prefix and len(call.prompts) == 2 * len(C.PROMPTS) and call.options.accept_rule == "typical"
    o = _resolve(_stand_in(), kwargs={"bad_token_ids": [3, 9], "repetition_penalty": 1.2}, grammar=C.automata()["A"], **routes).options
    assert o.processors is not None and o.processors.rp == 1.2 and o.fsm is C.automata()["A"] and o.accept_rule == "typical"


def test_the_host_loop_keeps_its_route():
    call = _resolve(C._stand_in("typical"))
    assert call.route == "host_policy" and call.options.accept_rule is None


def test_start_session_carries_the_rule(monkeypatch):
    from src.specdec.core import pipeline as P

    seen = []
    monkeypatch.setattr(P, "DecodeSession", lambda *a, **kw: seen.append(a) or "session")
    pipe = _stand_in()
    assert pipe.start_session(C.PROMPTS, 16, 0) == "session"
    assert seen[-1][4].accept_rule == "typical" and seen[-1][4].mode == "greedy"
    pipe.start_session(C.PROMPTS, 16, 0, {"temperature": 0.9, "top_k": 20, "top_p": None, "seed": 3}, bad_token_ids=[4])
    o = seen[-1][4]
    assert (o.mode, o.accept_rule, o.top_k) == ("sampled", "typical", 20) and o.processors is not None
    with pytest.raises(NotImplementedError, match="bonus-token emit mode"):
        pipe.start_session(C.PROMPTS, 16, 1)
    with pytest.raises(NotImplementedError, match="sampling_params"):
        pipe.start_session(C.PROMPTS, 16, 0, sampling_params=C._ROWS["plain"]())
    with pytest.raises(NotImplementedError, match="draft-model mode"):
        pipe.start_session(C.PROMPTS, 16, 0, self_draft=True)
    with pytest.raises(NotImplementedError, match="speculative sampling"):
        pipe.start_session(C.PROMPTS, 16, 0, {"spec": True, "temperature": 1.0, "top_k": None, "top_p": None, "seed": 0})
    # a pipeline without a device rule: start_session is what it was
    C._stand_in().start_session(C.PROMPTS, 16, 1)
    assert seen[-1][4].accept_rule is None


def test_every_refusal_names_its_reason():
    with pytest.raises(NotImplementedError, match="sampling_params are not supported with policy='typical' on the device"):
        _resolve(_stand_in(), sampling_params=C._ROWS["plain"]())
    with pytest.raises(NotImplementedError, match="sampling_params"):
        _resolve(_stand_in(), sampling_params=C._ROWS["plain"](), policy_routes=False)
    with pytest.raises(NotImplementedError, match="adaptive K is not supported"):
        _resolve(_stand_in(controller="adaptive", controller_params=C._ADAPTIVE))
    with pytest.raises(NotImplementedError, match="adaptive K is not supported"):
        _resolve(_stand_in(controller="adaptive", controller_params=dict(C._ADAPTIVE, per_row=True)), policy_routes=False)
    for kw in ({"draft_mode": "medusa", "draft": False, "heads": True}, {"draft_mode": "eagle", "draft": False}):
        with pytest.raises(NotImplementedError, match="medusa / eagle"):
            _resolve(_stand_in(**kw))
    with pytest.raises(NotImplementedError, match=r"generate\(\) emits no such token"):
        _resolve(_stand_in(), prompts=[C.PROMPTS[0]], single=True)
    with pytest.raises(NotImplementedError, match=r"generate\(\)"):
        _stand_in("topk_agree", {"backend": "device", "k": 1}).generate(C.PROMPTS[0])


def _ns(**kw):
    base = dict(policy="typical", policy_backend="device", typical_epsilon=None, typical_delta=None, temperature=None)
    return argparse.Namespace(**dict(base, **kw))


def test_cli_flags():
    from src.specdec.run_specdec import device_policy_params, parse_args
    from src.specdec_cli.main import build_parser

    a = parse_args(["--prompt", "x", "--policy", "typical", "--policy-backend", "device", "--typical-epsilon", "0.09", "--typical-delta", "0.3",
                    "--temperature", "0.7"])
    assert device_policy_params(a) == {"backend": "device", "p": 0.09, "delta": 0.3, "temperature": 0.7}
    a = parse_args(["--prompt", "x", "--policy", "topk_agree", "--policy-backend", "device", "--policy-k", "3"])
    assert device_policy_params(a) == {"backend": "device"} and a.policy_k == 3
    assert device_policy_params(parse_args(["--prompt", "x", "--policy", "typical", "--policy-p", "0.5"])) == {}       # the host loop, as before
    assert device_policy_params(_ns()) == {"backend": "device"}
    for ns, word in ((_ns(policy_backend="host", typical_delta=0.3), "belong to"), (_ns(policy="longest_prefix"), "belongs to"),
                     (_ns(policy="conf_threshold"), "belongs to"), (_ns(policy="topk_agree", typical_epsilon=0.1), "--policy typical")):
        with pytest.raises(ValueError, match=word):
            device_policy_params(ns)
    r = build_parser().parse_args(["run", "--policy", "typical", "--policy-backend", "device", "--typical-epsilon", "0.09", "--typical-delta",
                                   "0.3", "a prompt"])
    assert (r.policy, r.policy_backend, r.typical_epsilon, r.typical_delta) == ("typical", "device", 0.09, 0.3)
    assert device_policy_params(r) == {"backend": "device", "p": 0.09, "delta": 0.3, "temperature": 0.7}
    r = build_parser().parse_args(["run", "--policy", "topk_agree", "--policy-backend", "device", "--policy-k", "2", "a prompt"])
    assert (r.policy, r.policy_k) == ("topk_agree", 2)
    assert build_parser().parse_args(["run", "a prompt"]).policy == "longest_prefix"
