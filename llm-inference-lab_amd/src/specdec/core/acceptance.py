"""Lossy acceptance on the device: policy="typical" / "topk_agree" with policy_params["backend"] = "device" (csrc/typical_accept.hip,
sd_specdec_set_acceptance). `device_rule` reads the policy's parameters once, when the pipeline is made; `refuse_call` and
`session_rule` hold what a call or a session cannot combine with it; `with_rule` puts the rule into a call's StepOptions.

The rule judges d_{i+1} on the target's distribution AFTER d_1..d_i — the rows of the K+1-token verify pass. The host loop behind the
same policy names without the backend (SpeculativePipeline._decode_host_policy) judges it on the target's own greedy continuation."""

import math
from dataclasses import dataclass, replace
from typing import Any, Dict, Optional

RULES = ("typical", "topk_agree")


@dataclass(frozen=True)
class DeviceRule:
    """rule "typical": keep d iff p(d) >= min(epsilon, delta * exp(-H(p))) at `temperature` (delta None: the fixed threshold epsilon);
    rule "topk_agree": keep d iff it is among the k largest logits of the row."""
    rule: str
    temperature: float = 1.0
    epsilon: float = 0.09
    delta: Optional[float] = None
    k: int = 1


def device_rule(policy: str, policy_params: Optional[Dict[str, Any]], fake: bool, vocab: Optional[int] = None) -> Optional[DeviceRule]:
    """The rule of a pipeline made with (policy, policy_params), None when the device backend is not asked for or belongs to another
    policy (the caller's own checks). typical: p = epsilon (the policy's default 0.9), delta (None: fixed threshold), temperature
    (default 1.0); topk_agree: k (the policy's default 5)."""
    params = dict(policy_params or {})
    if str(params.get("backend", "host")) != "device":
        return None
    if policy == "conf_threshold":
        raise NotImplementedError("policy='conf_threshold' has no backend='device': it judges a draft token by the DRAFT's own confidence "
                                  "and needs no target distribution, so it is not verification (the device rules are 'typical' and "
                                  "'topk_agree', which judge it on the target's verify rows)")
    if policy not in RULES:
        return None
    if fake:
        raise NotImplementedError(f"policy={policy!r} with backend='device' needs the HIP engine (implementation='hip')")
    if policy == "topk_agree":
        k = params.get("k", 5)
        if isinstance(k, bool) or int(k) != k or int(k) < 1 or (vocab is not None and int(k) > vocab):
            raise ValueError(f"policy='topk_agree' (backend='device'): k={k!r} (an integer in 1..V)")
        return DeviceRule("topk_agree", k=int(k))
    eps, delta, t = float(params.get("p", 0.9)), params.get("delta"), float(params.get("temperature", 1.0))
    if not 0.0 < eps <= 1.0:
        raise ValueError(f"policy='typical' (backend='device'): p={eps} (the threshold epsilon, in (0, 1])")
    if delta is not None and not float(delta) > 0.0:
        raise ValueError(f"policy='typical' (backend='device'): delta={delta} (must be > 0; None = the fixed threshold p)")
    if not (t > 0.0 and math.isfinite(t)):
        raise ValueError(f"policy='typical' (backend='device'): temperature={t} (must be > 0)")
    return DeviceRule("typical", t, eps, None if delta is None or math.isinf(float(delta)) else float(delta))


def refuse_call(pipe, single: bool, sampling_params) -> None:
    """What generate / generate_batch / generate_many cannot combine with the device rule (adaptive K and the draft modes are gated
    by the caller, step_options.gate)."""
    name = pipe.policy_name
    if single:
        raise NotImplementedError(f"policy={name!r} with backend='device' belongs to generate_batch, generate_many and start_session: the rule "
                                  "emits the target's token after the accepted prefix every step, and generate() emits no such token")
    if sampling_params is not None:
        raise NotImplementedError(f"sampling_params are not supported with policy={name!r} on the device: the rule's parameters are the "
                                  "loop's, and the step reads no row table next to it (give do_sample / temperature / top_k / top_p / seed "
                                  "for the call)")


def with_rule(options, rule: DeviceRule):
    """`options` with the rule's fields; the mode stays what the call's sampling made it (greedy: the target's argmax follows the accepted
    prefix; sampled: a draw)."""
    return replace(options, accept_rule=rule.rule, accept_temperature=rule.temperature, accept_epsilon=rule.epsilon, accept_delta=rule.delta,
                   accept_k=rule.k)


def session_rule(pipe, options, emit_mode: int, self_draft: bool, sampling_params, bonus_mode: int):
    """start_session on a pipeline with a device rule: the options with the rule, or the refusal."""
    rule = getattr(pipe, "accept_device", None)
    if rule is None:
        return options
    name = pipe.policy_name
    refuse_call(pipe, False, sampling_params)
    if emit_mode != bonus_mode:
        raise NotImplementedError(f"policy={name!r} with backend='device' needs the bonus-token emit mode (generate_batch): the draft-emit "
                                  "mode emits no token of the target's after the accepted prefix")
    if self_draft:
        raise NotImplementedError(f"policy={name!r} with backend='device' needs the draft-model mode (draft_mode='vanilla'): medusa / eagle "
                                  "proposals are not judged by it")
    if options.mode == "spec" or options.row_params is not None:
        raise NotImplementedError(f"policy={name!r} with backend='device': speculative sampling and per-request parameters have no place next "
                                  "to the rule")
    return with_rule(options, rule)
