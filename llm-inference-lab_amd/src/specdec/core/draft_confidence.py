"""Confidence-gated draft length: draft_confidence=tau / draft_min_k= on generate_batch, generate_many and start_session
(csrc/draft_confidence.hip, sd_specdec_set_draft_confidence; HF assisted generation's assistant_confidence_threshold). `with_confidence`
puts a call's threshold into its StepOptions, `session_confidence` does it for start_session and `check_session` holds what a
DecodeSession cannot combine with it; every refusal of the feature is raised here. Where the run must be the captured step with a
draft model and a fixed K is step_options' table (`gate`, feature "draft_confidence").

A row stops drafting after the first draft forward i + 1 >= draft_min_k whose confidence — the draft's softmax probability of its own
token — is below tau; the token drawn at low confidence is still proposed. The device decides between two draft forwards and starts
every step at K again: the host takes a row's k from the step record and mirrors nothing."""

from dataclasses import replace
from typing import Tuple

# what the confidence-gated step has no place next to (StepOptions predicate, the refusal)
CLASHES = (
    (lambda o: o.mode == "spec", "draft_confidence is not supported with speculative sampling (policy='rejection' on the device): it keeps a fixed K"),
    (lambda o: o.accept_rule is not None, "draft_confidence is not supported with policy 'typical' / 'topk_agree' on the device: the rule keeps a fixed K"),
    (lambda o: o.row_params is not None, "draft_confidence is not supported with sampling_params: the step reads no row table next to it"),
    (lambda o: o.fsm is not None, "draft_confidence is not supported with a grammar: the masked draft rows keep a fixed K"),
    (lambda o: o.processors is not None, "draft_confidence is not supported with logit processors (penalties, logit_bias, token bans): the "
                                         "processed draft rows keep a fixed K"),
)


def check_confidence(tau, min_k) -> Tuple[float, int]:
    """(tau, min_k) of a call as the library takes them, or the ValueError: tau in (0, 1], min_k an integer >= 1 (None: 1)."""
    if isinstance(tau, bool) or not isinstance(tau, (int, float)) or not 0.0 < float(tau) <= 1.0:      # (a NaN compares false)
        raise ValueError(f"draft_confidence={tau!r} (a threshold in (0, 1])")
    min_k = 1 if min_k is None else min_k
    if isinstance(min_k, bool) or not isinstance(min_k, (int, float)) or int(min_k) != min_k or int(min_k) < 1:
        raise ValueError(f"draft_min_k={min_k!r} (an integer in 1..K)")
    return float(tau), int(min_k)


def with_confidence(pipe, options, tau, min_k, captured_step: bool = True, what: str = "", self_draft: bool = False, single: bool = False):
    """`options` with the confidence-gated draft length a call or a session asks for (tau None: not asked), every refusal raised."""
    from .step_options import gate

    if tau is None:
        if min_k is not None:
            raise ValueError("draft_min_k belongs to draft_confidence: give the threshold as well")
        return options
    if single:
        raise NotImplementedError("draft_confidence belongs to generate_batch, generate_many and start_session: generate() emits the draft's "
                                  "own tokens, and the confidence-gated step emits the target's (the bonus-token emit mode)")
    tau, min_k = check_confidence(tau, min_k)
    gate(pipe, "draft_confidence", captured_step, what, self_draft)
    for clash, message in CLASHES:
        if clash(options):
            raise NotImplementedError(message)
    return replace(options, draft_confidence=tau, draft_min_k=min_k)


def session_confidence(pipe, options, emit_mode: int, self_draft: bool, tau, min_k, bonus_mode: int):
    """start_session with draft_confidence: the options with it, or the refusal (the caller has chosen the route: only the mode is judged)."""
    if tau is not None and emit_mode != bonus_mode:
        raise NotImplementedError("draft_confidence needs the bonus-token emit mode (generate_batch): the draft-emit mode emits the draft's "
                                  "own tokens")
    return with_confidence(pipe, options, tau, min_k, not pipe._fake, "implementation='fake'", self_draft)


def check_session(options, other_step: bool, bonus: bool, k: int) -> bool:
    """Whether a DecodeSession's options ask for the mode, after what the session itself cannot give it: other_step = no draft model, the
    fake double, or a K that moves; bonus = the bonus-token emit mode; k = the step's shape."""
    if options.draft_confidence is None:
        return False
    if other_step or not bonus or any(clash(options) for clash, _ in CLASHES):
        raise NotImplementedError("draft_confidence needs the bonus-token HIP step with a draft model and a fixed K, and has no place next "
                                  "to speculative sampling, a device acceptance rule, logit processors, grammars or sampling_params")
    if options.draft_min_k > k:
        raise ValueError(f"draft_min_k={options.draft_min_k} exceeds the step's K ({k})")
    return True
