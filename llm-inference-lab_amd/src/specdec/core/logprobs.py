"""Per-token log-probs: logprobs=N on generate_batch, generate_many and start_session, and best_of on generate_batch
(csrc/token_logprobs.hip, sd_specdec_set_logprobs). `with_logprobs` puts a call's request into its StepOptions, `session_logprobs`
does it for start_session and `check_session` holds what a DecodeSession cannot combine with it; every refusal of the feature is
raised here. Where the run must be the captured step with a draft model and a fixed K is step_options' table (`gate`, feature
"logprobs").

The numbers are computed inside the step that emits the token, from the verify row the token was checked against or drawn from (the
processed row under logit processors and grammars, at temperature 1, before top-k / top-p shaping), and arrive with the step record.
The host rules that cut, strip and delete tokens (SpeculativePipeline._rules_batch) apply every such edit to a parallel payload of
`TokenInfo`, so entry j of a row's token_info is the record of generated[j]."""

from collections import namedtuple
from dataclasses import replace
from typing import Any, Dict, List, Optional

MAX_TOP = 20

# what the device said about one emitted token: top = [(id, logprob)] * N, the row's N largest entries
TokenInfo = namedtuple("TokenInfo", "token logprob rank top")


def check_logprobs(logprobs) -> Optional[int]:
    """The top_n a call's `logprobs` asks for: None / False -> None (not asked), True / 0 -> 0 (the chosen token's log-prob only),
    1..20 -> that many alternatives as well; anything else is the ValueError."""
    if logprobs is None or logprobs is False:
        return None
    if logprobs is True:
        return 0
    if not isinstance(logprobs, int) or not 0 <= logprobs <= MAX_TOP:
        raise ValueError(f"logprobs={logprobs!r} (True, or an integer in 0..{MAX_TOP})")
    return int(logprobs)


def with_logprobs(pipe, options, logprobs, captured_step: bool = True, what: str = "", self_draft: bool = False, single: bool = False):
    """`options` with the per-token log-probs a call or a session asks for (None: not asked), every refusal raised."""
    from .step_options import gate

    top_n = check_logprobs(logprobs)
    if top_n is None:
        return options
    if single:
        raise NotImplementedError("logprobs belong to generate_batch, generate_many and start_session: generate() emits the draft's own "
                                  "tokens, and the log-prob stage describes the target's (the bonus-token emit mode)")
    gate(pipe, "logprobs", captured_step, what, self_draft)
    if options.draft_confidence is not None:
        raise NotImplementedError("logprobs are not supported with draft_confidence: the confidence-gated step keeps itself apart")
    return replace(options, logprobs=top_n)


def session_logprobs(pipe, options, emit_mode: int, self_draft: bool, logprobs, bonus_mode: int):
    """start_session with logprobs: the options with it, or the refusal (the caller has chosen the route: only the mode is judged)."""
    if check_logprobs(logprobs) is not None and emit_mode != bonus_mode:
        raise NotImplementedError("logprobs need the bonus-token emit mode (generate_batch): the draft-emit mode (EMIT_DRAFT) emits the "
                                  "draft's own tokens")
    return with_logprobs(pipe, options, logprobs, not pipe._fake, "implementation='fake'", self_draft)


def check_session(options, other_step: bool, bonus: bool) -> Optional[int]:
    """The top_n a DecodeSession's options ask for (None: off), after what the session itself cannot give it: other_step = no draft
    model, the fake double, or a K that moves; bonus = the bonus-token emit mode."""
    if options.logprobs is None:
        return None
    if other_step or not bonus or options.draft_confidence is not None:
        raise NotImplementedError("logprobs need the bonus-token HIP step with a draft model and a fixed K, and have no place next to "
                                  "draft_confidence")
    return int(options.logprobs)


def step_payload(rec, b: int, width: int) -> List[Optional[TokenInfo]]:
    """Row b's payload of one step record, parallel to the step's tokens t[0..width): entry i < n_new is what the device computed for
    new_tokens[b][i] at verify row i, the others are None (nothing was emitted there, and the rules read no such position)."""
    n_new = int(rec.n_new[b])
    out: List[Optional[TokenInfo]] = [None] * width
    for i in range(min(n_new, width)):
        top = [(int(t), float(lp)) for t, lp in zip(rec.top_ids[b, i], rec.top_logprobs[b, i])]
        out[i] = TokenInfo(int(rec.new_tokens[b][i]), float(rec.logprob[b, i]), int(rec.rank[b, i]), top)
    return out


def redraw_payload(logits_row, token: int, top_n: int) -> TokenInfo:
    """The payload of a token the HOST redrew at another verify row (an EOS-cut full acceptance in sampled-bonus mode): the same
    device function on that row (specdec_hip.ops.token_logprobs), on the current stream."""
    from specdec_hip.ops import token_logprobs

    out = token_logprobs(logits_row.unsqueeze(0), [int(token)], top_n)
    lp, rank = float(out.logprob.item()), int(out.rank.item())
    top = [(int(t), float(x)) for t, x in zip(out.top_ids[0].tolist(), out.top_logprobs[0].tolist())]
    return TokenInfo(int(token), lp, rank, top)


def result_fields(row, top_n: Optional[int]) -> Dict[str, Any]:
    """What a result dict gains: logprobs, token_ranks, top_logprobs (when alternatives were asked) and cumulative_logprob — the
    Python float sum in emission order. {} while the mode is off."""
    if top_n is None:
        return {}
    info = row.token_info
    if len(info) != len(row.generated) or any(e.token != g for e, g in zip(info, row.generated)):
        raise RuntimeError("token_info is out of step with the generated tokens")
    out = {"logprobs": [e.logprob for e in info], "token_ranks": [e.rank for e in info]}
    if top_n > 0:
        out["top_logprobs"] = [list(e.top) for e in info]
    total = 0.0
    for e in info:
        total += e.logprob
    out["cumulative_logprob"] = total
    return out


def check_best_of(best_of, n: int) -> Optional[int]:
    """best_of of a generate_batch call: None -> None; an integer m >= n, else the ValueError."""
    if best_of is None:
        return None
    if isinstance(best_of, bool) or not isinstance(best_of, int) or best_of < int(n) or best_of < 1:
        raise ValueError(f"best_of={best_of!r} (an integer >= n = {n})")
    return int(best_of)


def pick_best(results: List[Dict[str, Any]], m: int, n: int) -> List[Dict[str, Any]]:
    """Prompt-major results of m rows per prompt -> the n with the highest cumulative_logprob per prompt, best first; ties go to the
    lower row index."""
    out = []
    for p in range(0, len(results), m):
        group = results[p:p + m]
        order = sorted(range(len(group)), key=lambda j: (-group[j]["cumulative_logprob"], j))
        out.extend(group[j] for j in order[:n])
    return out


def check_best_of_mode(options) -> None:
    """best_of needs rows that differ: a sampling mode (do_sample, rejection on the device, or sampling_params)."""
    if options.mode == "greedy":
        raise ValueError("best_of needs a sampling mode (do_sample=True, policy='rejection' with backend='device', or sampling_params): "
                         "greedy rows of one prompt are all equal")


def refuse_best_of(kwargs) -> None:
    """generate_many has no best_of."""
    if kwargs.pop("best_of", None) is not None:
        raise NotImplementedError("best_of belongs to generate_batch: generate_many hands slots to prompts one at a time and ranks nothing")
