"""What a call asks of the step, resolved once: `StepOptions`, the gate of the captured step's features, and `resolve`. Nothing here
touches the device and the pipeline is read through attributes only: a stand-in drives all of it on the CPU (tests/call_route_cases.py)."""

import math
from collections import namedtuple
from dataclasses import dataclass, replace
from typing import Any, ClassVar, Dict, List, Optional, Sequence, Tuple

import torch
from specdec_hip.grammar import TokenFSM
from specdec_hip.sampling_params import SamplingParams, check_penalties

from ..policies.controllers import FixedKController
from .acceptance import refuse_call, with_rule
from .draft_confidence import with_confidence
from .logprobs import with_logprobs

PROCESSOR_KEYS = ("repetition_penalty", "presence_penalty", "frequency_penalty", "logit_bias", "bad_token_ids", "allowed_token_ids")
ROW_SAMPLING_CLASH = ("top_k", "top_p", "repetition_penalty", "presence_penalty", "frequency_penalty")


@dataclass(frozen=True)
class Processors:
    """A run's logit-processor stage: the penalties, and `bias`, the one additive float32 [V] host table that logit_bias, banned and
    allowed ids all come down to (-inf bans), or None."""
    rp: float = 1.0
    presence: float = 0.0
    frequency: float = 0.0
    bias: Any = None
    IDENTITY: ClassVar["Processors"]       # the stage switched on with nothing to do by itself (a grammar, per-request penalties)


Processors.IDENTITY = Processors()


@dataclass(frozen=True)
class StepOptions:
    """What a session's step does. mode: "greedy", "sampled" (the bonus token is drawn) or "spec" (speculative sampling), with
    the run's scalars; row_params: every row's own SamplingParams, seeds resolved (None: the scalars rule); row_ids: every
    row's Philox stream id (None: its index); processors: None = the stage is off; fsm: the one table the device walks, with
    grammar_starts = every row's start state in it (-1: unconstrained)."""
    mode: str = "greedy"
    temperature: float = 1.0
    top_k: Optional[int] = None
    top_p: Optional[float] = None
    seed: int = 0
    row_params: Optional[Tuple[SamplingParams, ...]] = None
    row_ids: Optional[Tuple[int, ...]] = None
    processors: Optional[Processors] = None
    fsm: Any = None
    grammar_starts: Optional[Tuple[int, ...]] = None
    # the acceptance rule that goes with the mode (keyword fields): None = exact match (speculative sampling's own under "spec"), else
    # "typical" / "topk_agree" on the device (sd_specdec_set_acceptance); `mode` then says how the token after the accepted prefix is
    # chosen: "greedy" the target's argmax, "sampled" a draw
    accept_rule: Optional[str] = None
    accept_temperature: float = 1.0
    accept_epsilon: float = 0.09
    accept_delta: Optional[float] = None
    accept_k: int = 1
    # confidence-gated draft length (sd_specdec_set_draft_confidence): None = every row proposes K, else a row stops drafting after the
    # first forward i + 1 >= draft_min_k whose confidence (the draft's softmax probability of its own token) is below the threshold
    draft_confidence: Optional[float] = None
    draft_min_k: int = 1
    # per-token log-probs (sd_specdec_set_logprobs): None = off, else the alternatives listed per emitted token (0: its own log-prob only)
    logprobs: Optional[int] = None

    def __post_init__(self):
        # a grammar is a line of the processor stage, and requests with penalties of their own need it: identity scalars will do
        if self.processors is None and (self.fsm is not None or any(e.has_penalties for e in self.row_params or ())):
            object.__setattr__(self, "processors", Processors.IDENTITY)

    @classmethod
    def from_sampling(cls, sampling) -> "StepOptions":
        """A `sampling` description: None (greedy), a StepOptions, or {"temperature", "top_k", "top_p", "seed"} (+ "spec": True, "rows" / "ids")."""
        if sampling is None or isinstance(sampling, cls):
            return sampling or cls()
        rows = sampling.get("rows")
        return cls("spec" if sampling.get("spec") else "sampled", sampling["temperature"], sampling["top_k"], sampling["top_p"],
                   sampling["seed"], None if rows is None else tuple(rows), None if rows is None else tuple(sampling["ids"]))

    def rows(self, index: Sequence[int]) -> "StepOptions":
        """The options of a subset of the rows (a session over some of a call's requests): each keeps its own stream id."""
        per_row = {f: getattr(self, f) for f in ("row_params", "row_ids", "grammar_starts") if getattr(self, f) is not None}
        return replace(self, **{f: tuple(xs[i] for i in index) for f, xs in per_row.items()})


# feature -> what it says where the run is not the captured step ({what}), has no draft model, has no fixed K (None: not asked)
_GATE = {
    "processors": ("logit processors (penalties, logit_bias, token bans) run inside the captured device step: {what} is not supported with them",
                   "logit processors need the draft-model mode (draft_mode='vanilla'): medusa / eagle proposals come from no logits row",
                   "logit processors keep a fixed K (controller='fixed'): adaptive K is not supported"),
    "grammar": ("a grammar runs inside the captured device step: {what} is not supported with it",
                "a grammar needs the draft-model mode (draft_mode='vanilla'): medusa / eagle proposals come from no logits row",
                "a grammar keeps a fixed K (controller='fixed'): adaptive K is not supported"),
    "sampling_params": ("sampling_params are read by the captured device step (implementation='hip'; policy 'longest_prefix', or 'rejection' "
                        "with backend='device'): {what} is not supported with them",
                        "sampling_params need the draft-model mode (draft_mode='vanilla'): medusa / eagle drafting is not supported with them",
                        "sampling_params keep a fixed K (controller='fixed'): adaptive K is not supported"),
    "rejection": (None, None, "policy='rejection' (backend='device') keeps a fixed K (controller='fixed'): adaptive K is not supported"),
    "share_prefix": ("share_prefix / n need the captured device step ({what})", None, None),
    "acceptance": (None, "policy 'typical' / 'topk_agree' with backend='device' needs the draft-model mode (draft_mode='vanilla'): medusa / eagle "
                   "proposals are not judged by it",
                   "policy 'typical' / 'topk_agree' with backend='device' keeps a fixed K (controller='fixed'): adaptive K is not supported"),
    "draft_confidence": ("draft_confidence is decided inside the captured device step: {what} is not supported with it",
                         "draft_confidence needs the draft-model mode (draft_mode='vanilla'): medusa / eagle drafting has no draft forward to judge",
                         "draft_confidence moves every row's k inside the step and needs a fixed shape K (controller='fixed'): adaptive K is not "
                         "supported with it"),
    "logprobs": ("logprobs are computed inside the captured device step: {what} is not supported with them",
                 "logprobs need the draft-model mode (draft_mode='vanilla'): medusa / eagle / self-draft steps store no verify rows",
                 "logprobs keep a fixed K (controller='fixed'): adaptive K is not supported"),
    "context_window": ("context_window rolls the caches of the captured device step: {what} is not supported with it",
                       "context_window needs the draft-model mode (draft_mode='vanilla'): medusa / eagle / self-draft steps keep state that "
                       "a roll does not move",
                       "context_window keeps a fixed K (controller='fixed'): adaptive K is not supported"),
}


def gate(pipe, feature: str, captured_step: bool, what: str = "", self_draft: bool = False) -> None:
    """A feature of the captured step is refused, not approximated, where the run is not that step (`what` names it), has no draft model, or moves K."""
    route, draft, fixed = _GATE[feature]
    if not captured_step:
        raise NotImplementedError(route.format(what=what))
    if draft and (pipe.config.get("draft_mode", "vanilla") != "vanilla" or pipe.draft_lm is None or pipe.medusa_heads is not None or self_draft):
        raise NotImplementedError(draft)
    if fixed and not isinstance(pipe.controller, FixedKController):
        raise NotImplementedError(fixed)


def _processors(pipe, kwargs: Dict[str, Any]) -> Optional[Processors]:
    """The logit processors of a run (call kwargs over config): repetition_penalty (over prompt + generated tokens), presence_penalty /
    frequency_penalty (over generated tokens), logit_bias {id: value}, bad_token_ids, allowed_token_ids. None for identity values."""
    if set(kwargs) - set(PROCESSOR_KEYS):
        raise TypeError(f"unknown logit-processor argument(s): {sorted(set(kwargs) - set(PROCESSOR_KEYS))}")

    def val(key, default):
        v = kwargs.get(key) if kwargs.get(key) is not None else pipe.config.get(key)
        return default if v is None else v

    rp, pres, freq = float(val("repetition_penalty", 1.0)), float(val("presence_penalty", 0.0)), float(val("frequency_penalty", 0.0))
    check_penalties(rp, pres, freq)
    V = pipe.base_lm.vocab_size
    lb, bad, allowed = val("logit_bias", None), val("bad_token_ids", None), val("allowed_token_ids", None)

    def ids_of(name, xs):
        out = [int(x) for x in xs]
        if not all(0 <= x < V for x in out):
            raise ValueError(f"{name}: id {next(x for x in out if not 0 <= x < V)} is outside the vocabulary [0, {V})")
        return out

    bias = None
    if lb or bad or allowed is not None:
        bias = torch.zeros(V, dtype=torch.float32)
        if allowed is not None:
            keep = ids_of("allowed_token_ids", allowed)
            if not keep:
                raise ValueError("allowed_token_ids is empty: no token could be emitted")
            bias.fill_(float("-inf"))
            bias[keep] = 0.0
        for t, v in zip(ids_of("logit_bias", (lb or {}).keys()), (lb or {}).values()):
            if math.isnan(float(v)):
                raise ValueError(f"logit_bias[{t}] is NaN")
            bias[t] += float(v)
        if bad:
            bias[ids_of("bad_token_ids", bad)] = float("-inf")
    proc = Processors(rp, pres, freq, bias)
    return None if bias is None and proc == Processors.IDENTITY else proc


def _grammar(pipe, grammar, n_prompts: int) -> Dict[str, Any]:
    """The grammar of a run, a TokenFSM for every prompt or a list with one entry per prompt (None: unconstrained) -> StepOptions' fsm and
    grammar_starts ({}: none). Different automata are merged with TokenFSM.union, once per combination of member objects. The automaton's
    eos_id must be the pipeline's EOS where it has one: the host's EOS rule stops a row on it."""
    if grammar is None:
        return {}
    entries = list(grammar) if isinstance(grammar, (list, tuple)) else [grammar] * n_prompts
    if len(entries) != n_prompts:
        raise ValueError(f"grammar: {len(entries)} entries for {n_prompts} prompts")
    members: List[Any] = []
    for g in entries:
        if g is not None and not isinstance(g, TokenFSM):
            raise TypeError(f"grammar: expected a TokenFSM or None, got {type(g).__name__}")
        if g is not None and not any(g is m for m in members):
            members.append(g)
    if not members:
        return {}
    V, eos = pipe.base_lm.vocab_size, pipe.base_lm.get_tokenizer_info().get("eos_token_id")
    for g in members:
        if g.V != V:
            raise ValueError(f"grammar: the automaton is over {g.V} tokens, the vocabulary has {V}")
        if g.eos_id != members[0].eos_id or (eos is not None and g.eos_id != eos):
            raise ValueError(f"grammar: the automaton ends on eos_id {g.eos_id}, the pipeline's EOS is {eos}")
    if len(members) == 1:
        fsm, starts = members[0], [members[0].start]
    else:
        key = tuple(id(m) for m in members)
        if key not in pipe._grammar_unions:
            pipe._grammar_unions[key] = (members,) + TokenFSM.union(members)      # (the members are held: their ids stay theirs)
        _, fsm, starts = pipe._grammar_unions[key]
    start_of = {id(m): st for m, st in zip(members, starts)}
    return {"fsm": fsm, "grammar_starts": tuple(-1 if g is None else start_of[id(g)] for g in entries)}


def spec_options(pipe, kwargs: Dict[str, Any]) -> StepOptions:
    """policy="rejection" on the device: speculative sampling, shaped by the POLICY's temperature, seed, top_k and top_p (not the call's)."""
    if kwargs.get("top_k") or (kwargs.get("top_p") is not None and float(kwargs["top_p"]) < 1.0):
        raise NotImplementedError("policy='rejection' (backend='device'): top-k / top-p shaping of the two distributions is not supported")
    gate(pipe, "rejection", True)
    pol = pipe.policy
    return StepOptions("spec", float(pol.temperature), pol.top_k, pol.top_p if pol.top_k else None, int(kwargs.get("seed", pol.seed)))


def row_options(pipe, sampling_params, n_prompts: int, n: int, do_sample, kwargs: Dict[str, Any], self_draft: bool) -> Optional[StepOptions]:
    """Per-request parameters of a call, one SamplingParams per prompt, expanded with `n` as a grammar list is -> None, or the step's
    mode (policy="longest_prefix": the sampled bonus token; "rejection" on the device: speculative sampling) with every row's parameters,
    seeds resolved (an entry without one takes the call's), and stream id: its index among the call's rows, not its slot. Refused: call-level
    do_sample / top_k / top_p / penalties next to it, and values the device would only turn into a greedy row (SamplingParams.check)."""
    if sampling_params is None:
        return None
    clash = [k for k in ROW_SAMPLING_CLASH if kwargs.get(k) is not None] + (["do_sample"] if do_sample is not None else [])
    if clash:
        raise ValueError(f"sampling_params carries every request's own parameters: the call-level {sorted(clash)} cannot be given with it")
    entries = list(sampling_params)
    if len(entries) != n_prompts:
        raise ValueError(f"sampling_params: {len(entries)} entries for {n_prompts} prompts")
    for e in entries:
        if not isinstance(e, SamplingParams):
            raise TypeError(f"sampling_params: expected SamplingParams, got {type(e).__name__}")
    spec = pipe.policy_name == "rejection" and pipe.rejection_backend == "device"
    gate(pipe, "sampling_params", not pipe._fake and (pipe.policy_name == "longest_prefix" or spec),
         f"policy={pipe.policy_name!r} on the host loop", self_draft)
    seed = int(kwargs.get("seed", pipe.policy.seed if spec else (pipe.config.get("seed") or 0)))
    rows = tuple(e.with_seed(seed) for e in entries for _ in range(int(n)))
    for e in rows:
        e.check(pipe.base_lm.vocab_size, spec=spec)
    return StepOptions("spec" if spec else "sampled", float(pipe.policy.temperature) if spec else 1.0, None, None, seed, rows, tuple(range(len(rows))))


def with_stage(pipe, options: StepOptions, kwargs: Dict[str, Any], grammar, n_rows: int, gates=None) -> StepOptions:
    """`options` (the sampling side of a run) with the logit processors `kwargs` name and the grammar. gates: (the run is the captured
    step, and one a grammar can run in, what it is called in a refusal); None (start_session): its caller has chosen the route."""
    processors = _processors(pipe, kwargs)
    if processors is not None and gates:
        gate(pipe, "processors", gates[0], gates[2])
    table = _grammar(pipe, grammar, n_rows)
    if table and gates:
        gate(pipe, "grammar", gates[1], gates[2])
    return replace(options, processors=processors, **table)


# route: "step" (a DecodeSession on the captured device step), "host_policy" / "host_rejection" (the two host loops) or "fake"
Call = namedtuple("Call", "route prompts ids options max_tokens temperature sample_t share_prefix self_draft")


def resolve(pipe, prompts: Sequence[Any], max_tokens, temperature, do_sample, kwargs: Dict[str, Any], share_prefix=False, n=1,
            grammar=None, sampling_params=None, single: bool = False, policy_routes: bool = True, draft_confidence=None,
            draft_min_k=None, logprobs=None) -> Call:
    """A call's arguments -> its route, its prompts expanded with n, their ids and its options, every refusal raised on the way.
    single (generate): one row and no bonus token; the draft modes draft; do_sample=True is the host loop drawing the draft's tokens at
    sample_t. policy_routes (generate, generate_batch): the policy chooses between the captured step and the host loops, persistent heads
    may draft, rejection on the device admits share_prefix. Without it (generate_many): the draft model's captured step whatever the policy."""
    cfg, policy, fake, batch = pipe.config, pipe.policy_name, pipe._fake, policy_routes and not single
    longest, spec = policy == "longest_prefix", policy == "rejection" and pipe.rejection_backend == "device"
    heads, sample_t = batch and pipe.medusa_heads is not None, None      # (persistent heads also serve generate_batch)
    lossy = getattr(pipe, "accept_device", None)      # "typical" / "topk_agree" with backend="device": a rule of the captured step
    if lossy is not None:
        refuse_call(pipe, single, sampling_params)
        gate(pipe, "acceptance", True)
    if single and sampling_params is not None:
        raise NotImplementedError("sampling_params belong to generate_batch and generate_many (one entry per prompt of a batch): "
                                  "generate() decodes one row")
    if single and (share_prefix or int(n or 1) != 1):
        raise NotImplementedError("share_prefix / n belong to generate_batch and generate_many: generate() decodes one row")
    n = 1 if single else int(n)
    if n < 1:
        raise ValueError(f"n={n} (at least 1)")
    rows = None if single else row_options(pipe, sampling_params, len(prompts), n, do_sample, kwargs, heads)
    share_prefix = not single and (bool(share_prefix) or n > 1)
    if share_prefix:
        gate(pipe, "share_prefix", not fake and (longest or lossy is not None or (spec and batch)),
             "implementation='hip'; policy 'longest_prefix', or 'rejection' with backend='device'" if batch else
             "implementation='hip', policy='longest_prefix'")
    if fake and batch:
        # the double has no tokenizer to pad a batch with: the reference falls back to generate() per prompt (pipeline.py:1680-1700)
        if grammar is not None:
            gate(pipe, "grammar", False, "implementation='fake'")
        if draft_confidence is not None:
            gate(pipe, "draft_confidence", False, "implementation='fake'")
        with_logprobs(pipe, StepOptions(), logprobs, False, "implementation='fake'")
        return Call("fake", list(prompts), [], StepOptions(), max_tokens, temperature, None, False, False)
    max_tokens, temperature = max_tokens or cfg["max_new_tokens"], temperature or cfg["temperature"]      # (0 is "not given")
    do_sample, sampling = do_sample if do_sample is not None else cfg["do_sample"], rows
    if single and do_sample and not fake:   # (the fake double ignores sampling parameters, in the reference as here)
        # pipeline.py:1019-1027 / :1217-1224: the DRAFT's proposals, and the one base token of a zero-accept step, are drawn at the call's
        # temperature (models/hip_lm.py hf_sampling_probs); every verification path is greedy (speculative_scheduler.py:192-199, :304-310)
        if cfg.get("draft_mode", "vanilla") in ("medusa", "eagle") or not longest:
            raise NotImplementedError("generate(do_sample=True) is restated for the draft-model mode with the longest_prefix policy")
        sample_t = float(temperature)
    elif not single and sampling is None and do_sample:     # the sampled bonus token (kwargs over config, reference pipeline.py:3148-3153)
        top_k, top_p = kwargs.get("top_k", cfg.get("top_k", None)), kwargs.get("top_p", cfg.get("top_p", None))
        if top_k and min(int(top_k), pipe.base_lm.vocab_size) > 1024:
            raise NotImplementedError(f"do_sample=True: top_k={top_k} > 1024 is not on the HIP path")
        sampling = StepOptions("sampled", float(temperature), int(top_k) if top_k else None, None if top_p is None else float(top_p),
                               int(kwargs.get("seed", cfg.get("seed") or 0)))
    if not single and pipe.draft_lm is None and not heads:
        raise ValueError("generate_batch drafts with the draft model (the reference ignores draft_mode there): pass draft_lm / draft_model"
                         if batch else "generate_many drafts with the draft model: pass draft_lm / draft_model")
    if isinstance(grammar, (list, tuple)):
        grammar = [g for g in grammar for _ in range(n)]
    prompts = [p for p in prompts for _ in range(n)]
    ids = [pipe._encode(p) for p in prompts]
    if single and policy == "rejection":
        raise NotImplementedError("policy='rejection' is a generate_batch policy (it emits a correction / bonus token every step)")
    # the route: which runs are the captured step (and one a grammar can run in), and what the others are called in a refusal
    captured = (longest or spec or lossy is not None) if batch else ((longest or lossy is not None) and not fake and sample_t is None)
    grammar_ok = captured and not (pipe._medusa_random() if single else heads)
    what = ("generate(do_sample=True)" if sample_t is not None else f"policy={policy!r} on the host loop" if batch else
            f"policy={policy!r} / implementation={cfg['implementation']!r}")
    on_step = grammar_ok if single else captured or not batch      # (generate_many is always the step)
    route = "step" if on_step else "host_rejection" if policy == "rejection" else "host_policy"
    options = with_stage(pipe, sampling or StepOptions(), {k: kwargs[k] for k in PROCESSOR_KEYS if k in kwargs}, grammar, len(ids),
                         (captured, grammar_ok, what))
    if batch and spec and rows is None:       # (the stage's refusals come before the mode's)
        options = replace(spec_options(pipe, kwargs), processors=options.processors, fsm=options.fsm, grammar_starts=options.grammar_starts)
    elif route == "host_policy" and sampling is not None:
        raise NotImplementedError(f"policy={policy!r} with do_sample=True is not on the HIP path")
    if lossy is not None:                     # the rule goes with whatever mode the call's sampling made: greedy or the sampled bonus token
        options = with_rule(options, lossy)
    # confidence-gated draft length: the call's threshold over the config's (which generate() and the fake double do not read)
    if draft_confidence is None and not single and not fake:
        draft_confidence = cfg.get("draft_confidence_threshold")
        draft_min_k = cfg.get("draft_min_k") if draft_confidence is not None and draft_min_k is None else draft_min_k
    options = with_confidence(pipe, options, draft_confidence, draft_min_k, on_step and not fake, what, bool(heads), single)
    options = with_logprobs(pipe, options, logprobs, on_step and not fake, "implementation='fake'" if fake else what, bool(heads), single)
    self_draft = cfg.get("draft_mode") in ("medusa", "eagle") if single else heads and longest
    return Call(route, prompts, ids, options, max_tokens, float(temperature) if single else temperature, sample_t, share_prefix, self_draft)
