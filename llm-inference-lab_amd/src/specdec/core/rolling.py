"""The rolling context window: context_window=W / attention_sinks=S on generate_batch, generate_many and start_session
(csrc/kv_evict.hip, HipModel.evict_row). A row's cache keeps its first S positions (the attention sinks) and the most recent ones,
never more than W: when the next launches would not fit, a block of `drop` positions after the sinks is evicted, the survivors
move down and their keys are re-rotated to their new, cache-relative positions (StreamingLLM's rolling cache).

`plan` is the whole decision as a pure host function: the `Window` it returns says how much is dropped per roll, how much room
the launches of a session need, how large the cache rows must be, and — `Window.roll` — whether a row of a given cache length must
roll now. `call_window` / `session_window` turn a call's arguments into a Window or a refusal; every refusal of the feature is
raised here. Where the run must be the captured step with a draft model and a fixed K is step_options' table (`gate`, feature
"context_window")."""

from dataclasses import dataclass
from typing import Any, List, Optional, Sequence

ARCH_GPT2 = 1
LAUNCH_DEPTH = 2        # the most steps a DecodeSession keeps launched (SPECDEC_LAUNCH_DEPTH cannot raise it)


@dataclass(frozen=True)
class Window:
    """size = W, sinks = S; drop: positions evicted per roll, the largest multiple of 8 that is <= (W - S) / 2, at least 8;
    room: positions past a row's cache length that the launches between two looks at the row can address — the row's own step, the
    `depth` steps launched ahead of the host (the device advances every row by itself, void steps included) and the two positions
    a step reads below its length: (depth + 1) (K + 1) + 2; l_max: the cache rows a session needs, W + room: no launched step,
    void or not, addresses a position >= l_max (DecodeSession asserts it at every launch)."""
    size: int
    sinks: int
    drop: int
    room: int

    @property
    def l_max(self) -> int:
        return self.size + self.room

    def roll(self, cache_len: int) -> Optional[int]:
        """The positions to evict from a row whose cache length (sequence length minus what was evicted) is cache_len, now, before
        its next launch; None: the launches fit."""
        return self.drop if cache_len + self.room > self.size else None

    def fits(self, prompt_len: int) -> bool:
        """a prompt of this length starts without a roll (prompts are not truncated)"""
        return prompt_len + self.room <= self.size


def drop_of(size: int, sinks: int) -> int:
    return max(8, (size - sinks) // 2 // 8 * 8)


def plan(size: int, sinks: int, k: int, depth: int = LAUNCH_DEPTH, max_pos: Optional[int] = None) -> Window:
    """The Window of context_window=size, attention_sinks=sinks for steps of K = k proposals kept `depth` deep. ValueError: a
    window beyond the models' positions, or one so small that a step does not fit after a roll — a roll happens at a cache length c
    in (W - room, W] and leaves c - drop: it must have the sinks and the block below what the cache holds (S + drop <= W - room, the
    cache holds c - 1 positions) and leave room again (drop >= room)."""
    size, sinks, k, depth = int(size), int(sinks), int(k), int(depth)
    if sinks < 0:
        raise ValueError(f"attention_sinks={sinks} (at least 0)")
    if size < 1:
        raise ValueError(f"context_window={size} (a positive number of positions)")
    if max_pos is not None and size > max_pos:
        raise ValueError(f"context_window={size} exceeds the {max_pos} positions of the smaller model (max_pos)")
    w = Window(size, sinks, drop_of(size, sinks), (depth + 1) * (k + 1) + 2)
    if w.drop < w.room or sinks + w.drop > size - w.room:
        raise ValueError(f"context_window={size} is too small for steps of K={k}: a roll drops {w.drop} positions after {sinks} sinks and "
                         f"must leave room for {w.room} (the launches in flight); {sinks + 2 * w.room + 16} positions always fit")
    return w


def _value(pipe, given, key: str):
    return given if given is not None else pipe.config.get(key)


def refuse_single(pipe, kwargs) -> None:
    """generate() decodes one row on the draft-emit step: no window (the arguments are taken out of its kwargs either way)."""
    size = _value(pipe, kwargs.pop("context_window", None), "context_window")
    kwargs.pop("attention_sinks", None)
    if size is not None:
        raise NotImplementedError("context_window belongs to generate_batch, generate_many and start_session: generate() decodes one "
                                  "row within its cache")


def _models(pipe) -> List[Any]:
    return [lm for lm in (pipe.base_lm, pipe.draft_lm) if lm is not None]


def _window(pipe, size, sinks, k: int, captured: bool, what: str, self_draft: bool, share_prefix: bool, prompts: Sequence[Sequence[int]]) -> Window:
    from .step_options import gate

    gate(pipe, "context_window", captured, what, self_draft)
    for lm in _models(pipe):
        if getattr(lm.config, "arch", 0) == ARCH_GPT2:
            raise NotImplementedError("context_window needs Llama models: a GPT-2 model has learned positions in its hidden states, and "
                                      "there is nothing to re-rotate in its cache")
        if getattr(lm, "kv_page_len", None) is not None:
            raise NotImplementedError("context_window is not supported with paged KV (page-granular dropping is not built): use dense caches")
    if share_prefix:
        raise NotImplementedError("share_prefix / n are not supported with context_window: forked rows would need their own eviction events")
    w = plan(size, 4 if sinks is None else sinks, k, LAUNCH_DEPTH, min(int(lm.config.max_pos) for lm in _models(pipe)))
    for p in prompts:
        if not w.fits(len(p)):
            raise ValueError(f"prompt of {len(p)} tokens does not fit context_window={w.size} (steps of K={k} need {w.room} positions of "
                             "room; prompts are not truncated)")
    return w


def _k(pipe) -> int:
    ctl = pipe.controller
    return int(getattr(ctl, "k", None) or getattr(ctl, "max_k", None) or 4)


def call_window(pipe, context_window, attention_sinks, call) -> Optional[Window]:
    """generate_batch / generate_many: the Window of a resolved call (step_options.Call), None when no window is asked."""
    size = _value(pipe, context_window, "context_window")
    if size is None:
        return None
    what = "implementation='fake'" if pipe._fake or call.route == "fake" else f"policy={pipe.policy_name!r} on the host loop"
    return _window(pipe, size, _value(pipe, attention_sinks, "attention_sinks"), _k(pipe), call.route == "step" and not pipe._fake, what,
                   bool(call.self_draft), bool(call.share_prefix), call.ids)


def session_window(pipe, context_window, attention_sinks, emit_mode: int, self_draft: bool, share_prefix: bool, bonus_mode: int,
                   prompts: Sequence[Sequence[int]]) -> Optional[Window]:
    """start_session: the caller has chosen the route; the mode, the models and the prompts are judged."""
    size = _value(pipe, context_window, "context_window")
    if size is None:
        return None
    if emit_mode != bonus_mode:
        raise NotImplementedError("context_window needs the bonus-token emit mode (generate_batch): the draft-emit mode (EMIT_DRAFT) is "
                                  "generate()'s, which decodes one row within its cache")
    return _window(pipe, size, _value(pipe, attention_sinks, "attention_sinks"), _k(pipe), not pipe._fake, "implementation='fake'", self_draft,
                   share_prefix, prompts)


def check_session(window: Optional[Window], other_step: bool, bonus: bool, share_prefix: bool, k: int) -> Optional[Window]:
    """What a DecodeSession cannot combine with a window (other_step = no draft model, the fake double, or a K that moves)."""
    if window is None:
        return None
    if other_step or not bonus or share_prefix:
        raise NotImplementedError("context_window needs the bonus-token HIP step with a draft model and a fixed K, without share_prefix")
    if window.room < (LAUNCH_DEPTH + 1) * (k + 1) + 2:
        raise ValueError(f"the window was planned for fewer proposals than K={k}")
    return window


def refuse_paged(engines) -> None:
    if any(e.page_len is not None for e in engines):
        raise NotImplementedError("context_window is not supported with paged KV (page-granular dropping is not built): use dense caches")


def kept_tokens(seq: Sequence[int], sinks: int, evicted: int) -> List[int]:
    """The tokens whose positions a rolled row still holds, in cache order (the last one is pending, as in an unrolled row)."""
    return list(seq) if not evicted else list(seq[:sinks]) + list(seq[sinks + evicted:])
