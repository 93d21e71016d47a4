"""`SpeculativePipeline` — the draft-then-verify loop on MI355X.

Public surface of the reference (src/specdec/core/pipeline.py): the constructor
arguments (:198-218), `generate(prompt, max_tokens, temperature, do_sample)` (:893) and
`generate_batch(prompts, ...)` (:1605), and the result-dict keys (:1350-1380, :3876-3905).

What runs underneath is different. The reference makes 2K HF forwards per step over the
whole prefix from Python, synchronising the host several times per row. Here one call
per step (`HipSpecDec.step`) replays a hipGraph that holds the K draft forwards, ONE
K+1-token verify forward of the target over its appended KV cache, the accept scan and
the in-place state advance; the host reads one small pinned record per step and applies
the reference's host-side rules to it (EOS cut, bonus, de-duplication, budget — restated
in `_rules_batch` / `_rules_single`). When those rules leave a row where the device
assumed (the common case) nothing else happens; when they do not (a de-duplication
dropped or rewound tokens), the row's caches are rebuilt from its sequence.

`generate_batch(do_sample=True)` samples what the reference samples there — only the token after
the accepted prefix (`sample_bonus_token_from_logits`, :3156/:3231/:3355; drafting and verification
stay greedy, :2400/:2645) — inside the same captured step (csrc/sample.hip). `generate(do_sample=True)`
is another rule (:1019-1027, :1217-1224): the draft's proposals and the base token of a zero-accept step are
drawn by transformers' sampling on torch's global CPU generator, verification is greedy; it runs on the
host-policy loop and, seeded alike, makes the reference's draws (models/hip_lm.py hf_sampling_probs).
"""

from __future__ import annotations

import logging
import os
import time
from collections import deque
from typing import Any, Dict, List, Optional, Sequence, Union

import psutil
import torch
import yaml

from specdec_hip.engine import EngineGaveUp, HipModel, HipSpecDec

from ..models.hip_lm import HipLM, create_hip_lm, create_hip_pair, is_named_pair
from ..policies.controllers import FixedKController, create_controller
from ..policies.policies import create_policy
from ..utils.deterministic import ensure_deterministic, set_deterministic_mode
from ..utils.interfaces import LanguageModel
from .acceptance import device_rule, session_rule
from .draft_confidence import check_session, session_confidence
from . import logprobs as lpmod
from . import rolling
from .step_options import StepOptions, resolve, row_options, spec_options, with_stage

PromptLike = Union[str, Sequence[int], torch.Tensor]

_DEFAULTS: Dict[str, Any] = {
    "base_model": "synthetic:llama-3.2-3b",
    "draft_model": "synthetic:llama-3.2-1b",
    "max_draft": 4,
    "implementation": "hip",
    "temperature": 0.7,
    "do_sample": False,
    "max_new_tokens": 64,
    "top_p": 0.9,
    "top_k": 50,
    "repetition_penalty": 1.0,
    "device": "cuda",
    "seed": 1234,
    "log_level": "INFO",
    "verbose": False,
    "draft_mode": "vanilla",
    "medusa": {"enabled": False, "num_heads": 2, "head_init": "tie", "temperature": 0.7, "top_p": 1.0},
    "eagle": {"enabled": False, "alpha": 0.7, "max_draft": 2},
    # share_prefix: a row is forked over a prefix it has in common with a row already in the cache from this many tokens on
    # (rows whose whole prompts are equal are always forked)
    "min_shared_prefix": 32,
    # the rolling context window (core/rolling.py): None = a row lives within prompt + max_tokens cache positions; W = its cache keeps
    # attention_sinks first positions and the most recent ones, never more than W, and generation length is no longer bound by the cache
    "context_window": None,
    "attention_sinks": 4,
}


def _clamp(tok: int, vocab: int) -> int:
    return 0 if tok < 0 else (vocab - 1 if tok >= vocab else int(tok))


def expected_tokens_per_step(alpha: Sequence[float], k_max: int = 8) -> Dict[int, Optional[float]]:
    """{K: mean over t of sum_{j=0..K} prod_{i<j} alpha[t+i]} for K = 1..k_max: the tokens a step of K proposals emits (the
    accepted prefix plus the correction / bonus token) when position t+i accepts with probability alpha[t+i], averaged over the
    windows t = 0 .. len(alpha)-K that fit; None for a K with no window."""
    a = [float(x) for x in alpha]
    out: Dict[int, Optional[float]] = {}
    for K in range(1, int(k_max) + 1):
        windows = len(a) - K + 1
        if windows < 1:
            out[K] = None
            continue
        total = 0.0
        for t in range(windows):
            prod, acc = 1.0, 1.0
            for i in range(K):
                prod *= a[t + i]
                acc += prod
            total += acc
        out[K] = total / windows
    return out


class _Row:
    __slots__ = ("seq", "generated", "active", "proposed", "accepted", "draws", "steps", "strict_acc", "strict_prop", "k_trace", "counters",
                 "n_prompt", "token_info", "evicted", "evictions", "rebuilds")

    def __init__(self, seq: List[int]):
        self.seq, self.generated, self.active = seq, [], True
        self.n_prompt = len(seq)                   # seq[:n_prompt] is the prompt, the rest was generated (logit processors)
        self.proposed = self.accepted = self.draws = self.steps = 0
        self.counters: List[tuple] = []            # after each of the row's own steps: (proposed, accepted, tokens generated, accept length)
        self.strict_acc = self.strict_prop = 0     # per-row adaptive K: what the row's controller is fed with
        self.k_trace: List[int] = []               # ... and the k that counted in each of its steps
        self.token_info: List[Any] = []            # logprobs: entry j is the TokenInfo of generated[j] (empty while the mode is off)
        # context_window: positions evicted from the row's caches so far (its cache length is len(seq) - evicted), the rolls as
        # (tokens generated before the roll, drop), and the tokens generated before each rebuild of a rolled row's caches (a resync)
        self.evicted = 0
        self.evictions: List[tuple] = []
        self.rebuilds: List[int] = []


class SpeculativePipeline:
    def __init__(self, base_lm: Optional[LanguageModel] = None, draft_lm: Optional[LanguageModel] = None,
                 config_path: Optional[str] = None, base_model: Optional[Any] = None,
                 draft_model: Optional[Any] = None, max_draft: Optional[int] = None, device: str = "auto",
                 seed: Optional[int] = None, implementation: Optional[str] = None,
                 force_device: Optional[str] = None, policy: str = "longest_prefix",
                 policy_params: Optional[Dict[str, Any]] = None, controller: str = "fixed",
                 controller_params: Optional[Dict[str, Any]] = None, draft_mode: str = "vanilla",
                 enable_optimization: bool = True, enable_profiling: bool = False,
                 profile_dir: Optional[str] = None, medusa_heads: Optional[Any] = None):
        self.logger = logging.getLogger(__name__)
        self.config = self._load_config(config_path)
        for key, val in (("base_model", base_model), ("draft_model", draft_model), ("max_draft", max_draft),
                         ("seed", seed), ("implementation", implementation), ("draft_mode", draft_mode)):
            if val is not None:
                self.config[key] = val
        impl = self.config["implementation"]
        if impl not in ("hip", "hf", "fake"):
            # CPU / MPS implementations of the reference have no counterpart here: the product is the GPU path
            raise ValueError(f"implementation={impl!r} is not available in this build (use 'hip')")
        # "fake": the reference's weight-less test double (models/fake_lm.py; what the reference's own configs/specdec.yaml
        # selects): token ids are a function of the input ids, logits are noise on the device; drives the step loop, the
        # policies and the registry ops without a model (generate / generate_batch through the host-policy loop)
        self._fake = impl == "fake"
        mode = self.config.get("draft_mode", "vanilla")
        # persistent heads (specdec_hip.weights.MedusaHeads): not in the reference — K trained/tied heads evaluated
        # in K GEMVs over the target's last hidden state replace the draft forwards
        self.medusa_heads = medusa_heads
        if medusa_heads is not None and mode != "medusa":
            raise ValueError("medusa_heads needs draft_mode='medusa'")
        if mode == "medusa" and medusa_heads is not None:
            pass
        elif mode == "medusa":
            # `head_init: tie` / `copy`: Medusa-lite as the reference's draftor defines it (modes/medusa.py): heads tied to /
            # copied from the lm_head, head 0 evaluated on the same last hidden state for all K proposals -> K copies of the
            # target's own next token.
            # `head_init: random`: what the reference PIPELINE runs for every Medusa configuration (_run_medusa_hf,
            # pipeline.py:655-763: fresh nn.Linear heads with normal_(0, 0.02) weights and multinomial draws from the global
            # torch generator on every step): _draft_medusa_random below, generate() only.
            if self.config.get("medusa", {}).get("head_init", "tie") not in ("tie", "copy", "random"):
                raise ValueError("medusa.head_init must be 'tie', 'copy' or 'random'")
        elif mode == "eagle":
            # EAGLE-lite as the reference's HF path defines it (_run_eagle_hf, pipeline.py:765-889): draft tokens are the
            # argmax of the lm_head over hidden states extrapolated from the target's last two states, min(k, max_draft)
            # of them per step; generate() only, no draft model (sd_specdec_set_eagle).
            pass
        elif mode != "vanilla":
            raise NotImplementedError(f"draft_mode={mode!r}: 'vanilla', 'medusa' and 'eagle' drafting are on the HIP path")
        if not torch.cuda.is_available():
            raise RuntimeError("SpeculativePipeline needs a GPU (PyTorch-ROCm device 'cuda'); there is no CPU path")
        self.device = "cuda"
        self.dtype = torch.bfloat16
        self.amp_enabled = False
        self.enable_cuda_graph = True  # hipGraph replay of the step (the reference pins this to False)
        if self.config.get("seed") is not None:
            set_deterministic_mode(int(self.config["seed"]))
        ensure_deterministic(int(self.config.get("seed") or 1234))

        if self._fake:
            from ..models.fake_lm import create_fake_lm

            if mode != "vanilla" or medusa_heads is not None:
                raise NotImplementedError("implementation='fake' drafts with the fake draft model (draft_mode='vanilla')")
            sd = self.config.get("seed")
            self.base_lm = base_lm if base_lm is not None else create_fake_lm(f"fake-base-{self.config['base_model']}", seed=sd)
            self.draft_lm = draft_lm if draft_lm is not None else create_fake_lm(f"fake-draft-{self.config['draft_model']}", seed=sd)
        else:
            self.base_lm = base_lm if base_lm is not None else None
        no_draft = mode in ("medusa", "eagle") and draft_lm is None and self.config.get("draft_model") in (None, "", "none", "NONE")
        if not self._fake:
            if base_lm is None and draft_lm is None and not no_draft and is_named_pair(self.config["base_model"], self.config["draft_model"]):
                self.base_lm, self.draft_lm = create_hip_pair(self.config["base_model"], self.config["draft_model"])
            else:
                self.base_lm = base_lm if base_lm is not None else create_hip_lm(self.config["base_model"])
                self.draft_lm = draft_lm if (draft_lm is not None or no_draft) else create_hip_lm(self.config["draft_model"])
        for who, lm in (("base", self.base_lm), ("draft", self.draft_lm)):
            if self._fake:
                break
            if lm is None and who == "draft":
                continue                         # Medusa-lite drafts from the target itself (generate() only)
            if not isinstance(lm, HipLM):
                raise TypeError(f"{who}_lm must be a HipLM (got {type(lm).__name__}): the step loop drives the "
                                "models through the C-ABI engine, not through generate_tokens")
        if self.draft_lm is not None and self.base_lm.vocab_size != self.draft_lm.vocab_size:
            raise ValueError(f"draft/base vocabularies differ: {self.draft_lm.vocab_size} vs {self.base_lm.vocab_size}")
        self.speculative_enabled = True
        self.policy = create_policy(policy, **(policy_params or {}))
        # longest_prefix (exact match) is the policy inside the captured device step. The logit-threshold policies
        # (typical, topk_agree, conf_threshold) take the reference's own route (_decode_host_policy): they compare the draft with
        # what the base model generates by itself from the same prefix, which a parallel pass over the DRAFT tokens does
        # not give once a non-argmax draft token is accepted.
        self.policy_name = policy
        # policy="rejection": backend "host" (default) is the host loop (_decode_rejection); "device" runs speculative sampling
        # inside the captured step (csrc/spec_sample.hip, sd_specdec_set_spec_sampling) with the policy's temperature and seed
        self.rejection_backend = str((policy_params or {}).get("backend", "host"))
        if self.rejection_backend not in ("host", "device"):
            raise ValueError(f"policy_params['backend']={self.rejection_backend!r} (one of 'host', 'device')")
        # policy="typical" / "topk_agree" with backend "device": the rule runs inside the captured step on the verify pass's own rows —
        # the target's distribution after d_1..d_i, where the host loop scores the draft against the target's own continuation
        self.accept_device = device_rule(policy, policy_params, self._fake, self.base_lm.vocab_size)
        if self.rejection_backend == "device" and self.accept_device is None:
            if policy != "rejection":
                raise ValueError("policy_params['backend']='device' belongs to policy='rejection'")
            if self._fake:
                raise NotImplementedError("policy='rejection' with backend='device' needs the HIP engine (implementation='hip')")
            if not float((policy_params or {}).get("temperature", 1.0)) > 0:
                raise ValueError("policy='rejection' with backend='device' needs temperature > 0")
            # the policy shapes the mode: top_k (1..1024), optionally with top_p, as sd_sample_token defines them
            tk, tp = self.policy.top_k, self.policy.top_p
            if tk is not None and not 1 <= tk <= 1024:
                raise NotImplementedError(f"policy='rejection' (backend='device'): top_k={tk} is outside 1..1024")
            if tp is not None and not tp > 0:
                raise ValueError(f"policy='rejection' (backend='device'): top_p={tp} (must be > 0)")
            if tk is None and tp is not None and tp < 1.0:
                raise NotImplementedError("policy='rejection' (backend='device'): top_p without top_k (the full-vocabulary nucleus) is not "
                                          "supported; give a top_k in 1..1024")
        elif policy == "rejection" and any((policy_params or {}).get(key) is not None for key in ("top_k", "top_p")):
            raise NotImplementedError("policy='rejection' with backend='host' is unshaped: top_k / top_p in policy_params belong to "
                                      "backend='device'")
        if policy != "longest_prefix" and (mode != "vanilla" or medusa_heads is not None):
            raise NotImplementedError(f"policy={policy!r} drafts with the draft model (draft_mode='vanilla')")
        self.controller = create_controller(controller, **(controller_params or {}))
        from src.scheduler import create_speculative_scheduler

        self.scheduler = create_speculative_scheduler(device="cuda")
        self.metrics: Dict[str, Any] = {}
        self._runtimes: Dict[Any, Any] = {}
        # kept: the ids of member automata -> (the members, their union, its starts); (pattern, eos_id) -> the compiled TokenFSM
        self._grammar_unions, self._grammar_regexes = {}, {}

    # ------------------------------------------------------------------ configuration
    def _load_config(self, config_path: Optional[str]) -> Dict[str, Any]:
        """Flat YAML merged over the defaults (pipeline.py:398-438)."""
        cfg = dict(_DEFAULTS)
        if config_path:
            with open(config_path) as f:
                loaded = yaml.safe_load(f) or {}
            if not isinstance(loaded, dict):
                raise ValueError(f"{config_path}: expected a flat mapping")
            cfg.update(loaded)
        return cfg

    # ------------------------------------------------------------------ runtime pieces
    def _runtime(self, batch: int, need_len: int, k: int, emit_mode: int, self_draft: bool = False, adaptive: bool = False,
                 windowed: bool = False):
        """Engine instances (own KV caches over the shared weights) + the step loop object (`adaptive`: the loop whose
        rows carry their own K, a different captured step from the fixed-K loop of the same shape). windowed (context_window): the
        caches are sized by need_len itself, the window and its slack, and kept apart from those sized by prompt + budget."""
        key = (batch, emit_mode, self_draft, "window") if windowed else (batch, emit_mode, self_draft)
        rt = self._runtimes.get(key)
        if rt is None or rt["l_max"] < need_len:
            l_max = ((need_len if windowed else max(need_len, 256)) + 63) // 64 * 64
            rt = {"l_max": l_max, "target": self.base_lm.new_engine(batch, l_max),
                  "draft": None if self_draft else self.draft_lm.new_engine(batch, l_max), "loops": {}}
            self._runtimes[key] = rt
        lkey = ("adaptive", k) if adaptive else k
        loop = rt["loops"].get(lkey)
        if loop is None:
            loop = rt["loops"][lkey] = HipSpecDec(rt["draft"], rt["target"], batch, k, emit_mode)
            if self_draft and self.medusa_heads is not None:
                if self.medusa_heads.n_heads != k:
                    raise ValueError(f"{self.medusa_heads.n_heads} medusa heads but K={k}")
                loop.set_medusa(self.medusa_heads.weights, self.base_lm.weight_dtype)
            elif self_draft and self._eagle():
                # one state workspace per runtime: loops of different K continue the same extrapolation state
                rt["eagle_ws"] = loop.set_eagle(float(self.config.get("eagle", {}).get("alpha", 0.7)), rt.get("eagle_ws"))
        return rt, loop

    def _eagle(self) -> bool:
        return self.config.get("draft_mode") == "eagle"

    def _effective_k(self, k: int, self_draft: bool) -> int:
        """EAGLE-lite proposes min(k, eagle.max_draft) tokens per step (pipeline.py:818 of the reference)."""
        if self_draft and self._eagle():
            return max(1, min(int(k), int(self.config.get("eagle", {}).get("max_draft", 2))))
        return int(k)

    def _encode(self, prompt: PromptLike) -> List[int]:
        if isinstance(prompt, str):
            return [int(x) for x in self.base_lm.encode(prompt).flatten().tolist()]
        if isinstance(prompt, torch.Tensor):
            return [int(x) for x in prompt.flatten().tolist()]
        return [int(x) for x in prompt]

    def _prefill_row(self, rt, b: int, seq: List[int]) -> None:
        """KV of seq[:-1] into row b of both caches (the step recomputes the last two)."""
        if len(seq) < 2:
            return
        toks = torch.tensor([seq[:-1]], dtype=torch.int32, device="cuda")
        zero = torch.zeros(1, dtype=torch.int32, device="cuda")
        rt["target"].forward(toks, zero, 0, skip_head=True, row0=b)
        if rt["draft"] is not None:
            rt["draft"].forward(toks, zero, 0, skip_head=True, row0=b)

    def _absorb_row(self, rt, b: int, seq: List[int], held: List[Optional[List[int]]], stats: Dict[str, Any]) -> None:
        """share_prefix: KV of seq[:-1] into row b of both caches, computing as little of it as the other rows allow.
        held[j] is the token prefix whose KV row j's caches hold (None: nothing to rely on). The row with the longest common
        prefix c is the source: c == len(seq) - 1 (the same prompt) -> the row is forked from it (HipModel.fork_row, both
        engines) and nothing is computed; c >= min_shared_prefix -> forked over those c positions, and seq[c:-1] is forwarded
        at pos_base = c; otherwise the row is prefilled as _prefill_row does. Runs on the current stream, like the prefill."""
        want = seq[:-1]
        held[b] = None
        best, c = -1, 0
        for j, h in enumerate(held):
            if j == b or h is None:
                continue
            n = 0
            for x, y in zip(want, h):
                if x != y:
                    break
                n += 1
            if n > c:
                best, c = j, n
        engines = [e for e in (rt["target"], rt["draft"]) if e is not None]
        if want and c == len(want) or c >= max(int(self.config.get("min_shared_prefix", 32)), 1):
            for e in engines:
                e.fork_row(best, [b], c)
            if c < len(want):
                toks = torch.tensor([want[c:]], dtype=torch.int32, device="cuda")
                base = torch.tensor([c], dtype=torch.int32, device="cuda")
                for e in engines:
                    e.forward(toks, base, 0, skip_head=True, row0=b)
            stats["forked_rows"] += 1
            stats["shared_positions"] += c
        else:
            self._prefill_row(rt, b, seq)
            stats["prefilled_rows"] += 1 if want else 0
        held[b] = list(want)

    def _prefill(self, rt, rows: List[_Row], held: Optional[List[Optional[List[int]]]] = None,
                 stats: Optional[Dict[str, Any]] = None) -> None:
        """held (share_prefix): the session's record of what each row's caches hold; rows are then absorbed one by one, each
        forked from an earlier one where their prompts allow (_absorb_row)."""
        if held is not None:
            for b, r in enumerate(rows):
                self._absorb_row(rt, b, r.seq, held, stats)
            return
        if stats is not None:
            stats["prefilled_rows"] += sum(1 for r in rows if len(r.seq) >= 2)
        lens = {len(r.seq) for r in rows}
        if len(lens) == 1 and len(rows[0].seq) >= 2:
            toks = torch.tensor([r.seq[:-1] for r in rows], dtype=torch.int32, device="cuda")
            zero = torch.zeros(len(rows), dtype=torch.int32, device="cuda")
            rt["target"].forward(toks, zero, 0, skip_head=True)
            if rt["draft"] is not None:
                rt["draft"].forward(toks, zero, 0, skip_head=True)
        else:
            for b, r in enumerate(rows):
                self._prefill_row(rt, b, r.seq)

    @staticmethod
    def _set_row(loop: HipSpecDec, b: int, row: _Row) -> None:
        seq = row.seq       # (a rolled row sits at its cache length: what was evicted no longer counts)
        loop.set_row(b, len(seq) - row.evicted, seq[-2] if len(seq) >= 2 else 0, seq[-1], row.active)

    # ------------------------------------------------------------------ host-side rules
    def _rules_batch(self, row: _Row, k: int, a: int, t: List[int], max_tokens: int, eos: Optional[int],
                     resample=None, dedup: bool = True, info=None, resample_info=None) -> None:
        """One row of one generate_batch step (pipeline.py:3018-3590), from the step record:
        a = accepted length, t[i] = target argmax after the row's sequence + d_1..d_i (sampling mode:
        t[a] is the token the device sampled at position a; `resample(pos)` draws at another position
        with the same Philox draw — only an EOS-cut full acceptance needs it). dedup=False (a row under a grammar): the
        overlap / de-duplication rules are not applied — they delete tokens the row's automaton has consumed.
        info (logprobs; None: nothing is tracked): a payload parallel to t, entry i describing t[i]; every slice, append and delete
        applied to the tokens is applied to it too, into row.token_info, which stays parallel to row.generated.
        resample_info(pos, token): the payload of a token `resample` drew at another position."""
        V = self.base_lm.vocab_size
        gen, ginfo = row.generated, row.token_info
        if a > 0:
            acc = [_clamp(x, V) for x in t[:a]]
            acc_i = list(info[:a]) if info is not None else None
            if eos is not None and eos in acc:           # accepted EOS: cut there, row stops (:3120-3131)
                acc = acc[: acc.index(eos)]
                row.active = False
            pos = a if a < k else len(acc)                # (:3140-3231) the extra forward runs over seq + cut acc
            redrawn = not (resample is None or pos == a)
            bonus = _clamp(resample(pos) if redrawn else t[pos], V)
            if eos is not None and bonus == eos:         # bonus EOS stays in the output (:3274-3280)
                row.active = False
            acc.append(bonus)
            if info is not None:
                acc_i = acc_i[: len(acc) - 1] + [resample_info(pos, bonus) if redrawn else info[pos]]
            if gen and dedup:                            # overlap with the generated tail (:3295-3318)
                for c in range(min(5, len(gen), len(acc)), 0, -1):
                    if gen[-c:] == acc[:c]:
                        acc = acc[c:]
                        acc_i = acc_i[c:] if info is not None else None
                        break
            gen.extend(acc)
            emitted = acc
        else:
            emitted = [_clamp(t[0], V)]
            acc_i = [info[0]] if info is not None else None
            if eos is not None and emitted[0] == eos:    # (:3360-3365)
                row.active = False
                emitted = []
            if dedup and emitted and gen and gen[-1] == emitted[0]:  # (:3367-3376)
                emitted = []
            gen.extend(emitted)
            if not emitted:
                acc_i = [] if info is not None else None
        if info is not None:
            ginfo.extend(acc_i)
        row.proposed += k
        row.accepted += len(emitted)
        if emitted:                                      # sequence update with its own overlap rule (:3470-3572)
            acc, cur = list(emitted), row.seq
            c = min(5, len(cur), len(acc)) if dedup else 0
            if c > 0 and cur[-c:] == acc[:c]:
                if len(acc) > c:
                    acc = acc[c:]
                    if len(gen) >= c:
                        del gen[-c:]
                        if info is not None:
                            del ginfo[-c:]
                else:
                    acc = []
            row.seq = cur + acc
        if len(gen) >= max_tokens:                       # (:3589-3590)
            row.active = False

    @staticmethod
    def _rules_single(row: _Row, k: int, a: int, d: List[int], t: List[int], max_tokens: int,
                      eos: Optional[int]) -> None:
        """One step of generate() (pipeline.py:1190-1272): draft ids cut to the budget, or one
        base token when nothing was accepted."""
        remaining = max_tokens - len(row.generated)
        new = [int(x) for x in d[: min(a, max(remaining, 0))]] if a > 0 else ([int(t[0])] if remaining > 0 else [])
        row.proposed += k
        row.accepted += a
        row.generated.extend(new)
        row.seq = row.seq + new
        if len(row.generated) >= max_tokens:
            row.active = False
        elif eos is not None and row.generated and row.generated[-1] == eos:
            row.active = False

    # ------------------------------------------------------------------ the loop
    def start_session(self, prompts: List[List[int]], max_tokens: int, emit_mode: int,
                      sampling: Union[None, Dict[str, Any], StepOptions] = None, step_limit: Optional[int] = None,
                      self_draft: bool = False, share_prefix: bool = False, grammar=None, sampling_params=None,
                      draft_confidence: Optional[float] = None, draft_min_k: Optional[int] = None, logprobs=None,
                      context_window: Optional[int] = None, attention_sinks: Optional[int] = None, **processors) -> "DecodeSession":
        """Prefill + device state for a batch of rows; `advance()` then runs one step at a time
        (generate / generate_batch drive it to completion, bench.py times exact step counts).
        share_prefix: rows that hold the same prompt, or a common prefix of >= min_shared_prefix tokens, pay for it once
        (DecodeSession). sampling: None (greedy), {"temperature", "top_k", "top_p", "seed"} or a StepOptions. processors:
        repetition_penalty, presence_penalty, frequency_penalty, logit_bias, bad_token_ids, allowed_token_ids; identity values
        leave the stage off. grammar: a TokenFSM, or a list with one entry per prompt (None: that row is unconstrained).
        sampling_params: one SamplingParams per prompt (in place of `sampling` and of penalty arguments); only they are gated.
        draft_confidence / draft_min_k: the confidence-gated draft length (generate_batch), the bonus-token emit mode only.
        logprobs: per-token log-probs (True / 0: the chosen token's; 1..20: that many alternatives too), the bonus-token emit mode
        only; every row's token_info then stays parallel to its generated tokens.
        context_window / attention_sinks: the rolling context window (core/rolling.py), the bonus-token emit mode only: the caches
        are sized by the window, not by max_tokens, and a row rolls whenever its next launches would not fit."""
        if sampling_params is not None and sampling is not None:
            raise ValueError("sampling_params carries every request's own parameters: a `sampling` description cannot be given with it")
        session_rule(self, StepOptions(), emit_mode, self_draft, sampling_params, HipSpecDec.EMIT_BONUS)   # (its refusals come first)
        options = (StepOptions.from_sampling(sampling) if sampling_params is None else
                   row_options(self, sampling_params, len(prompts), 1, None, processors, self_draft))
        options = with_stage(self, options, processors, grammar, len(prompts))
        options = session_rule(self, options, emit_mode, self_draft, sampling_params, HipSpecDec.EMIT_BONUS)   # (a device acceptance rule)
        options = session_confidence(self, options, emit_mode, self_draft, draft_confidence, draft_min_k, HipSpecDec.EMIT_BONUS)
        options = lpmod.session_logprobs(self, options, emit_mode, self_draft, logprobs, HipSpecDec.EMIT_BONUS)
        window = rolling.session_window(self, context_window, attention_sinks, emit_mode, self_draft, share_prefix, HipSpecDec.EMIT_BONUS, prompts)
        return DecodeSession(self, prompts, max_tokens, emit_mode, options, step_limit, self_draft, share_prefix, window=window)

    def _decode(self, prompts: List[List[int]], max_tokens: int, emit_mode: int, step_limit: int,
                options: Optional[StepOptions] = None, self_draft: bool = False, share_prefix: bool = False, window=None):
        t_start = time.time()
        sess = DecodeSession(self, prompts, max_tokens, emit_mode, options, step_limit, self_draft, share_prefix, window=window)
        while sess.any_active():    # every row stops after `step_limit` steps of its own
            if not sess.advance():
                break
        sess.finish()
        torch.cuda.synchronize()
        st = sess.stats
        st["total_ms"] = (time.time() - t_start) * 1e3
        st["k"] = sess.k
        return sess.rows, st

    def _medusa_random(self) -> bool:
        return (self.config.get("draft_mode") == "medusa" and self.medusa_heads is None
                and self.config.get("medusa", {}).get("head_init", "tie") == "random")

    def _draft_medusa_random(self, seq: List[int], k: int, temperature: float, row: int, rows: int):
        """_run_medusa_hf (pipeline.py:655-763) on the HIP engine: the target's last hidden state (after the final norm) of
        the last token; `num_heads` FRESH heads per call — torch.nn.Linear's default init, then normal_(0, 0.02), both from
        the global torch generator on the host, exactly as the reference creates them; every head still in range draws one
        token per proposal with torch.multinomial from softmax(logits / T) (global generator, host); the proposal of a step
        is head 0's draw. The hidden state does not move between proposals, so every head's logits are computed once
        (a [num_heads x V x d] product on the device, bf16 as the engine holds weights). Returns (ids [1,k], logits [1,k,V])."""
        h = self.base_lm.last_hidden_state(torch.tensor([seq], dtype=torch.long), row=row, rows=rows)   # [1,1,d] fp32, bf16 values
        num_heads = int(self.config.get("medusa", {}).get("num_heads", 2))
        d, V = h.shape[-1], self.base_lm.vocab_size
        heads = []
        for _ in range(num_heads):
            head = torch.nn.Linear(d, V, bias=False)
            torch.nn.init.normal_(head.weight, 0, 0.02)
            heads.append(head.weight.detach().to(torch.bfloat16))
        hw = torch.stack(heads).to("cuda").float()                                    # [H,V,d], bf16 values
        logits = torch.matmul(hw, h.view(-1)).to(torch.bfloat16).float().cpu()         # [H,V] bf16-rounded, on the host for the draws
        ids = []
        for step in range(k):
            toks = []
            for hi in range(min(num_heads, k - step)):
                lg = logits[hi].view(1, 1, -1)
                if temperature > 0:
                    lg = lg / temperature
                toks.append(torch.multinomial(torch.softmax(lg, dim=-1).squeeze(1), 1))
            ids.append(toks[0])
        d_ids = torch.cat(ids, dim=1).to("cuda")
        d_logits = logits[0].view(1, 1, -1).expand(1, k, -1).contiguous().to("cuda")
        return d_ids, d_logits

    def _decode_host_policy(self, prompts: List[List[int]], max_tokens: int, emit_mode: int, step_limit: int,
                            temperature: float = 0.7, sample_t: Optional[float] = None, sample_kwargs: Optional[Dict[str, Any]] = None):
        """The reference's verification for the logit-threshold policies (speculative_scheduler.py:294-368, policies.py:213-396;
        pipeline.py:1019-1100 and :2397-3030): per row and step, K greedy draft tokens with their logits, the base model's
        OWN K greedy tokens with their logits from the same prefix (K one-token HIP forwards each, over the rows' cached
        prefixes), the policy on the device logits, then the same host rules as the device step. A full acceptance takes
        the extra base forward the reference takes (:3199-3206).
        sample_t (generate(do_sample=True), pipeline.py:1019-1027): the draft's tokens are DRAWN at that temperature (a draft that
        draws EOS is shorter, and `proposed` counts what came back, :1122); verification stays greedy; the one base token of a
        zero-accept step is drawn too (:1217-1224) — the step's last draw."""
        skw = dict(sample_kwargs or {})
        t_start = time.time()
        rows = [_Row(list(p)) for p in prompts]
        for r in rows:
            if not r.seq:
                raise ValueError("empty prompt")
        eos = self.base_lm.get_tokenizer_info().get("eos_token_id")
        n = len(rows)
        medusa = self._medusa_random()
        for lm in (self.base_lm, self.draft_lm):
            if lm is not None:
                lm.clear_kv_cache()
        stats = {"steps": 0, "resyncs": 0, "proposed": 0, "accepted": 0, "device_ms": 0.0, "void_row_steps": 0}
        step = 0
        while any(r.active for r in rows):
            step += 1
            ctx = {"step": step, "generated_tokens": max(len(r.generated) for r in rows),
                   "acceptance_rate": stats["accepted"] / max(stats["proposed"], 1)}
            k = int(self.controller.get_k(step, ctx))
            if k <= 0:
                break
            t0 = time.time()
            for b, r in enumerate(rows):
                if not r.active:
                    continue
                ids = torch.tensor([r.seq], dtype=torch.long)
                kb = k   # proposals of this row in this step
                if medusa:
                    d_ids, d_logits = self._draft_medusa_random(r.seq, kb, temperature, b, n)
                elif sample_t is not None:
                    d_ids, d_logits = self.draft_lm.generate_tokens(ids, kb, temperature=sample_t, do_sample=True, row=b, rows=n, **skw)
                    kb = int(d_ids.shape[1])
                else:
                    d_ids, d_logits = self.draft_lm.generate_tokens(ids, kb, do_sample=False, row=b, rows=n)
                b_ids, b_logits = self.base_lm.generate_tokens(ids, kb, do_sample=False, row=b, rows=n)
                a, _info = self.policy.accept_tokens(d_ids, b_ids, d_logits, b_logits)
                d, t = d_ids[0].tolist(), b_ids[0].tolist()
                if sample_t is not None and a == 0:
                    fb, _ = self.base_lm.generate_tokens(ids, 1, temperature=sample_t, do_sample=True, row=b, rows=n, **skw)
                    t[0] = int(fb[0, 0])
                if a == kb and emit_mode == HipSpecDec.EMIT_BONUS:
                    more, _ = self.base_lm.generate_tokens(torch.tensor([r.seq + t], dtype=torch.long), 1, do_sample=False, row=b, rows=n)
                    t.append(int(more[0, 0]))
                else:
                    t.append(-1)
                acc0 = r.accepted
                if emit_mode == HipSpecDec.EMIT_BONUS:
                    self._rules_batch(r, kb, a, t, max_tokens, eos)
                else:
                    self._rules_single(r, kb, a, d, t, max_tokens, eos)
                r.steps += 1
                stats["proposed"] += kb
                stats["accepted"] += r.accepted - acc0
                if r.active and r.steps >= step_limit:
                    r.active = False
            stats["device_ms"] += (time.time() - t0) * 1e3
        torch.cuda.synchronize()
        stats["steps"] = max((r.steps for r in rows), default=0)
        stats["total_ms"] = (time.time() - t_start) * 1e3
        stats["k"] = int(getattr(self.controller, "k", 0) or 0)
        return rows, stats

    def _decode_rejection(self, prompts: List[List[int]], max_tokens: int, step_limit: int):
        """policy="rejection" (opt-in speculative sampling, policies.RejectionSamplingPolicy; generate_batch): per row and
        step K draft tokens DRAWN from the draft's distribution (one HIP forward each over the row's cached prefix), ONE
        K+1-token parallel verify pass of the target over them, the accept test on the device logits, the correction /
        bonus token drawn from the distribution the policy returns. Every uniform comes from the policy's generator."""
        t_start = time.time()
        pol = self.policy
        pol.reseed()
        rows = [_Row(list(p)) for p in prompts]
        eos = self.base_lm.get_tokenizer_info().get("eos_token_id")
        n = len(rows)
        for lm in (self.base_lm, self.draft_lm):
            lm.clear_kv_cache()
        stats = {"steps": 0, "resyncs": 0, "proposed": 0, "accepted": 0, "accepted_draft": 0, "device_ms": 0.0, "void_row_steps": 0}
        step = 0
        while any(r.active for r in rows):
            step += 1
            # the controller sees the STRICT rate (accepted draft tokens / proposed, <= 1): the reported `accepted` counts the
            # bonus / correction token as generate_batch does and would read (k+1)/k on a fully accepted step
            ctx = {"step": step, "generated_tokens": max(len(r.generated) for r in rows),
                   "acceptance_rate": stats["accepted_draft"] / max(stats["proposed"], 1)}
            k = int(self.controller.get_k(step, ctx))
            if k <= 0:
                break
            for b, r in enumerate(rows):
                if not r.active:
                    continue
                drafted, d_logits = [], []
                for _ in range(k):
                    _, lg = self.draft_lm.generate_tokens(torch.tensor([r.seq + drafted], dtype=torch.long), 1, do_sample=False, row=b, rows=n)
                    d_logits.append(lg[:, 0])
                    drafted.append(pol.draw(pol.distributions(lg[0, 0]), float(pol.uniforms(1)[0])))
                d_ids = torch.tensor([drafted], dtype=torch.long, device="cuda")
                _, b_logits = self.base_lm.verify_tokens(torch.tensor([r.seq], dtype=torch.long), d_ids, row=b, rows=n)
                a, info = pol.accept_tokens(d_ids, d_ids, torch.stack(d_logits, dim=1), b_logits)
                nxt = pol.draw(info["next_distribution"], float(pol.uniforms(1)[0]))
                emitted = drafted[:a] + [nxt]
                if eos is not None and eos in emitted:
                    emitted = emitted[: emitted.index(eos) + 1]
                    r.active = False
                emitted = emitted[: max(max_tokens - len(r.generated), 0)]   # this path is the product's own: no overshoot of the budget
                r.seq = r.seq + emitted
                r.generated.extend(emitted)
                r.proposed += k
                r.accepted += a + 1                        # the bonus / correction token counted, as generate_batch counts it
                r.steps += 1
                stats["proposed"] += k
                stats["accepted"] += a + 1
                stats["accepted_draft"] += a
                if len(r.generated) >= max_tokens or r.steps >= step_limit:
                    r.active = False
        torch.cuda.synchronize()
        stats["steps"] = max((r.steps for r in rows), default=0)
        stats["total_ms"] = (time.time() - t_start) * 1e3
        stats["k"] = int(getattr(self.controller, "k", 0) or 0)
        return rows, stats

    # ------------------------------------------------------------------ public API
    def grammar_from_regex(self, pattern: str, eos_id: Optional[int] = None):
        """The TokenFSM of a regular expression over the target's tokenizer (specdec_hip.grammar.from_tokenizer; its limitation
        for byte-level BPE vocabularies is written there). eos_id defaults to the pipeline's EOS; a pipeline without one must
        pass it. Compiled once per (pattern, eos_id) and kept."""
        from specdec_hip.grammar import from_tokenizer

        if eos_id is None:
            eos_id = self.base_lm.get_tokenizer_info().get("eos_token_id")
            if eos_id is None:
                raise ValueError("grammar_from_regex: the pipeline has no EOS token; pass eos_id")
        cache = self._grammar_regexes
        if (pattern, int(eos_id)) not in cache:
            cache[(pattern, int(eos_id))] = from_tokenizer(pattern, self.base_lm._tokenizer, self.base_lm.vocab_size, int(eos_id))
        return cache[(pattern, int(eos_id))]

    _spec_sampling_config = spec_options     # the `sampling` of policy="rejection" with backend="device", for start_session

    def generate(self, prompt: PromptLike, max_tokens: Optional[int] = None, temperature: Optional[float] = None,
                 do_sample: Optional[bool] = None, **kwargs) -> Dict[str, Any]:
        """Single-prompt speculative decoding (reference :893-1413): accepted tokens are the
        draft's, no bonus token, a zero-accept step emits one base token."""
        t_begin = time.time()
        rolling.refuse_single(self, kwargs)
        call = resolve(self, [prompt], max_tokens, temperature, do_sample, kwargs, grammar=kwargs.pop("grammar", None),
                       sampling_params=kwargs.pop("sampling_params", None), share_prefix=kwargs.get("share_prefix"), n=kwargs.get("n", 1),
                       single=True, draft_confidence=kwargs.pop("draft_confidence", None), draft_min_k=kwargs.pop("draft_min_k", None),
                       logprobs=kwargs.pop("logprobs", None))
        if call.route == "host_policy":
            rows, st = self._decode_host_policy(call.ids, call.max_tokens, HipSpecDec.EMIT_DRAFT, step_limit=2 * call.max_tokens,
                                                temperature=call.temperature, sample_t=call.sample_t,
                                                sample_kwargs={k: kwargs[k] for k in ("top_k", "top_p") if k in kwargs})
        else:
            rows, st = self._decode(call.ids, call.max_tokens, HipSpecDec.EMIT_DRAFT, step_limit=2 * call.max_tokens,
                                    options=call.options, self_draft=call.self_draft)
        r = rows[0]
        total_ms = (time.time() - t_begin) * 1e3
        self.metrics = {"total_proposed": r.proposed, "total_accepted": r.accepted, "total_steps": st["steps"],
                        "total_verification_time_ms": st["device_ms"], "total_generation_time_ms": total_ms,
                        "kv_appended_tokens_total": len(r.generated), "kv_append_time_ms": 0.0}
        text = self.base_lm.decode(r.generated) if r.generated else ""
        n = len(r.generated)
        return {
            "text": text, "generated_tokens": list(r.generated), "latency_ms": total_ms,
            "proposed": r.proposed, "accepted": r.accepted,
            "acceptance_rate": r.accepted / r.proposed if r.proposed > 0 else 0.0,
            "tokens_per_sec": n / (total_ms / 1e3) if total_ms > 0 else 0.0, "steps": st["steps"],
            "verification_time_ms": st["device_ms"], "generation_time_ms": total_ms,
            "kv_appended_tokens_total": n, "kv_append_time_ms": 0.0, "kv_append_enabled": True,
            "kv_append_backend": "hip", **self._sysinfo(),
        }

    def generate_batch(self, prompts: Sequence[PromptLike], max_tokens: Optional[int] = None,
                       temperature: Optional[float] = None, do_sample: Optional[bool] = None,
                       share_prefix: bool = False, n: int = 1, grammar=None, sampling_params=None,
                       draft_confidence: Optional[float] = None, draft_min_k: Optional[int] = None, logprobs=None,
                       best_of: Optional[int] = None, context_window: Optional[int] = None, attention_sinks: Optional[int] = None,
                       **kwargs) -> List[Dict[str, Any]]:
        """Batched speculative decoding (reference :1605-3931): base tokens + bonus token per
        step, step-count bound, no truncation to max_tokens. Rows are independent sequences.

        share_prefix (opt-in; not in the reference): rows pay for a prompt once. Rows whose prompts are equal are prefilled
        once, on the first of them, and the others are forked from it in both engines (csrc/kv_fork.hip: a copy of the KV, or
        shared pages with paged KV); a row that has only a prefix of >= `min_shared_prefix` tokens (config key, default 32) in
        common with a row already in the cache is forked over that prefix and forwards the rest of its prompt from there.
        With equal prompts the result is that of the unshared run, token for token. With a partial prefix the suffix is
        computed in other chunks than a whole-prompt prefill uses, so it may differ from the unshared run at bf16 rounding
        level — which is why sharing is opt-in. `n` > 1: every prompt becomes n adjacent rows (n samples of it: do_sample=True,
        or policy="rejection" with backend="device", whose per-row Philox streams make the rows differ), results come back
        prompt-major; implies share_prefix. Both are for the captured step (longest_prefix, device sampling, rejection on
        the device) and are refused elsewhere. batch_metrics carries prefilled_rows / forked_rows / shared_positions.

        grammar (opt-in; not in the reference): a specdec_hip.grammar.TokenFSM, or a list with one entry per prompt (None: that
        row is unconstrained). A row under a grammar emits only token sequences its automaton allows, draft and target alike
        (the mask is a line of the step's logit-processor stage), ends on the automaton's eos, and is exempt from the overlap /
        de-duplication rules, which would delete tokens the automaton has consumed; greedy output is the target's own greedy
        decoding under the mask, token for token.

        sampling_params (opt-in; not in the reference): one SamplingParams per prompt (expanded with n) — every request its own
        temperature (0: greedy), top_k, top_p, seed and penalties, read by the step's kernels row by row (step_options).
        Under policy="longest_prefix" the step samples the bonus token; under policy="rejection" with backend="device" it is
        speculative sampling. A request's Philox stream is its index among the call's rows.

        draft_confidence (opt-in; config key draft_confidence_threshold; HF assisted generation's assistant_confidence_threshold):
        a row stops drafting after the first draft forward i + 1 >= draft_min_k (default 1) whose confidence — the draft's
        softmax probability of its own token — is below the threshold; the token drawn at low confidence is still proposed.
        Decided on the device between two draft forwards of the captured step (sd_specdec_set_draft_confidence): only the row's
        first k proposals count, a draft forward no row needs returns at entry, every step starts at K again. Greedy output is
        the target's own greedy decoding whatever k was. Results carry `k_trace`; `proposed` counts the k of every step;
        batch_metrics carries mean_k and draft_forwards_skipped. For the draft-model mode with a fixed K, greedy or do_sample;
        refused next to speculative sampling, the device acceptance rules, logit processors, grammars and sampling_params.

        logprobs (opt-in; not in the reference): True or 0 — every result gains `logprobs` (one float per generated token),
        `token_ranks` and `cumulative_logprob` (their Python float sum, in emission order); 1..20 — also `top_logprobs`, that
        many (id, logprob) alternatives per token. Computed on the device inside the step that emits the token
        (sd_specdec_set_logprobs), from the verify row the token was checked against or drawn from: the target's distribution at
        temperature 1 after the logit processors and the grammar, before top-k / top-p shaping. For the captured step with a
        draft model and a fixed K, in every select mode; refused on the host loops, with implementation='fake', medusa / eagle /
        self-draft, adaptive K, draft_confidence and generate().

        best_of=m >= n (opt-in): every prompt decodes m rows (the `n` machinery: one shared prompt, a Philox stream per row) and
        the n with the highest cumulative_logprob come back, best first, ties to the lower row. Implies logprobs; needs a
        sampling mode (greedy rows are all equal). batch_metrics carries best_of.

        context_window=W / attention_sinks=S (opt-in; config keys of the same names, S defaults to 4; not in the reference): the rolling
        context window. The caches are sized by W (plus the slack the launches in flight need), not by prompt + max_tokens, and
        generation length is no longer bound by the cache or by the models' max_pos. A row's cache keeps its first S positions and
        the most recent ones: when its next launches would not fit within W, the `drop` positions after the sinks are evicted in
        both engines (csrc/kv_evict.hip: the survivors move down and their keys are re-rotated to their new positions), at the
        session's repair point, and the row goes on. Results carry `evictions`, a list of (tokens generated before the roll, drop):
        the output is the target's own greedy decoding over the rolled cache GIVEN that schedule, and the schedule depends on where
        the step boundaries fall, hence on acceptance. batch_metrics carries evictions / evicted_positions. For the captured step
        with a draft model and a fixed K, in every select mode, with processors, grammars, sampling_params, logprobs and
        draft_confidence; refused with paged KV, GPT-2 models, the host loops, implementation='fake', medusa / eagle / self-draft,
        adaptive K, share_prefix / n, generate(), and a prompt the window has no room for (prompts are not truncated)."""
        if not prompts:
            return []
        m_best = lpmod.check_best_of(best_of, n)
        if m_best is not None:
            n_keep, n, logprobs = int(n), m_best, (0 if lpmod.check_logprobs(logprobs) is None else logprobs)
        call = resolve(self, prompts, max_tokens, temperature, do_sample, kwargs, share_prefix=share_prefix, n=n, grammar=grammar,
                       sampling_params=sampling_params, draft_confidence=draft_confidence, draft_min_k=draft_min_k, logprobs=logprobs)
        if m_best is not None:
            lpmod.check_best_of_mode(call.options)
        window = rolling.call_window(self, context_window, attention_sinks, call)
        if call.route == "fake":
            return [self.generate(p, max_tokens=max_tokens, temperature=temperature, do_sample=do_sample, **kwargs) for p in prompts]
        prompts, max_tokens = call.prompts, call.max_tokens
        if call.route == "host_rejection":
            rows, st = self._decode_rejection(call.ids, max_tokens, step_limit=max_tokens)
        elif call.route == "host_policy":
            rows, st = self._decode_host_policy(call.ids, max_tokens, HipSpecDec.EMIT_BONUS, step_limit=max_tokens)
        else:
            rows, st = self._decode(call.ids, max_tokens, HipSpecDec.EMIT_BONUS, step_limit=max_tokens, options=call.options,
                                    self_draft=call.self_draft, share_prefix=call.share_prefix, **({} if window is None else {"window": window}))
        total_ms = st["total_ms"]
        tot_prop = sum(r.proposed for r in rows)
        tot_acc = sum(r.accepted for r in rows)
        tot_gen = sum(len(r.generated) for r in rows)
        batch_metrics = {
            "total_proposed": tot_prop, "total_accepted": tot_acc, "total_generated_tokens": tot_acc,
            "total_steps": st["steps"], "total_draft_time_ms": 0.0, "total_verification_time_ms": st["device_ms"],
            "total_generation_time_ms": total_ms, "total_time_ms": total_ms,
            "tokens_per_sec": tot_acc / (total_ms / 1e3) if total_ms > 0 else 0.0,
            "emitted_tokens": tot_gen, "resyncs": st["resyncs"], "k": st["k"],
            # proposals that counted per row and step (K unless a row's k moves), and — confidence-gated draft length — the draft
            # forwards of the consumed steps that no row the host took tokens from needed
            "mean_k": tot_prop / max(sum(r.steps for r in rows), 1), "draft_forwards_skipped": st.get("draft_forwards_skipped", 0),
            **{key: st.get(key, 0) for key in ("prefilled_rows", "forked_rows", "shared_positions")},
            **({} if window is None else {key: st.get(key, 0) for key in ("evictions", "evicted_positions")}),
        }
        out = []
        for i, (p, r) in enumerate(zip(prompts, rows)):
            n = len(r.generated)
            text = self.base_lm.decode(r.generated) if r.generated else ""
            tps = n / (total_ms / 1e3) if total_ms > 0 else 0.0
            out.append({
                "prompt": p, "text": text, "generated_text": text, "generated_tokens": list(r.generated),
                "num_generated": n, "batch_index": i, "batch_size": len(rows),
                "latency_ms": total_ms / n if n else 0.0, "total_time_ms": total_ms,
                "tokens_per_sec": tps, "throughput_tokens_per_sec": tps,
                "acceptance_rate": tot_acc / max(tot_prop, 1),   # batch-wide, as the reference (:3834)
                "proposed": r.proposed, "accepted": r.accepted,
                "draft_avg_ms": 0.0, "verify_avg_ms": st["device_ms"] / max(st["steps"], 1),
                "batch_metrics": batch_metrics, "kv_append_enabled": True, "kv_append_backend": "hip",
                "kv_appended_tokens": n, "kv_append_time_ms": 0.0, "sequence": list(r.seq),
                **({"k_trace": list(r.k_trace)} if r.k_trace else {}),     # per-row adaptive K: the k of each of the row's steps
                **lpmod.result_fields(r, call.options.logprobs),
                **({} if window is None else {"evictions": list(r.evictions), "window_rebuilds": list(r.rebuilds)}),
            })
        if m_best is not None:
            batch_metrics["best_of"] = m_best
            out = lpmod.pick_best(out, m_best, n_keep)
        return out

    def generate_many(self, prompts: Sequence[PromptLike], max_tokens: Optional[int] = None, batch_size: int = 8,
                      temperature: Optional[float] = None, do_sample: Optional[bool] = None, share_prefix: bool = False, n: int = 1,
                      grammar=None, sampling_params=None, draft_confidence: Optional[float] = None,
                      draft_min_k: Optional[int] = None, logprobs=None, context_window: Optional[int] = None,
                      attention_sinks: Optional[int] = None, **kwargs) -> List[Dict[str, Any]]:
        """Continuous batching over a list of prompts: `batch_size` rows decode together (generate_batch
        semantics per row) and a finished row's slot is handed to the next waiting prompt at once, instead of
        the reference harness' fixed batches that idle until their slowest row ends
        (comprehensive_k_sweep.py:444-535). Rows are independent, so every result equals the prompt's own
        generate_batch([prompt]) run. Results come back in prompt order.
        share_prefix / n: as generate_batch — a prompt admitted to a slot is also compared with the rows the session holds at
        that moment (finished rows whose caches are still intact included), so a system prompt in front of many questions is
        computed once per session, not once per question; with n > 1 the results are prompt-major (n per prompt).
        grammar: as generate_batch, one entry per prompt; a prompt admitted to a slot starts in its own automaton's start state.
        sampling_params: as generate_batch, one entry per prompt; a prompt admitted to a slot brings its own entry, its seed and
        its Philox stream (its index among the call's rows) with it — the slot's table entry, stream id and draw counter are
        rewritten on the loop's stream and the captured step is kept.
        draft_confidence / draft_min_k: as generate_batch; the device keeps no per-row state for it, so an admission sets nothing.
        logprobs: as generate_batch (best_of is a generate_batch argument and is refused here).
        context_window / attention_sinks: as generate_batch; a prompt admitted to a slot starts with nothing evicted, and must fit the
        window as the first ones must."""
        if not prompts:
            return []
        lpmod.refuse_best_of(kwargs)
        call = resolve(self, prompts, max_tokens, temperature, do_sample, kwargs, share_prefix=share_prefix, n=n, grammar=grammar,
                       sampling_params=sampling_params, policy_routes=False, draft_confidence=draft_confidence, draft_min_k=draft_min_k,
                       logprobs=logprobs)
        prompts, ids, max_tokens, options = call.prompts, call.ids, call.max_tokens, call.options
        window = rolling.call_window(self, context_window, attention_sinks, call)
        n_slots = max(1, min(int(batch_size), len(ids)))
        order = sorted(range(len(ids)), key=lambda i: -len(ids[i]))   # the longest prompts size the session
        first = order[:n_slots]
        waiting = [i for i in range(len(ids)) if i not in set(first)]
        t_start = time.time()
        sess = DecodeSession(self, [ids[i] for i in first], max_tokens, HipSpecDec.EMIT_BONUS, options.rows(first), max_tokens,
                             share_prefix=call.share_prefix, **({} if window is None else {"window": window}))
        owner: List[Optional[int]] = list(first)
        done: Dict[int, Any] = {}
        while len(done) < len(ids):
            if sess.any_active():
                if not sess.advance():
                    break
            for b, r in enumerate(sess.rows):
                if owner[b] is not None and not r.active:
                    done[owner[b]] = (r, (time.time() - t_start) * 1e3)
                    owner[b] = None
                    if waiting:
                        nxt = waiting.pop(0)
                        sess.admit(b, ids[nxt], -1 if options.fsm is None else options.grammar_starts[nxt],
                                   params=None if options.row_params is None else options.row_params[nxt], index=nxt)
                        owner[b] = nxt
            if not sess.any_active() and not waiting and all(o is None for o in owner):
                break
        sess.finish()
        torch.cuda.synchronize()
        total_ms = (time.time() - t_start) * 1e3
        tot_tok = sum(len(r.generated) for r, _ in done.values())
        out = []
        for i, p in enumerate(prompts):
            r, t_ms = done[i]
            n = len(r.generated)
            text = self.base_lm.decode(r.generated) if r.generated else ""
            out.append({"prompt": p, "text": text, "generated_text": text, "generated_tokens": list(r.generated), "num_generated": n,
                        "batch_index": i, "batch_size": n_slots, "latency_ms": t_ms, "total_time_ms": total_ms,
                        "tokens_per_sec": n / (t_ms / 1e3) if t_ms > 0 else 0.0,
                        "throughput_tokens_per_sec": tot_tok / (total_ms / 1e3) if total_ms > 0 else 0.0,
                        "acceptance_rate": r.accepted / max(r.proposed, 1), "proposed": r.proposed, "accepted": r.accepted,
                        "steps": r.steps, "sequence": list(r.seq), "kv_append_enabled": True, "kv_append_backend": "hip",
                        **({"k_trace": list(r.k_trace)} if r.k_trace else {}), **lpmod.result_fields(r, options.logprobs),
                        **({} if window is None else {"evictions": list(r.evictions), "window_rebuilds": list(r.rebuilds)}),
                        "batch_metrics": {**({} if window is None else {key: sess.stats[key] for key in ("evictions", "evicted_positions")}),"total_steps": sess.stats["steps"], "device_steps": sess.step, "resyncs": sess.stats["resyncs"],
                                          "void_row_steps": sess.stats["void_row_steps"], "k": sess.k,
                                          "mean_k": sess.stats["proposed"] / max(sum(x.steps for x, _ in done.values()), 1),
                                          "draft_forwards_skipped": sess.stats.get("draft_forwards_skipped", 0),
                                          **{key: sess.stats[key] for key in ("prefilled_rows", "forked_rows", "shared_positions")}}})
        return out

    def draft_agreement(self, text_or_ids: PromptLike, temperature: float = 1.0, chunk: int = 256) -> Dict[str, Any]:
        """How well the draft fits the target on a text, without generating: the sequence is teacher-forced through both models
        (HipLM.score_logits, the prefill route of score) in chunks of <= `chunk` positions and the two logit rows of every
        position are reduced on the device (specdec_hip.ops.spec_agreement) — the [n][V] logits stay in two reusable
        [chunk][V] bf16 buffers and never pass through torch arithmetic.

        Returns, for positions 0..n-2 (the predictions of tokens 1..n-1): `alpha` (per-position acceptance probability of
        speculative sampling at `temperature`, sum_v min(p, q)), `kl` (KL(target || draft)), `agree` (equal argmax: what greedy
        verification accepts), their means `mean_alpha` / `mean_kl` / `greedy_agreement`, and `expected_tokens_per_step`
        {"sampling": {K: ..}, "greedy": {K: ..}} for K = 1..8 (expected_tokens_per_step over alpha, and over agree as 0 / 1).
        `expected_tokens_per_step` is an estimate on the contexts of the GIVEN text: in a real step the later positions of a
        window condition on the draft's own continuation, not on the text's tokens, so it is a guide to choosing K, not a
        measurement of a run. Both cache rows 0 then hold the first n-1 tokens."""
        from specdec_hip.ops import spec_agreement

        if self._fake:
            raise NotImplementedError("draft_agreement needs the HIP models (implementation='hip'): the fake models have no logits on the device")
        mode = self.config.get("draft_mode", "vanilla")
        if mode in ("medusa", "eagle") or self.draft_lm is None:
            raise NotImplementedError(f"draft_agreement compares a separate draft model with the target; draft_mode={mode!r} drafts from "
                                      "the target's own hidden state (no draft model / a different draft input)")
        for lm in (self.base_lm, self.draft_lm):
            if not hasattr(lm, "score_logits"):
                raise NotImplementedError("draft_agreement needs models with score_logits (HipLM)")
        ids = self._encode(text_or_ids)
        if len(ids) < 2:
            raise ValueError(f"draft_agreement: {len(ids)} token(s); an agreement needs at least 2")
        if not (float(temperature) > 0.0):
            raise ValueError(f"draft_agreement: temperature {temperature} (must be > 0)")
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f"draft_agreement: chunk={chunk}")
        m = len(ids) - 1                                   # positions whose prediction has a token to be compared with
        V, dev = self.base_lm.vocab_size, self.base_lm.device
        c = min(chunk, m)
        bufs = [torch.empty((c, V), dtype=torch.bfloat16, device=dev) for _ in range(2)]
        alpha, kl, agree = [], [], []
        for p0 in range(0, m, c):
            part = ids[p0:min(p0 + c, m)]
            q, _ = self.draft_lm.score_logits(part, pos0=p0, out=bufs[0], reserve=m)
            p, _ = self.base_lm.score_logits(part, pos0=p0, out=bufs[1], reserve=m)
            a, k, g, _, _ = spec_agreement(q, p, temperature)
            alpha.append(a)
            kl.append(k)
            agree.append(g)
        alpha = torch.cat(alpha).cpu().tolist()
        kl = torch.cat(kl).cpu().tolist()
        agree = [bool(x) for x in torch.cat(agree).cpu().tolist()]
        return {"alpha": alpha, "kl": kl, "agree": agree, "positions": m, "temperature": float(temperature),
                "mean_alpha": sum(alpha) / m, "mean_kl": sum(kl) / m, "greedy_agreement": sum(agree) / m,
                "expected_tokens_per_step": {"sampling": expected_tokens_per_step(alpha),
                                             "greedy": expected_tokens_per_step([1.0 if x else 0.0 for x in agree])}}

    def _sysinfo(self) -> Dict[str, Any]:
        return {
            "mem_rss_mb": psutil.Process().memory_info().rss / 1024 / 1024,
            "cuda_mem_allocated_mb": float(torch.cuda.memory_allocated() / 1024 / 1024),
            "cuda_mem_peak_mb": float(torch.cuda.max_memory_allocated() / 1024 / 1024),
            "policy": self.policy.get_info(), "controller": self.controller.get_info(),
            "impl": "hip", "device": self.device, "dtype": "bfloat16", "amp_enabled": False,
            "base_model": self.base_lm.model_name, "draft_model": self.draft_lm.model_name if self.draft_lm is not None else "none (self-drafting from the base model: medusa heads tied to its lm_head / eagle extrapolation)",
            "draft_mode": self.config.get("draft_mode", "vanilla"),
        }


class DecodeSession:
    """One batch of rows being decoded: host mirror of the sequences + the device loop.

    The device advances its own state at the end of a step, so the NEXT steps do not need anything from
    the host. With a fixed K and greedy decoding `advance()` therefore keeps up to two steps launched: while
    the host applies the reference's rules to the record of step s, step s+1 is running and step s+2 is
    queued behind it (records land in two alternating pinned slots, each launch has its own completion
    event) — the GPU never waits for the host's turn. When the rules change a row (it finishes, or a
    de-duplication rewrites it), the steps already launched are void FOR THAT ROW: their records are
    ignored for it, no further step is launched until the queue has drained, the row's device state is
    repaired there (idle stream) and it rejoins. Steps are counted per row, so the reference's step bound
    applies to each row's own valid steps. Adaptive K, the sampled mode and the persistent Medusa heads
    keep the launch -> wait -> rules order (their next launch depends on the host, or on counters that a void
    step would disturb).

    share_prefix: the session records, per row, the token prefix whose KV the row's caches hold (the prompt without its last
    token, from the moment it was prefilled or forked until the slot is handed to another prompt). A row that enters — at the
    start, or through admit() — is forked from the recorded row it has the longest prefix in common with instead of being
    prefilled (SpeculativePipeline._absorb_row); stats counts prefilled_rows / forked_rows / shared_positions."""

    def __init__(self, pipe: SpeculativePipeline, prompts: List[List[int]], max_tokens: int, emit_mode: int,
                 options: Optional[StepOptions] = None, step_limit: Optional[int] = None, self_draft: bool = False, share_prefix: bool = False,
                 window: Optional[rolling.Window] = None):
        self.pipe, self.max_tokens, self.emit_mode = pipe, max_tokens, emit_mode
        self.options = o = options if options is not None else StepOptions()      # what the step does: greedy, sampled bonus token, spec
        other_step = self_draft or pipe._fake or bool(getattr(pipe.controller, "per_row", False))     # no draft model, or no fixed K
        if o.processors is not None and other_step:
            raise NotImplementedError("logit processors and grammars need the HIP step with a draft model and a fixed K")
        if share_prefix and pipe._fake:
            raise NotImplementedError("share_prefix needs the HIP engines (implementation='hip')")
        if o.row_params is not None and (len(o.row_params) != len(prompts) or len(o.row_ids) != len(prompts)):
            raise ValueError(f"sampling: {len(o.row_params)} rows / {len(o.row_ids)} ids for {len(prompts)} prompts")
        if o.row_params is not None and other_step:
            raise NotImplementedError("sampling_params need the HIP step with a draft model and a fixed K")
        if o.mode != "greedy" and emit_mode != HipSpecDec.EMIT_BONUS:
            raise ValueError("sampling is a generate_batch (bonus-token) feature")
        self._sampled, self._spec = o.mode != "greedy", o.mode == "spec"
        # a device acceptance rule: the record's emitted tokens are taken as they are (the draft's ids, then the target's token), the way
        # speculative sampling's are; a sampled token after them costs one draw per step and is never drawn again on the host
        self._accept = o.accept_rule is not None
        # the processor stage (None: off) has a counts row, and the grammar (None: off) a state, per cache row: both are (re)written wherever
        # the row's device state is. What admit() rewrites — start states, per-request parameters, stream ids — is the session's own
        self.grammar, self.processors, self.self_draft = o.fsm, o.processors, self_draft
        self.grammar_starts: List[int] = list(o.grammar_starts) if o.fsm is not None else [-1] * len(prompts)
        self.row_params = list(o.row_params) if o.row_params is not None else None
        self.row_ids: List[int] = list(o.row_ids) if o.row_ids is not None else list(range(len(prompts)))
        self._resample_state = False            # admit() without per-request parameters: draw counters restart at the next launch point
        self.step_limit = step_limit
        self.rows = [_Row(list(p)) for p in prompts]
        for r in self.rows:
            if not r.seq:
                raise ValueError("empty prompt")
        self.eos = pipe.base_lm.get_tokenizer_info().get("eos_token_id")
        ctl = pipe.controller
        k_max = getattr(ctl, "max_k", None) or getattr(ctl, "k", 4)
        self.need = max(len(r.seq) for r in self.rows) + max_tokens + 2 * int(k_max) + 8
        # per-row adaptive K: the step keeps the shape max_k, the device moves every row's own k (sd_specdec_set_adaptive)
        self.per_row = bool(getattr(ctl, "per_row", False))
        if self.per_row and self_draft:
            raise NotImplementedError("per-row adaptive K needs a draft model (the self-draft modes keep a fixed K)")
        if self.per_row:
            self.k = int(ctl.max_k)
            self.row_ctl = [self._new_row_controller() for _ in self.rows]
        else:
            self.k = pipe._effective_k(ctl.get_k(1, {"step": 1, "generated_tokens": 0, "acceptance_rate": 0.0}), self_draft)
        # confidence-gated draft length: the device rewrites every row's k inside each step and the record carries it; the host mirrors nothing
        self._conf = check_session(o, other_step, emit_mode == HipSpecDec.EMIT_BONUS, self.k)
        # per-token log-probs: the step describes every emitted token and the record carries it (None: off, else top_n)
        self._logprobs = lpmod.check_session(o, other_step, emit_mode == HipSpecDec.EMIT_BONUS)
        # the rolling context window (None: off): the caches are sized by the window and its slack, not by prompt + max_tokens
        self.window = rolling.check_session(window, other_step, emit_mode == HipSpecDec.EMIT_BONUS, share_prefix, self.k)
        if self.window is not None:
            self.need = self.window.l_max
        self.rt, self.loop = pipe._runtime(len(self.rows), self.need, self.k, emit_mode, self.self_draft, adaptive=self.per_row,
                                           **({} if self.window is None else {"windowed": True}))
        # positions a row may use: the cache rows and both models' position tables (a windowed row's positions are its cache's:
        # they stay below the window, which is within both tables, and nothing here stops it)
        self.pos_limit = min(self.rt["l_max"], pipe.base_lm.config.max_pos,
                             pipe.draft_lm.config.max_pos if not self_draft else pipe.base_lm.config.max_pos)
        if self.window is not None:
            rolling.refuse_paged([e for e in (self.rt["target"], self.rt["draft"]) if e is not None])
            assert self.rt["l_max"] >= self.window.l_max and all(self.window.fits(len(r.seq)) for r in self.rows)
        for r in self.rows:
            if len(r.seq) + 2 * self.k + 4 > self.pos_limit:
                raise ValueError(f"prompt of {len(r.seq)} tokens leaves no room for a step within {self.pos_limit} positions")
        self._engines = [e for e in (self.rt["target"], self.rt["draft"]) if e is not None]
        for e in self._engines:                 # paged KV: the previous session's pages go back to the pool
            for b in range(len(self.rows)):
                e.release(b)
        self._fresh: set = set()                # rows whose slot was handed to a new sequence (admit)
        self.stats = {"steps": 0, "resyncs": 0, "proposed": 0, "accepted": 0, "device_ms": 0.0, "void_row_steps": 0,
                      "prefilled_rows": 0, "forked_rows": 0, "shared_positions": 0}
        if self.window is not None:
            self.stats.update(evictions=0, evicted_positions=0)
        # share_prefix: per row, the tokens whose KV both caches hold at positions [0, len) — None: not to be relied on
        self._held: Optional[List[Optional[List[int]]]] = [None] * len(self.rows) if share_prefix else None
        pipe._prefill(self.rt, self.rows, self._held, self.stats)
        self.loop.join_current_stream()
        for b, r in enumerate(self.rows):
            pipe._set_row(self.loop, b, r)
        if self.per_row:
            params = (ctl.initial_k, ctl.min_k, ctl.max_k, ctl.step_size, ctl.target_acceptance_rate)
            if self.loop.adaptive_params != params:
                self.loop.set_adaptive(True, ctl.initial_k, ctl.min_k, ctl.max_k, ctl.step_size, ctl.target_acceptance_rate)
                self.loop.adaptive_params = params       # (enabling restarts every row; drops the captured step once)
            else:
                for b in range(len(self.rows)):
                    self.loop.set_adaptive_row(b, ctl.initial_k)
        self._configure_loop()
        self._configure_logprobs()
        self._stateful_draft = self_draft and (pipe.medusa_heads is not None or pipe._eagle())
        if self_draft and pipe._eagle():
            self.loop.reset_eagle()   # the reference keeps the state on the pipeline object, across generate() calls even; here a run starts clean
        self.step = 0
        # (persistent Medusa heads / EAGLE-lite: a void step would replace the next proposals with ones derived from stale
        # state — harmless for the tokens, but the counters would no longer be those of the in-order loop)
        # (speculative sampling advances a row's draw counter on the device by K + 1 per step, void steps included: the host's
        # in-order counters are written back whenever a row is repaired, so its steps can be queued ahead like greedy ones)
        self._early = ((isinstance(ctl, FixedKController) or self.per_row) and (not self._sampled or self._spec or self._accept)
                       and not self._stateful_draft
                       and os.environ.get("SPECDEC_EARLY_LAUNCH", "1") != "0")
        self._depth = 2 if self._early else 1
        if os.environ.get("SPECDEC_LAUNCH_DEPTH"):
            self._depth = max(1, min(2, int(os.environ["SPECDEC_LAUNCH_DEPTH"])))
        self._queue = deque()                # launched, not yet consumed: (launch index, set of rows it is void for)
        self._flagged: Dict[int, str] = {}   # rows whose device state must be repaired before the next launch
        # The persistent draft forward serves rows of up to 1280 positions (one CU walks a head's whole cache); a session whose
        # cache is sized for more starts on it all the same: every launch point tells the engines how far the rows can have
        # got by the end of the step (sd_model_set_length_hint), and when that moves a model to the other path the queue is
        # drained once and the step captured again (the captured kernels are correct at any length, only slower past the bound).
        self._hint()

    def _reach(self) -> int:
        """Cache positions the steps in flight plus one more can have reached on the longest row."""
        return max(len(r.seq) - r.evicted for r in self.rows) + (len(self._queue) + 2) * (self.k + 1) + 2

    def _hint(self) -> tuple:
        reach = self._reach()
        for e in self._engines:
            e.set_length_hint(reach)
        return tuple(e.persist_active(1) for e in self._engines)

    def any_active(self) -> bool:
        return any(r.active for r in self.rows)

    def _new_row_controller(self):
        """The host's mirror of a row's device-side controller: the same rule, already past the reference's first get_k
        (which reports acceptance_rate 0.0 before any step)."""
        m = self.pipe.controller.fork()
        m.get_k(1, {"step": 1, "generated_tokens": 0, "acceptance_rate": 0.0})
        return m

    def _configure_sampling(self) -> None:
        """Loops are cached per (batch, K) and outlive sessions: switch the one in use off what another run left on it and to this
        run's sampling mode, with every row's stream id and draw count. Every set_* call drops the captured step."""
        o, loop, spec = self.options, self.loop, self._spec
        if getattr(loop, "logprobs", None) not in (None, self._logprobs):    # (first of all: confidence gating's setter refuses next to it)
            loop.drain()
            loop.set_logprobs(None)
        want_conf = (o.draft_confidence, o.draft_min_k) if self._conf else None
        if getattr(loop, "draft_confidence", None) not in (None, want_conf):    # (first of all: every other mode's setter refuses next to it)
            loop.sync()
            loop.set_draft_confidence(None)
        if getattr(loop, "acceptance", None) is not None and not self._accept:        # (first: the other modes' setters refuse next to a rule)
            loop.sync()
            loop.set_acceptance(None)
        if loop.row_table is not None and self.row_params is None:   # a cached loop another run left a table on
            loop.sync()
            loop.set_row_sampling(None)
        if loop.spec_sampling and not spec:
            loop.sync()
            loop.set_spec_sampling(False)
        if loop.sampling and (not self._sampled or spec):
            loop.sync()
            loop.set_sampling(False)
        if self._sampled:
            loop.sync()
            if spec:
                if self.per_row or self.self_draft:
                    raise NotImplementedError("speculative sampling needs a draft model and a fixed K")
                loop.set_spec_sampling(True, o.temperature, o.seed, stream_ids=list(self.row_ids),
                                       draw_counts=[r.draws for r in self.rows], top_k=o.top_k, top_p=o.top_p)
            else:
                loop.set_sampling(True, o.temperature, o.top_k, o.top_p, o.seed,
                                  stream_ids=list(self.row_ids), draw_counts=[r.draws for r in self.rows])
            if self.row_params is not None:   # the mode's launches read table[b]; the scalars above are not in them
                loop.set_row_sampling(self.row_params)
        if self._accept:
            loop.sync()
            loop.set_acceptance(o.accept_rule, o.accept_temperature, o.accept_epsilon, o.accept_delta, o.accept_k)

    def _configure_loop(self) -> None:
        """_configure_sampling, then the processor stage: on or off, its bias rows, every row's counts (forked rows' own too), the grammar."""
        self._configure_sampling()
        lp, loop = self.processors, self.loop
        if lp is None:
            if loop.logit_processors:
                loop.sync()
                loop.set_logit_processors(False)
            # confidence-gated draft length, last: its setter refuses next to what the lines above have switched off by now
            if self._conf and loop.draft_confidence != (self.options.draft_confidence, self.options.draft_min_k):
                loop.drain()
                loop.set_draft_confidence(self.options.draft_confidence, self.options.draft_min_k)
            return
        loop.sync()
        loop.set_logit_processors(True, lp.rp, lp.presence, lp.frequency, bias=lp.bias is not None)
        if lp.bias is not None:
            with torch.cuda.stream(loop.stream_t):
                loop.logit_bias.copy_(lp.bias.to(loop.device).unsqueeze(0).expand_as(loop.logit_bias))
        for b in range(len(self.rows)):
            self._set_counts(b)
        if self.grammar is not None:
            loop.set_grammar(self.grammar)               # (the tables are uploaded once per automaton and kept by the loop)
            for b in range(len(self.rows)):
                self._set_grammar_state(b)
        elif loop.grammar is not None:
            loop.set_grammar(None)

    def _configure_logprobs(self) -> None:
        """The log-prob stage of this run, after every other mode is what the run wants (what _configure_sampling left on from an
        earlier run with the same top_n stays on)."""
        if self._logprobs is not None and self.loop.logprobs != self._logprobs:
            self.loop.drain()
            self.loop.set_logprobs(self._logprobs)

    def _resample_info(self, b: int):
        """The payload of a token the host redrew at another row of the step's logits (next to _resampler's draw)."""
        loop, top_n = self.loop, self._logprobs

        def resample_info(pos: int, tok: int):
            with torch.cuda.stream(loop.stream_t):
                return lpmod.redraw_payload(loop.step_logits[b, pos], tok, top_n)
        return resample_info

    def _set_grammar_state(self, b: int) -> None:
        """Row b's automaton state as the host sees the row: its own start state walked over what it has generated so far."""
        if self.grammar is not None:
            r, st = self.rows[b], self.grammar_starts[b]
            self.loop.set_grammar_state(b, self.grammar.walk(st, r.seq[r.n_prompt:]) if st >= 0 else -1)

    def _set_counts(self, b: int) -> None:
        """Row b's counts as the host sees the row: the prompt's ids, and what it has generated so far."""
        if self.processors is not None:
            r = self.rows[b]
            self.loop.set_logit_counts_row(b, r.seq[:r.n_prompt], r.seq[r.n_prompt:])

    def _resampler(self, b: int, row: _Row):
        """Draw at another position of the step's logits with the row's current Philox draw."""
        from specdec_hip.ops import sample_token_hip

        sp, loop = vars(self.options), self.loop       # (read by key: temperature, top_k, top_p, seed)
        if self.row_params is not None:    # the row's own parameters, as the step's kernels normalise them
            sp = self.row_params[b].scalars(vocab=self.pipe.base_lm.vocab_size)
        sid = self.row_ids[b]

        def resample(pos: int) -> int:
            with torch.cuda.stream(loop.stream_t):
                tok = sample_token_hip(loop.step_logits[b, pos], sp["temperature"], sp["top_k"], sp["top_p"], seed=sp["seed"],
                                       draw=row.draws, stream_ids=torch.tensor([sid], dtype=torch.int32, device="cuda"))
                return int(tok.item())
        return resample

    # ---- device-side repairs, applied only while the loop's stream is idle
    def _repair_rows(self) -> None:
        pipe, loop, rt = self.pipe, self.loop, self.rt
        for b, what in self._flagged.items():
            r = self.rows[b]
            fresh = b in self._fresh
            if fresh:                              # a new sequence in the slot: the old one's pages go back first (idle stream)
                for e in self._engines:
                    e.release(b)
                self._fresh.discard(b)
            if what == "resync" and r.active:      # a new sequence, or the host rules rewrote the row: rebuild its caches
                if fresh and self._held is not None:
                    pipe._absorb_row(rt, b, r.seq, self._held, self.stats)    # forked from a row the session holds, if one fits
                else:
                    for e in self._engines:
                        e.unshare(b)               # (pages shared with other rows are never written: the rebuild gets fresh ones)
                    if r.evicted:                  # a rolled row is rebuilt from the tokens its cache still holds, at their cache positions
                        pipe._prefill_row(rt, b, rolling.kept_tokens(r.seq, self.window.sinks, r.evicted))
                        r.rebuilds.append(len(r.seq) - r.n_prompt)
                    else:
                        pipe._prefill_row(rt, b, r.seq)
                    self.stats["prefilled_rows"] += 1 if fresh else 0
                loop.join_current_stream()
            if self.window is not None and r.active:
                self._roll(b, r)                   # (whatever flagged the row: its next launches must fit the window)
            pipe._set_row(loop, b, r)              # (re)position, or freeze a finished row
            if r.active:
                self._set_counts(b)                # (void steps counted tokens the row never kept: back to the in-order view)
                self._set_grammar_state(b)         # (and advanced its automaton over them)
            if self.per_row:                       # the device counted steps the host voided: hand it the in-order view
                m = self.row_ctl[b]
                loop.set_adaptive_row(b, m.current_k, r.strict_acc, r.strict_prop, m.acceptance_history[-4:])
        if self._flagged and ((self._spec and loop.spec_sampling) or (self._accept and self._sampled and loop.sampling)):
            loop.set_draw_counts([r.draws for r in self.rows])   # void steps drew for the flagged rows: back to the in-order view
        self._flagged.clear()

    def _roll(self, b: int, r: _Row) -> None:
        """The rolling context window, at the repair point (idle stream): when row b's next launches would not fit the window, the
        `drop` positions after the sinks leave both caches — evict_row on the loop's stream moves the survivors down and re-rotates
        their keys — and the row's cache length drops by as much. The caches hold the positions of seq[:-1] (the draft's `prev`
        hole among them: it moves with the rest and the next forward 0 refills it at its new position); what void steps wrote
        above them is stale and is overwritten. Token-counting state (processor counts, grammar state, log-prob payloads, draw
        counters) counts tokens, not positions: nothing to do."""
        w = self.window
        length = len(r.seq) - r.evicted
        drop = w.roll(length)
        if drop is None:
            return
        assert w.sinks + drop <= length - 1 <= w.size, (w, length)
        for e in self._engines:
            e.evict_row(b, w.sinks, drop, length - 1, stream=self.loop.stream_t)
        r.evicted += drop
        r.evictions.append((len(r.seq) - r.n_prompt, drop))
        self.stats["evictions"] += 1
        self.stats["evicted_positions"] += drop
        if self._held is not None:
            self._held[b] = None                   # a rolled row is no longer a source to fork from
        assert w.roll(len(r.seq) - r.evicted) is None

    def _recover(self, err: Exception) -> None:
        """A persistent launch of one of the models gave up (its bounded waits expired: the CUs were shared with another
        kernel). Every step since is void: drain the loop, clear the engines' health words and move them to the launch path
        (HipModel.recover), drop the captured step, rebuild every active row's caches from the host's sequences. Twice in one
        session: give up for real."""
        n = self.stats["engine_recoveries"] = self.stats.get("engine_recoveries", 0) + 1
        if n > 2:
            raise err
        self.pipe.logger.warning("decode session: %s — continuing on the launch path", err)
        self.loop.drain()
        self._queue.clear()
        for e in self._engines:
            e.recover(self.loop.stream_t)
        self.loop.invalidate()
        self.loop.captured_paths = None
        for b, r in enumerate(self.rows):
            self._flagged[b] = "resync" if r.active else "freeze"
            if self._held is not None and not r.active:
                self._held[b] = None      # a finished row is not rebuilt: its caches are no longer a source to fork from

    @property
    def _inflight(self) -> bool:
        return bool(self._queue)

    def _launch(self) -> None:
        """Only with an empty queue are repairs possible (idle stream); callers guarantee it when rows are flagged."""
        if self._flagged or self._resample_state:
            assert not self._queue
            self._repair_rows()
            if self._resample_state:
                self._resample_state = False
                self._configure_sampling()
        if not self._queue:
            paths = self._hint()
            was = self.loop.captured_paths
            if was is not None and was != paths:      # a model changed path (rows passed the persistent launch's context bound)
                self.loop.drain()
                self.loop.invalidate()
                self.stats["path_switches"] = self.stats.get("path_switches", 0) + 1
            self.loop.captured_paths = paths
        idx = self.loop.launches
        if self.window is not None:
            # the device advances every row in every launched step, void or not: what this launch and the ones in flight can address
            # on the longest row stays inside the cache rows (the window's slack: rolling.Window.room)
            assert self._reach() <= self.rt["l_max"], (self._reach(), self.rt["l_max"], self.window)
        if self._engines[0].page_len is not None:
            # paged KV: the device advances by itself, so every row gets the pages of all the steps in flight plus this one
            # before it is launched (table writes go to the loop's stream, ahead of the step). Frozen rows keep writing their
            # K+1 positions in place and keep their pages until the slot is handed on.
            reach = (len(self._queue) + 2) * (self.k + 1) + 2
            for b, r in enumerate(self.rows):
                for e in self._engines:
                    e.reserve(b, len(r.seq) + reach, stream=self.loop.stream_t)
        self.loop.step(use_graph=True)
        self._queue.append((idx, set()))

    def _can_launch_ahead(self) -> bool:
        """Conservative: some row cannot finish within the steps already launched, and nothing waits for a repair."""
        if self._flagged or self._resample_state:
            return False
        if self._hint() != self.loop.captured_paths:
            return False                   # a path switch is due: the queue drains first (_launch re-captures)
        ahead = len(self._queue) + 1       # steps whose records are still to come, counting the one being considered
        per_step = self.k + 1 if self.emit_mode == HipSpecDec.EMIT_BONUS else self.k
        for b, r in enumerate(self.rows):
            if not r.active:
                continue
            if len(r.generated) + ahead * per_step >= self.max_tokens:
                continue
            if self.step_limit is not None and r.steps + ahead + 1 > self.step_limit:
                continue
            if self.window is None and len(r.seq) + (ahead + 2) * self.k + 6 > self.pos_limit:
                continue                   # (a windowed row is flagged "roll" before it gets there, and no flagged row is launched ahead)
            return True
        return False

    def advance(self) -> bool:
        """One draft-then-verify step for every active row. Returns False when the controller
        stops the run."""
        pipe, rows, stats = self.pipe, self.rows, self.stats
        self.step += 1
        step = self.step
        if step > 1 and not self._early and not self.per_row:
            ctx = {"step": step, "generated_tokens": max(len(r.generated) for r in rows),
                   "acceptance_rate": stats["accepted"] / max(stats["proposed"], 1)}
            k_new = int(pipe.controller.get_k(step, ctx))
            if k_new <= 0:
                return False
            k_new = pipe._effective_k(k_new, self.self_draft)
            if k_new != self.k:  # adaptive K: another captured step over the same caches
                self.loop.sync()
                self._repair_rows()
                self.k = k_new
                self.rt, self.loop = pipe._runtime(len(rows), self.need, self.k, self.emit_mode, self.self_draft)
                self.loop.join_current_stream()
                for b, r in enumerate(rows):
                    pipe._set_row(self.loop, b, r)
                self._configure_loop()
                self._configure_logprobs()
        k, loop, rt = self.k, self.loop, self.rt
        t0 = time.time()
        if not self._queue:
            self._launch()              # (repairs flagged rows first: the stream is idle)
        while self._early and len(self._queue) < self._depth and self._can_launch_ahead():
            self._launch()              # keep the GPU's queue ahead of the host
        idx, void = self._queue.popleft()
        try:
            rec = loop.wait(idx) if self._queue else loop.sync()
        except EngineGaveUp as e:
            self._recover(e)
            return True                 # nothing was taken from the void steps; the rows rejoin at the next launch
        self.last_record = rec
        while self._early and len(self._queue) < self._depth and self._can_launch_ahead():
            self._launch()              # step s+1 (s+2) runs while the rules of step s are applied below
        stats["device_ms"] += (time.time() - t0) * 1e3
        widest = 0                  # confidence-gated draft length: the widest k among the rows this step counts for
        for b, r in enumerate(rows):
            if not r.active:
                continue
            if b in void:           # launched before the host repaired this row: nothing to take from it
                stats["void_row_steps"] += 1
                continue
            a = int(rec.accept_len[b])
            t = [int(x) for x in rec.target_ids[b]]
            d = [int(x) for x in rec.draft_tokens[b]]
            before, acc0 = r.seq, r.accepted
            if self.per_row:                    # the k that counted for this row in this step, from the device's controller
                k = int(rec.k_row[b])
                m = self.row_ctl[b]
                if k != m.current_k:
                    raise RuntimeError(f"row {b}: the device ran step {r.steps + 1} at k={k}, the host's controller says {m.current_k}")
                r.k_trace.append(k)
                r.strict_acc += a
                r.strict_prop += k
                m.get_k(r.steps + 2, {"step": r.steps + 2, "acceptance_rate": r.strict_acc / max(r.strict_prop, 1)})
            if self._conf:                      # the k the device's judgements left the row in this step: taken from the record, not mirrored
                k = int(rec.k_row[b])
                if not 1 <= k <= self.k:
                    raise RuntimeError(f"row {b}: the step record carries k={k} outside 1..{self.k}")
                r.k_trace.append(k)
                widest = max(widest, k)
            if self._spec or self._accept:
                # speculative sampling (and a device acceptance rule alike): the accepted tokens are the DRAFT's ids, then the redrawn / bonus token. An accepted EOS
                # ends the row by the rule as it stands for greedy steps: the accepted tokens are cut BEFORE the EOS, then the
                # rule appends t[pos] — a < k: pos = a, the token redrawn after the accepted prefix (the EOS itself is dropped);
                # a == k: pos = length of the cut, which is the EOS (it stays as the last token)
                t = [int(x) for x in rec.new_tokens[b]]
            elif self._sampled:
                t[a] = int(rec.new_tokens[b][a])       # the token the device sampled at position a
            assumed = before + t[: int(rec.n_new[b])]  # what the device advanced to
            if self.emit_mode == HipSpecDec.EMIT_BONUS:
                constrained = self.grammar is not None and self.grammar_starts[b] >= 0
                # logprobs: t[i] is new_tokens[b][i] for every i < n_new, and the rules read no other position
                info = lpmod.step_payload(rec, b, len(t)) if self._logprobs is not None else None
                pipe._rules_batch(r, k, a, t, self.max_tokens, self.grammar.eos_id if constrained else self.eos,
                                  self._resampler(b, r) if (self._sampled and not self._spec and not self._accept) else None,
                                  dedup=not constrained, info=info, resample_info=self._resample_info(b) if info is not None else None)
                if self._sampled:
                    r.draws += (k + 1) if self._spec else 1
            else:
                pipe._rules_single(r, k, a, d, t, self.max_tokens,
                                   self.grammar.eos_id if (self.grammar is not None and self.grammar_starts[b] >= 0) else self.eos)
            r.steps += 1
            r.counters.append((r.proposed, r.accepted, len(r.generated), a))
            if a >= k:
                stats["full_accepts"] = stats.get("full_accepts", 0) + 1
            stats["proposed"] += k
            stats["accepted"] += r.accepted - acc0
            if r.active and self.step_limit is not None and r.steps >= self.step_limit:
                r.active = False                # the reference's loop bound counts steps (pipeline.py:1984, :984)
            if self.window is None and r.active and len(r.seq) + 2 * self.k + 4 > self.pos_limit:
                r.active = False                # out of cache rows / model positions
            if not r.active:
                self._flagged[b] = "freeze"     # stop the row on the device
            elif r.seq != assumed:
                stats["resyncs"] += 1
                self._flagged[b] = "resync"
            elif self.window is not None and self.window.roll(len(r.seq) - r.evicted) is not None:
                self._flagged[b] = "roll"       # its next launches would not fit the window: evicted at the repair point (_roll)
            if b in self._flagged:
                for _, vs in self._queue:      # every step already launched is void for this row
                    vs.add(b)
        if widest:
            stats["draft_forwards_skipped"] = stats.get("draft_forwards_skipped", 0) + self.k - widest
        stats["steps"] = max(r.steps for r in rows)
        return True

    def admit(self, b: int, prompt: List[int], grammar_start: int = -1, params=None, index: Optional[int] = None) -> None:
        """Continuous batching: put a new sequence into the slot of a finished row. Its caches are prefilled
        and its device state set at the next launch point; the other rows keep stepping meanwhile. grammar_start: the new
        row's start state in the session's automaton (-1: unconstrained). params / index (a session with per-request
        parameters): the new request's SamplingParams (seed resolved) and its Philox stream id; the slot's table entry, stream
        id and draw counter are rewritten on the loop's stream, behind the steps in flight (which are void for the slot), and
        the captured step is kept."""
        if self.rows[b].active:
            raise ValueError(f"row {b} is still decoding")
        if not prompt:
            raise ValueError("empty prompt")
        if self.window is not None:         # the cache is sized by the window: the prompt must start without a roll, the budget does not count
            fits = self.window.fits(len(prompt))
        else:
            fits = not (len(prompt) + self.max_tokens + 2 * self.k + 8 > self.rt["l_max"] or len(prompt) + 2 * self.k + 4 > self.pos_limit)
        if not fits:
            raise ValueError(f"prompt of {len(prompt)} tokens does not fit this session (l_max {self.rt['l_max']}, positions {self.pos_limit})")
        if grammar_start >= 0 and self.grammar is None:
            raise ValueError("admit: the session was started without a grammar")
        if (params is not None) != (self.row_params is not None):
            raise ValueError("admit: the session was started without sampling_params" if params is not None else
                             "admit: the session decodes with per-request sampling parameters; pass the new request's")
        if params is not None and params.has_penalties and self.processors is None:
            raise ValueError("admit: the request has penalties but the session's logit-processor stage is off")
        self.rows[b] = _Row(list(prompt))
        self.grammar_starts[b] = int(grammar_start)
        self._fresh.add(b)
        if self._held is not None:
            self._held[b] = None          # the slot is reused: what its caches hold is no longer on record
        if self.per_row:
            self.row_ctl[b] = self._new_row_controller()
        self._flagged[b] = "resync"
        for _, vs in self._queue:
            vs.add(b)
        if params is not None:
            self.row_params[b] = params = params.with_seed(self.options.seed)
            self.row_ids[b] = b if index is None else int(index)
            self.loop.set_row_params(b, params, stream_id=self.row_ids[b], draw_count=0)
        elif self._sampled:
            self._resample_state = True   # draw counters restart for the new row at the next launch point

    def finish(self) -> None:
        """Drain a step launched ahead of a run that ended, and leave the device rows consistent."""
        if self._queue:
            self.loop.sync()
            self._queue.clear()
        self._repair_rows()
