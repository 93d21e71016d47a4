"""`python -m src.specdec.run_specdec` — command line over SpeculativePipeline.generate.

Counterpart of the reference CLI (src/specdec/run_specdec.py:40-283): same options and the same one-line JSON
on stdout (latency_ms, proposed, accepted, acceptance_rate, tokens_per_sec, text, impl, device, base_model,
draft_model, draft_mode, dtype). Differences forced by this build: `--impl` is `hip` (the reference's
`fake`/`hf` have no counterpart: there is no CPU path), models are local checkpoint directories or
`synthetic:<preset>` (nothing is fetched by name), and with synthetic weights the prompt is a list of token
ids ("12 7 99"). Decoding is greedy (`generate(do_sample=True)` is refused, see pipeline.py)."""

from __future__ import annotations

import argparse
import json
import logging
import math
import sys

from .core.pipeline import SpeculativePipeline


def parse_args(argv=None) -> argparse.Namespace:
    ap = argparse.ArgumentParser(description="Speculative decoding on MI355X (HIP path)")
    ap.add_argument("--prompt", type=str, required=True, help="prompt text (token ids for synthetic models)")
    ap.add_argument("--max-tokens", type=int)
    ap.add_argument("--config", type=str, help="YAML configuration (configs/specdec.yaml keys)")
    ap.add_argument("--verbose", action="store_true")
    ap.add_argument("--base-model", type=str, help="checkpoint directory or synthetic:<preset>")
    ap.add_argument("--draft-model", type=str)
    ap.add_argument("--max-draft", type=int)
    ap.add_argument("--temperature", type=float)
    ap.add_argument("--seed", type=int)
    ap.add_argument("--device", type=str, choices=["auto", "cuda"], default="auto")
    ap.add_argument("--impl", type=str, choices=["hip"], default="hip")
    ap.add_argument("--draft-mode", type=str, choices=["vanilla", "medusa", "eagle"], default="vanilla")
    ap.add_argument("--policy", type=str, choices=["longest_prefix", "conf_threshold", "topk_agree", "typical"], default="longest_prefix")
    ap.add_argument("--policy-tau", type=float, help="conf_threshold: tau")
    ap.add_argument("--policy-k", type=int, help="topk_agree: k")
    ap.add_argument("--policy-p", type=float, help="typical: p")
    ap.add_argument("--policy-backend", type=str, choices=["host", "device"], default="host",
                    help="typical / topk_agree: 'device' runs the rule inside the captured step on the verify pass's rows (the target's "
                         "distribution after the draft tokens; decodes through generate_batch); 'host' is the reference's loop, which "
                         "scores the draft against the target's own continuation")
    ap.add_argument("--typical-epsilon", type=float, help="--policy typical --policy-backend device: the threshold epsilon (same as --policy-p)")
    ap.add_argument("--typical-delta", type=float, help="--policy typical --policy-backend device: accept p(d) >= min(epsilon, delta * exp(-H)); "
                                                        "without it the threshold is epsilon alone")
    ap.add_argument("--spec-sampling", action="store_true",
                    help="speculative sampling inside the captured step (policy 'rejection', backend 'device'): the output is "
                         "distributed as the target's own sampling at --temperature; drawn with --seed; fixed K, draft-model mode")
    ap.add_argument("--spec-top-k", type=int, help="--spec-sampling: keep the top_k (1..1024) largest logits of both distributions")
    ap.add_argument("--spec-top-p", type=float, help="--spec-sampling: nucleus cut inside --spec-top-k (needs it)")
    ap.add_argument("--controller", type=str, choices=["fixed", "adaptive"], default="fixed")
    ap.add_argument("--K", type=int, default=4, help="K of the fixed controller")
    ap.add_argument("--adaptive-K", action="store_true")
    ap.add_argument("--min-k", type=int)
    ap.add_argument("--max-k", type=int)
    ap.add_argument("--target-acceptance", type=float)
    ap.add_argument("--per-row-K", action="store_true",
                    help="adaptive controller: every batch row its own K, moved on the device inside the captured step (not in the reference)")
    ap.add_argument("--draft-confidence", type=float, metavar="TAU",
                    help="stop drafting a row once the draft's probability of its own token falls below TAU in (0, 1]: decided on the "
                         "device between two draft forwards of the captured step; fixed K, draft-model mode; decodes through generate_batch")
    ap.add_argument("--draft-min-k", type=int, metavar="N", help="--draft-confidence: always draft at least N tokens (default 1)")
    ap.add_argument("--prefill-backend", type=str, choices=["auto", "passes", "rocblas", "native"], default="auto",
                    help="how prompts are absorbed into the KV cache: auto (rocBLAS where it serves the model, else the 128-token passes), "
                         "passes, rocblas, or native (this library's MFMA GEMM over the packed weights; bf16 and fp8, dense and paged KV)")
    ap.add_argument("--n", type=int, default=1,
                    help="n completions of the prompt as n rows of one generate_batch call: the prompt is prefilled once and the other "
                         "rows are forked from it (implies --share-prefix); they differ under --spec-sampling (a Philox stream per row)")
    ap.add_argument("--share-prefix", action="store_true",
                    help="decode through generate_batch with share_prefix=True (rows pay for an equal prompt or a common prefix once)")
    ap.add_argument("--repetition-penalty", type=float, help="divide (multiply, when negative) the logits of tokens in the prompt or "
                                                              "generated so far by this (> 0; inside the captured step)")
    ap.add_argument("--presence-penalty", type=float, help="subtracted from the logit of every token generated so far")
    ap.add_argument("--frequency-penalty", type=float, help="subtracted from the logit of a token once per time it was generated")
    ap.add_argument("--ban-token", type=int, action="append", metavar="ID", help="never emit this token id (repeatable)")
    ap.add_argument("--regex", type=str, metavar="PATTERN",
                    help="constrain the output to full matches of this regular expression over the tokens' bytes: a token automaton "
                         "masks draft and target logits inside the captured step (literals, classes, groups, |, * + ? {m,n})")
    ap.add_argument("--sampling-params", type=str, metavar="FILE",
                    help="JSON list with one object per prompt (temperature, top_k, top_p, seed, repetition_penalty, presence_penalty, "
                         "frequency_penalty): per-request parameters read row by row inside the captured step; temperature 0 is a "
                         "greedy request; with --n every completion shares its prompt's entry; decodes through generate_batch "
                         "(sampled bonus token, or speculative sampling with --spec-sampling)")
    ap.add_argument("--logprobs", type=int, metavar="N",
                    help="per-token log-probs of the generated tokens under the target, computed inside the captured step from the row "
                         "each token was checked against or drawn from: 0 = the chosen token's log-prob and rank, 1..20 = that many "
                         "alternatives as well; adds logprobs, token_ranks, top_logprobs, cumulative_logprob; decodes through generate_batch")
    ap.add_argument("--best-of", type=int, metavar="M",
                    help="decode M >= --n rows of the prompt and return the --n with the highest cumulative log-prob, best first "
                         "(implies --logprobs 0; needs a sampling mode: --spec-sampling or --sampling-params)")
    ap.add_argument("--context-window", type=int, metavar="W",
                    help="rolling context window: a row's cache keeps --attention-sinks first positions and the most recent ones, never "
                         "more than W; the caches are sized by W, not by --max-tokens, and the middle is evicted (keys re-rotated on the "
                         "device) whenever the next steps would not fit; adds evictions; decodes through generate_batch")
    ap.add_argument("--attention-sinks", type=int, metavar="S", help="--context-window: positions kept at the start of the cache (default 4)")
    ap.add_argument("--eval-perplexity", action="store_true",
                    help="add perplexity / perplexity_loss of the generated tokens under the target model (scored on the device)")
    ap.add_argument("--eval-agreement", action="store_true",
                    help="add the draft's agreement with the target on prompt + generated tokens (acceptance probability at "
                         "--temperature, KL, greedy agreement, expected tokens per step for K = 1..8; reduced on the device)")
    return ap.parse_args(argv)


def cli_sampling_params(args: argparse.Namespace):
    """The entries of --sampling-params (None without it); ValueError where another option carries the same parameter or
    selects a mode the entries are not read in."""
    from specdec_hip.sampling_params import load_for_cli

    return load_for_cli(args.sampling_params, 1, {
        "--repetition-penalty": args.repetition_penalty, "--presence-penalty": args.presence_penalty,
        "--frequency-penalty": args.frequency_penalty, "--spec-top-k": args.spec_top_k, "--spec-top-p": args.spec_top_p,
        "--adaptive-K": args.adaptive_K, "--controller adaptive": args.controller == "adaptive", "--per-row-K": args.per_row_K,
        "--draft-mode " + args.draft_mode: args.draft_mode != "vanilla",
        "--policy " + args.policy: args.policy != "longest_prefix"})


def device_policy_params(args: argparse.Namespace) -> dict:
    """The policy_params --policy-backend / --typical-epsilon / --typical-delta add ({} on the host backend); ValueError where they
    are given without the device backend or with a policy that has none."""
    device = getattr(args, "policy_backend", "host") == "device"
    eps, delta = getattr(args, "typical_epsilon", None), getattr(args, "typical_delta", None)
    if not device:
        if eps is not None or delta is not None:
            raise ValueError("--typical-epsilon / --typical-delta belong to --policy typical --policy-backend device")
        return {}
    if args.policy not in ("typical", "topk_agree"):
        raise ValueError(f"--policy-backend device belongs to --policy typical / topk_agree (speculative sampling is --spec-sampling), not {args.policy}")
    if args.policy != "typical" and (eps is not None or delta is not None):
        raise ValueError("--typical-epsilon / --typical-delta belong to --policy typical")
    out = {"backend": "device"}
    if args.policy == "typical":
        out.update({k: v for k, v in (("p", eps), ("delta", delta)) if v is not None})
        if getattr(args, "temperature", None) is not None:
            out["temperature"] = args.temperature
    return out


def generated_perplexity(lm, tokens):
    """(perplexity, loss) of the generated ids under `lm` (HipLM.score); (inf, inf) for fewer than 2 tokens, as the reference's
    evaluator reports a text it cannot score."""
    ids = [int(t) for t in tokens]
    if len(ids) < 2:
        return float("inf"), float("inf")
    logprob, _ = lm.score(ids)
    loss = -float(logprob.double().mean())
    return math.exp(loss), loss


def sequence_agreement(pipe, tokens, temperature=None):
    """The summary keys of SpeculativePipeline.draft_agreement over `tokens` (agreement_alpha, agreement_kl, agreement_greedy,
    expected_tokens_per_step); None each for fewer than 2 tokens."""
    ids = [int(t) for t in tokens]
    if len(ids) < 2:
        return {"agreement_alpha": None, "agreement_kl": None, "agreement_greedy": None, "expected_tokens_per_step": None}
    r = pipe.draft_agreement(ids, temperature=1.0 if temperature is None else temperature)
    return {"agreement_alpha": r["mean_alpha"], "agreement_kl": r["mean_kl"], "agreement_greedy": r["greedy_agreement"],
            "expected_tokens_per_step": r["expected_tokens_per_step"]}


def main(argv=None) -> int:
    args = parse_args(argv)
    logging.basicConfig(level=logging.DEBUG if args.verbose else logging.WARNING, stream=sys.stderr)
    raw = list(argv) if argv is not None else sys.argv[1:]
    if any(a == "--K" or a.startswith("--K=") for a in raw) and args.adaptive_K:
        logging.error("Cannot specify both --K and --adaptive-K")
        return 1
    try:
        row_params = cli_sampling_params(args)
    except (OSError, ValueError, TypeError) as e:
        logging.error("Error: %s", e)
        return 1
    if args.adaptive_K or args.controller == "adaptive":
        controller, cp = "adaptive", {k: v for k, v in (("min_k", args.min_k), ("max_k", args.max_k),
                                                       ("target_acceptance_rate", args.target_acceptance)) if v is not None}
        if args.per_row_K:
            cp["per_row"] = True
            # the device controller requires min_k <= initial_k <= max_k (sd_specdec_set_adaptive): clamp the default of 4
            lo = args.min_k if args.min_k is not None else 1
            hi = args.max_k if args.max_k is not None else max(4, lo)
            cp["initial_k"] = max(lo, min(4, hi))
    else:
        controller, cp = "fixed", {"k": args.K}
    policy, pp = args.policy, {k: v for k, v in (("tau", args.policy_tau), ("k", args.policy_k), ("p", args.policy_p)) if v is not None}
    try:
        pp.update(device_policy_params(args))
    except ValueError as e:
        logging.error("Error: %s", e)
        return 1
    if args.spec_sampling:
        if args.policy != "longest_prefix":
            logging.error("Cannot specify both --policy and --spec-sampling")
            return 1
        policy, pp = "rejection", {"backend": "device", "temperature": 0.7 if args.temperature is None else args.temperature,
                               "seed": 0 if args.seed is None else args.seed}   # (the pipeline refuses a temperature <= 0)
        pp.update({k: v for k, v in (("top_k", args.spec_top_k), ("top_p", args.spec_top_p)) if v is not None})
    elif args.spec_top_k is not None or args.spec_top_p is not None:
        logging.error("--spec-top-k / --spec-top-p belong to --spec-sampling")
        return 1
    if args.draft_min_k is not None and args.draft_confidence is None:
        logging.error("--draft-min-k belongs to --draft-confidence")
        return 1
    if args.attention_sinks is not None and args.context_window is None:
        logging.error("--attention-sinks belongs to --context-window")
        return 1
    try:
        pipe = SpeculativePipeline(config_path=args.config, base_model=args.base_model, draft_model=args.draft_model,
                                   max_draft=args.max_draft, device=args.device, seed=args.seed, implementation=args.impl,
                                   policy=policy, controller=controller, controller_params=cp, draft_mode=args.draft_mode,
                                   policy_params=pp)
        for lm in (pipe.base_lm, pipe.draft_lm):
            if lm is not None and hasattr(lm, "prefill_backend"):
                lm.prefill_backend = args.prefill_backend    # read when the pipeline creates its engines (first generate)
        conf = args.draft_confidence is not None
        lp = args.logprobs is not None or args.best_of is not None
        roll = args.context_window is not None
        batch = (roll or lp or conf or args.spec_sampling or args.share_prefix or args.n != 1 or row_params is not None
                 or pp.get("backend") == "device")
        proc = {k: v for k, v in (("repetition_penalty", args.repetition_penalty), ("presence_penalty", args.presence_penalty),
                                  ("frequency_penalty", args.frequency_penalty), ("bad_token_ids", args.ban_token)) if v is not None}
        if args.regex is not None:
            proc["grammar"] = pipe.grammar_from_regex(args.regex)
        if row_params is not None:
            proc["sampling_params"] = row_params
        if conf:       # confidence-gated draft length inside the captured step
            proc.update(draft_confidence=args.draft_confidence, draft_min_k=args.draft_min_k)
        if lp:         # per-token log-probs inside the captured step; best_of ranks the rows by their sum
            proc.update(logprobs=args.logprobs, best_of=args.best_of)
        if roll:       # the rolling context window: the caches are sized by it, rows roll at the session's repair point
            proc.update(context_window=args.context_window, attention_sinks=args.attention_sinks)
        if batch:      # generate_batch modes (a correction / bonus token every step): a batch of the prompt's --n rows
            rs = pipe.generate_batch([args.prompt], max_tokens=args.max_tokens, share_prefix=args.share_prefix, n=args.n, **proc)
            r = {**pipe._sysinfo(), **rs[0], "latency_ms": rs[0]["total_time_ms"],
                 "acceptance_rate": rs[0]["accepted"] / max(rs[0]["proposed"], 1), "n": len(rs), "texts": [x["text"] for x in rs],
                 "forked_rows": rs[0]["batch_metrics"]["forked_rows"], "shared_positions": rs[0]["batch_metrics"]["shared_positions"],
                 "cumulative_logprobs": [x.get("cumulative_logprob") for x in rs]}
        else:
            r = pipe.generate(prompt=args.prompt, max_tokens=args.max_tokens, temperature=args.temperature, do_sample=False, **proc)
        if args.eval_perplexity:
            r["perplexity"], r["perplexity_loss"] = generated_perplexity(pipe.base_lm, r["generated_tokens"])
        if args.eval_agreement:
            r.update(sequence_agreement(pipe, pipe._encode(args.prompt) + [int(t) for t in r["generated_tokens"]], args.temperature))
    except Exception as e:  # the reference CLI reports and exits 1 (run_specdec.py:276-278)
        logging.error("Error: %s", e)
        return 1
    keys = ("latency_ms", "proposed", "accepted", "acceptance_rate", "tokens_per_sec", "text", "impl", "device",
            "base_model", "draft_model", "draft_mode", "dtype")
    if args.share_prefix or args.n != 1:
        keys += ("n", "texts", "forked_rows", "shared_positions")
    if args.logprobs is not None or args.best_of is not None:
        keys += ("generated_tokens", "logprobs", "token_ranks", "cumulative_logprob", "cumulative_logprobs")
        keys += ("top_logprobs",) if (args.logprobs or 0) > 0 else ()
    if args.context_window is not None:
        keys += ("evictions",)
    if args.eval_perplexity:
        keys += ("perplexity", "perplexity_loss")
    if args.eval_agreement:
        keys += ("agreement_alpha", "agreement_kl", "agreement_greedy", "expected_tokens_per_step")
    print(json.dumps({k: r[k] for k in keys}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
