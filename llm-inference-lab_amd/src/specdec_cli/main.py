"""`python -m src.specdec_cli.main {bench,run}` — counterpart of the reference's `specdec` console script
(src/specdec_cli/main.py:1-102): `bench` runs the K-sweep harness and writes its CSV + JSON, `run` decodes one prompt
through `SpeculativePipeline.generate` and prints the device / dtype / kernel backends and the text.

Same sub-commands and options; what differs is forced by this build: the device is always `cuda` (PyTorch-ROCm's name for
the MI355X), models are local checkpoint directories or `synthetic:<preset>` (nothing is fetched by name, so the defaults
are the synthetic Llama-3.2 pair instead of gpt2 / distilgpt2), `--k` is actually applied (the reference passes it as
max_draft, which its controller ignores), and `run --do-sample` is refused by generate() as documented there."""

from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

from kernels import get_kernel_info
from specdec import SpeculativePipeline


def _harness():
    scripts = Path(__file__).resolve().parent.parent.parent / "scripts"
    if str(scripts) not in sys.path:
        sys.path.insert(0, str(scripts))
    import k_sweep  # noqa: E402  (llm-inference-lab_amd/scripts/k_sweep.py)

    return k_sweep


def cmd_bench(args: argparse.Namespace) -> int:
    H = _harness()
    ns = argparse.Namespace(base_model=args.base_model, draft_model=args.draft_model, max_tokens=args.max_tokens,
                            iterations=args.iterations, max_k=args.max_k, batch_size=int(os.getenv("SPECDEC_BATCH_SIZE", "1")),
                            share_draft_embeddings=args.draft_model.startswith("synthetic:"), flip=args.flip, continuous=False,
                            do_sample=False)
    if args.deterministic:
        os.environ["SPECDEC_DETERMINISTIC"] = "1"
    results, detailed = H.run(ns)
    csv_file, json_file = H.save(results, detailed, args.output_dir, ns.batch_size)
    print(f"Results saved to {csv_file} and {json_file}")
    return 0


def cli_sampling_params(args: argparse.Namespace):
    """The entries of `run --sampling-params` (None without it); ValueError where another option carries the same parameter."""
    from specdec_hip.sampling_params import load_for_cli

    return load_for_cli(args.sampling_params, 1, {
        "--do-sample": args.do_sample, "--repetition-penalty": args.repetition_penalty, "--presence-penalty": args.presence_penalty,
        "--frequency-penalty": args.frequency_penalty, "--spec-top-k": args.spec_top_k, "--spec-top-p": args.spec_top_p})


def cmd_run(args: argparse.Namespace) -> int:
    try:
        row_params = cli_sampling_params(args)
    except (OSError, ValueError, TypeError) as e:
        raise SystemExit(f"--sampling-params: {e}")
    spec = getattr(args, "spec_sampling", False)
    extra = {"policy": "rejection", "policy_params": {"backend": "device", "temperature": args.temperature, "seed": args.seed}} if spec else {}
    shape = {k: v for k, v in (("top_k", args.spec_top_k), ("top_p", args.spec_top_p)) if v is not None}
    if shape and not spec:
        raise SystemExit("--spec-top-k / --spec-top-p belong to --spec-sampling")
    if spec:
        extra["policy_params"].update(shape)
    lossy = args.policy != "longest_prefix"
    if lossy:    # typical / topk_agree inside the captured step (the device backend)
        from specdec.run_specdec import device_policy_params

        if spec:
            raise SystemExit("--policy and --spec-sampling cannot be given together")
        try:
            pp = device_policy_params(args)
        except ValueError as e:
            raise SystemExit(str(e))
        if not pp:
            raise SystemExit(f"--policy {args.policy} needs --policy-backend device here (the host loop is run_specdec's)")
        if args.policy == "topk_agree" and args.policy_k is not None:
            pp["k"] = args.policy_k
        extra = {"policy": args.policy, "policy_params": pp}
    pipe = SpeculativePipeline(base_model=args.base_model, draft_model=args.draft_model, max_draft=args.k, implementation="hip",
                               device=args.device, controller="fixed", controller_params={"k": args.k}, enable_optimization=True,
                               draft_mode="vanilla", **extra)
    proc = {k: v for k, v in (("repetition_penalty", args.repetition_penalty), ("presence_penalty", args.presence_penalty),
                              ("frequency_penalty", args.frequency_penalty), ("bad_token_ids", args.ban_token)) if v is not None}
    if args.regex is not None:
        proc["grammar"] = pipe.grammar_from_regex(args.regex)
    if row_params is not None:
        proc["sampling_params"] = row_params
    conf = args.draft_confidence is not None
    if args.draft_min_k is not None and not conf:
        raise SystemExit("--draft-min-k belongs to --draft-confidence")
    if conf:     # confidence-gated draft length inside the captured step (a generate_batch mode)
        proc.update(draft_confidence=args.draft_confidence, draft_min_k=args.draft_min_k)
    lp = args.logprobs is not None or args.best_of is not None
    if lp:       # per-token log-probs inside the captured step; best_of ranks the rows by their sum (generate_batch)
        proc.update(logprobs=args.logprobs, best_of=args.best_of)
        if args.do_sample:
            proc.update(do_sample=True, temperature=args.temperature, seed=args.seed)
    roll = args.context_window is not None
    if args.attention_sinks is not None and not roll:
        raise SystemExit("--attention-sinks belongs to --context-window")
    if roll:     # the rolling context window (a generate_batch mode): caches sized by the window, rows roll at the repair point
        proc.update(context_window=args.context_window, attention_sinks=args.attention_sinks)
    if roll or lp or conf or spec or lossy or args.share_prefix or args.n != 1 or row_params is not None:  # generate_batch modes (speculative sampling inside the captured step; --n rows of the prompt)
        rs = pipe.generate_batch([args.prompt], max_tokens=args.max_tokens, share_prefix=args.share_prefix, n=args.n, **proc)
        res = {**pipe._sysinfo(), **rs[0]}
        for i, x in enumerate(rs[1:], 1):
            print(f"Text {i}: {x.get('text', '')}")
        if lp:
            import json

            fields = ("generated_tokens", "logprobs", "token_ranks", "top_logprobs", "cumulative_logprob")
            print("Logprobs: " + json.dumps([{k: x[k] for k in fields if k in x} for x in rs]))
        if roll:
            print(f"Evictions (tokens generated before the roll, positions dropped): {[list(e) for e in rs[0]['evictions']]}")
    else:
        res = pipe.generate(prompt=args.prompt, max_tokens=args.max_tokens, temperature=args.temperature, do_sample=args.do_sample, **proc)
    kinfo = get_kernel_info()
    print(f"Device: {res.get('device')} | Dtype: {res.get('dtype')} | "
          f"Backends: verify={kinfo.get('verify_backend')}, kv_append={kinfo.get('kv_append_backend')}")
    print(f"Text: {res.get('text', '')}")
    return 0


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(prog="specdec", description="MI355X speculative-decoding CLI")
    sub = p.add_subparsers(dest="cmd", required=True)
    pb = sub.add_parser("bench", help="Run a K-sweep benchmark")
    pb.add_argument("--base-model", default="synthetic:llama-3.2-3b")
    pb.add_argument("--draft-model", default="synthetic:llama-3.2-1b")
    pb.add_argument("--max-tokens", type=int, default=32)
    pb.add_argument("--iterations", type=int, default=10)
    pb.add_argument("--max-k", type=int, default=4)
    pb.add_argument("--flip", type=float, default=0.2, help="synthetic pairs: fraction of tokens whose draft successor differs")
    pb.add_argument("--device", choices=["auto", "cuda"], default="auto")
    pb.add_argument("--output-dir", type=Path, default=Path("results"))
    pb.add_argument("--deterministic", action="store_true")
    pb.set_defaults(func=cmd_bench)
    pr = sub.add_parser("run", help="Run a single prompt via SpeculativePipeline")
    pr.add_argument("--base-model", default="synthetic:llama-3.2-3b")
    pr.add_argument("--draft-model", default="synthetic:llama-3.2-1b")
    pr.add_argument("--k", type=int, default=2)
    pr.add_argument("--max-tokens", type=int, default=32)
    pr.add_argument("--device", choices=["auto", "cuda"], default="auto")
    pr.add_argument("--temperature", type=float, default=0.7)
    pr.add_argument("--do-sample", action="store_true")
    pr.add_argument("--spec-sampling", action="store_true",
                    help="speculative sampling on the device (policy 'rejection', backend 'device') at --temperature, drawn with --seed")
    pr.add_argument("--spec-top-k", type=int, help="--spec-sampling: keep the top_k (1..1024) largest logits of both distributions")
    pr.add_argument("--spec-top-p", type=float, help="--spec-sampling: nucleus cut inside --spec-top-k (needs it)")
    pr.add_argument("--policy", choices=["longest_prefix", "typical", "topk_agree"], default="longest_prefix",
                    help="acceptance rule of the captured step; typical / topk_agree need --policy-backend device")
    pr.add_argument("--policy-backend", choices=["host", "device"], default="host",
                    help="'device': the rule runs inside the captured step on the verify pass's rows (the target after the draft tokens)")
    pr.add_argument("--policy-k", type=int, help="--policy topk_agree: accept a draft token among the target's k largest logits")
    pr.add_argument("--typical-epsilon", type=float, help="--policy typical: the threshold epsilon")
    pr.add_argument("--typical-delta", type=float, help="--policy typical: accept p(d) >= min(epsilon, delta * exp(-H)); without it epsilon alone")
    pr.add_argument("--seed", type=int, default=0)
    pr.add_argument("--draft-confidence", type=float, metavar="TAU",
                    help="stop drafting a row once the draft's probability of its own token falls below TAU in (0, 1], decided on the "
                         "device between two draft forwards of the captured step (generate_batch)")
    pr.add_argument("--draft-min-k", type=int, metavar="N", help="--draft-confidence: always draft at least N tokens (default 1)")
    pr.add_argument("--logprobs", type=int, metavar="N",
                    help="per-token log-probs of the generated tokens, computed inside the captured step: 0 = the chosen token's, "
                         "1..20 = that many alternatives as well; printed as one JSON line (generate_batch)")
    pr.add_argument("--best-of", type=int, metavar="M",
                    help="decode M >= --n rows and keep the --n with the highest cumulative log-prob, best first (implies --logprobs 0; "
                         "needs --do-sample, --spec-sampling or --sampling-params)")
    pr.add_argument("--context-window", type=int, metavar="W",
                    help="rolling context window: a row's cache keeps --attention-sinks first positions and the most recent ones, never "
                         "more than W; the caches are sized by W, not by --max-tokens (generate_batch)")
    pr.add_argument("--attention-sinks", type=int, metavar="S", help="--context-window: positions kept at the start of the cache (default 4)")
    pr.add_argument("--repetition-penalty", type=float, help="repetition penalty (> 0) over prompt + generated tokens, inside the captured step")
    pr.add_argument("--presence-penalty", type=float, help="subtracted from the logit of every token generated so far")
    pr.add_argument("--frequency-penalty", type=float, help="subtracted from the logit of a token once per time it was generated")
    pr.add_argument("--ban-token", type=int, action="append", metavar="ID", help="never emit this token id (repeatable)")
    pr.add_argument("--regex", type=str, metavar="PATTERN", help="constrain the output to full matches of this regular expression over the "
                                                                 "tokens' bytes (a token automaton inside the captured step)")
    pr.add_argument("--sampling-params", type=str, metavar="FILE",
                    help="JSON list with one object per prompt (temperature, top_k, top_p, seed, repetition_penalty, presence_penalty, "
                         "frequency_penalty): per-request parameters read row by row inside the captured step (generate_batch)")
    pr.add_argument("--n", type=int, default=1, help="n completions of the prompt: n rows of one generate_batch call, the prompt prefilled "
                                                     "once and forked into the others (implies --share-prefix)")
    pr.add_argument("--share-prefix", action="store_true", help="decode through generate_batch with share_prefix=True")
    pr.add_argument("prompt", type=str)
    pr.set_defaults(func=cmd_run)
    return p


def main(argv=None) -> None:
    args = build_parser().parse_args(argv)
    raise SystemExit(args.func(args))


if __name__ == "__main__":
    main()
