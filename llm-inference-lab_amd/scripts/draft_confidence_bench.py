"""ms per step of the captured step with the confidence-gated draft length (sd_specdec_set_draft_confidence) against the same step
without it, on one pair and the same prompts (profiles/draft_confidence.md).

    python llm-inference-lab_amd/scripts/draft_confidence_bench.py [--target llama-3.2-3b --draft llama-3.2-1b --steps 60 --warmup 10]
                                                                   [--shapes 4x1,4x8,8x1,8x8] [--out profiles/draft_confidence.md]

Per shape (K x rows), three legs of one run, one JSON line each:
    off          the mode never set: the yardstick (launch for launch the step as it is without the feature)
    never_stops  tau = 1e-6: every row drafts K tokens; what is added is the stored rows of the judged forwards and the judgement launches
    stops_at_1   tau = 1 with min_k = 1: every row stops after forward 0, so forwards 1..K-1 return at entry (their residual cost) and the
                 verify forward still scores K + 1 positions
The synthetic draft is all but one-hot (its confidence is exactly 1, which tau = 1 lets through), so its final norm weight is scaled by
--soft (default 4 / d_model: the token still leads by ~4 logits, the largest confidence stays below 1) in ALL legs; a launch's cost does
not depend on the values. The largest confidence seen is printed with the never_stops leg. No claim about accepted tokens per second is
made from this pair: its confidences are not tied to its engineered acceptance.
The judgement kernel's own time: run this script under `rocprofv3 --kernel-trace --stats` and read confidence_judge_kernel."""

import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(ROOT)]

import torch  # noqa: E402

LEGS = (("off", None), ("never_stops", 1e-6), ("stops_at_1", 1.0))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default="llama-3.2-3b")
    ap.add_argument("--draft", default="llama-3.2-1b")
    ap.add_argument("--shapes", default="4x1,4x8,8x1,8x8", help="K x rows, comma separated")
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--flip", type=float, default=0.2)
    ap.add_argument("--soft", type=float, default=None)
    ap.add_argument("--out", default=None, help="write the table as markdown here")
    args = ap.parse_args()
    from specdec_hip import weights as W
    from specdec_hip.engine import HipSpecDec
    from src.specdec import HipLM, SpeculativePipeline

    presets = {"llama-3.2-1b": W.LLAMA_3_2_1B, "llama-3.2-3b": W.LLAMA_3_2_3B, "llama-3-8b": W.LLAMA_3_8B}
    tgt = W.synthetic_llama(presets[args.target], seed=0, device="cuda")
    drf = W.synthetic_llama(presets[args.draft], seed=1, device="cuda", embed_from=tgt, flip_fraction=args.flip)
    soft = args.soft if args.soft else 4.0 / drf.config.d_model
    drf.final_norm_w = (drf.final_norm_w.float() * soft).to(drf.final_norm_w.dtype)
    base, draft = HipLM(tgt), HipLM(drf)
    V = tgt.config.vocab
    total = args.warmup + args.steps
    rows_out = []
    for shape in args.shapes.split(","):
        k, batch = (int(x) for x in shape.split("x"))
        prompts = [torch.randint(4, V, (32,), generator=torch.Generator().manual_seed(1234 + i), dtype=torch.int64).tolist() for i in range(batch)]
        for name, tau in LEGS:
            pipe = SpeculativePipeline(base_lm=base, draft_lm=draft, draft_model="none", controller="fixed", controller_params={"k": k}, seed=1234)
            kw = {} if tau is None else {"draft_confidence": tau}
            sess = pipe.start_session(prompts, max_tokens=total * (k + 1) + 1, emit_mode=HipSpecDec.EMIT_BONUS, **kw)
            c_max = 0.0
            for _ in range(args.warmup):
                sess.advance()
                if tau is not None:
                    c = sess.loop.draft_conf
                    c_max = max(c_max, float(torch.nan_to_num(c, nan=0.0).max()))
            n0, p0 = sum(len(r.generated) for r in sess.rows), sess.stats["proposed"]
            gc.collect()
            gc.disable()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.steps):
                sess.advance()
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            gc.enable()
            nodes = sess.loop.graph_nodes
            sess.finish()
            n = sum(len(r.generated) for r in sess.rows) - n0
            rec = {"leg": name, "k": k, "batch": batch, "ms_per_step": round(1e3 * dt / args.steps, 4), "graph_nodes": nodes,
                   "mean_k": round((sess.stats["proposed"] - p0) / args.steps / batch, 3), "tokens_per_step_per_row": round(n / args.steps / batch, 3),
                   "resyncs": sess.stats["resyncs"], "largest_confidence": round(c_max, 6) if tau is not None else None, "soft": soft}
            print(json.dumps(rec), flush=True)
            rows_out.append(rec)
            del sess, pipe
    if args.out:
        with open(args.out, "w") as f:
            f.write("| K | rows | leg | ms/step | vs off | graph nodes | mean k | tokens/step/row | largest confidence |\n|---|---|---|---|---|---|---|---|---|\n")
            for r in rows_out:
                off = next(x for x in rows_out if (x["k"], x["batch"], x["leg"]) == (r["k"], r["batch"], "off"))
                tau = dict(LEGS)[r["leg"]]
                leg = r["leg"] if tau is None else f"{r['leg']} (tau {tau:g})"
                conf = "-" if r["largest_confidence"] is None else f"{r['largest_confidence']:.6f}"
                f.write(f"| {r['k']} | {r['batch']} | {leg} | {r['ms_per_step']:.4f} | {r['ms_per_step'] - off['ms_per_step']:+.4f} | {r['graph_nodes']} | "
                        f"{r['mean_k']} | {r['tokens_per_step_per_row']} | {conf} |\n")


if __name__ == "__main__":
    main()
