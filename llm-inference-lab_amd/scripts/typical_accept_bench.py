"""ms per step and tokens per step of the captured step under the device acceptance rules, against the greedy and the sampled-bonus
step, on one pair and the same prompts (profiles/typical_accept.md).

    python llm-inference-lab_amd/scripts/typical_accept_bench.py [--target llama-3.2-3b --draft llama-3.2-1b --k 4 --steps 60 --warmup 10]

Prints one JSON line per mode: greedy (longest_prefix), sampled (longest_prefix, do_sample), typical at (epsilon, delta, T) =
(0.09, 0.3, 0.7) greedy and sampled, topk_agree k = 1 and k = 5. With --soft G the target's final norm weight is scaled by G: the
synthetic target is all but one-hot, so without it a lossy rule accepts what exact match accepts (same tokens per step); the cost
per step does not depend on it."""

import argparse
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.dirname(ROOT)]

import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--target", default="llama-3.2-3b")
    ap.add_argument("--draft", default="llama-3.2-1b")
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--flip", type=float, default=0.2)
    ap.add_argument("--soft", type=float, default=None)
    args = ap.parse_args()
    from specdec_hip import weights as W
    from specdec_hip.engine import HipSpecDec
    from src.specdec import HipLM, SpeculativePipeline

    presets = {"llama-3.2-1b": W.LLAMA_3_2_1B, "llama-3.2-3b": W.LLAMA_3_2_3B, "llama-3-8b": W.LLAMA_3_8B}
    tgt = W.synthetic_llama(presets[args.target], seed=0, device="cuda")
    drf = W.synthetic_llama(presets[args.draft], seed=1, device="cuda", embed_from=tgt, flip_fraction=args.flip)
    if args.soft:
        tgt.final_norm_w = (tgt.final_norm_w.float() * args.soft).to(tgt.final_norm_w.dtype)
    base, draft = HipLM(tgt), HipLM(drf)
    V = tgt.config.vocab
    prompts = [torch.randint(4, V, (32,), generator=torch.Generator().manual_seed(1234 + i), dtype=torch.int64).tolist() for i in range(args.batch)]
    typical = {"backend": "device", "p": 0.09, "delta": 0.3, "temperature": 0.7}
    sampling = {"temperature": 0.7, "top_k": 50, "top_p": 0.9, "seed": 1234}
    modes = [("greedy", "longest_prefix", None, None), ("sampled_bonus", "longest_prefix", None, sampling),
             ("typical", "typical", typical, None), ("typical+sampled", "typical", typical, sampling),
             ("topk_agree_k1", "topk_agree", {"backend": "device", "k": 1}, None), ("topk_agree_k5", "topk_agree", {"backend": "device", "k": 5}, None)]
    total = args.warmup + args.steps
    for name, policy, pp, samp in modes:
        pipe = SpeculativePipeline(base_lm=base, draft_lm=draft, draft_model="none", controller="fixed", controller_params={"k": args.k},
                                   seed=1234, policy=policy, policy_params=pp)
        sess = pipe.start_session(prompts, max_tokens=total * (args.k + 1) + 1, emit_mode=HipSpecDec.EMIT_BONUS, sampling=samp)
        for _ in range(args.warmup):
            sess.advance()
        n0 = sum(len(r.generated) for r in sess.rows)
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
        print(json.dumps({"mode": name, "ms_per_step": round(1e3 * dt / args.steps, 4), "tokens_per_step_per_row": round(n / args.steps / args.batch, 3),
                          "graph_nodes": nodes, "resyncs": sess.stats["resyncs"], "k": args.k, "batch": args.batch, "soft": args.soft}), flush=True)
        del sess, pipe


if __name__ == "__main__":
    main()
