"""Cost of speculative sampling inside the captured step (csrc/spec_sample.hip) on the headline pair (synthetic Llama-3.2-3B
target + 1B draft, K = 4, bf16):

  steps    ms per captured step of the greedy step, the sampled-bonus step (T 0.7, top_k 50, top_p 0.9), the
           speculative-sampling step and its top-k / top-p shaped variant (top_k 50, top_p 0.9), 1 row and 8 rows, the device
           advancing its own state (no host rule between steps); --modes picks a subset (a library without the shaped
           variant: --modes greedy,sampled-bonus,speculative);
  decode   tokens/s of generate_batch(policy="rejection") with backend="device" against backend="host" (the host loop);
  trace    a short run of the speculative-sampling step alone, for `rocprofv3 --kernel-trace --stats -- python ... trace`;
  trace-shaped   the same for the shaped step.

`python profiles/tools/spec_sample_probe.py {steps,decode,trace,trace-shaped} [--rows 1,8] [--steps 60]`. Run each leg in a
process of its own with a time limit (`timeout -k 10 600 python ...`); results are written up in profiles/spec_sampling.md
and profiles/spec_sampling_shaped.md."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "llm-inference-lab_amd"))
import torch  # noqa: E402

from specdec_hip import weights as W  # noqa: E402
from specdec_hip.engine import HipSpecDec  # noqa: E402
from src.specdec import HipLM, SpeculativePipeline  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("leg", choices=["steps", "decode", "trace", "trace-shaped"])
ap.add_argument("--modes", default="greedy,sampled-bonus,speculative,shaped")
ap.add_argument("--rows", default="1,8")
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--k", type=int, default=4)
ap.add_argument("--temperature", type=float, default=0.7)
ap.add_argument("--flip", type=float, default=0.2)
ap.add_argument("--max-tokens", type=int, default=64)
args = ap.parse_args()
K, T = args.k, args.temperature

tgt = W.synthetic_llama(W.LLAMA_3_2_3B, seed=0, device="cuda")
drf = W.synthetic_llama(W.LLAMA_3_2_1B, seed=1, device="cuda", embed_from=tgt, flip_fraction=args.flip)
V = tgt.config.vocab


def prompts(n, length=32):
    return [torch.randint(4, V, (length,), generator=torch.Generator().manual_seed(1234 + i)).tolist() for i in range(n)]


def pipeline(policy="longest_prefix", params=None):
    return SpeculativePipeline(base_lm=HipLM(tgt), draft_lm=HipLM(drf), controller="fixed", controller_params={"k": K}, seed=1234,
                               policy=policy, policy_params=params)


def time_steps(loop, n):
    """ms per step over n captured steps, after 3 warm-up steps (the first is eager, the second captures); 3 repeats, the best"""
    for _ in range(3):
        loop.step(use_graph=True)
    loop.sync()
    best = float("inf")
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            loop.step(use_graph=True)
        loop.sync()
        best = min(best, (time.perf_counter() - t0) * 1e3 / n)
    return best


def mode_steps(B, mode, n):
    pipe = pipeline()
    # room for every step of the three timing repeats plus the warm-up at full acceptance
    sess = pipe.start_session(prompts(B), (3 * n + 8) * (K + 1), HipSpecDec.EMIT_BONUS, None)
    loop = sess.loop
    loop.sync()
    if mode == "sampled-bonus":
        loop.set_sampling(True, T, 50, 0.9, 1234)
    elif mode == "speculative":
        loop.set_spec_sampling(True, T, 1234)
    elif mode == "shaped":
        loop.set_spec_sampling(True, T, 1234, top_k=50, top_p=0.9)
    ms = time_steps(loop, n)
    rec = loop.sync()
    acc = float(rec.accept_len.mean())
    if mode == "sampled-bonus":
        loop.set_sampling(False)
    elif mode in ("speculative", "shaped"):
        loop.set_spec_sampling(False)
    sess.finish()
    return ms, acc


if args.leg == "steps":
    for B in [int(x) for x in args.rows.split(",")]:
        res = {m: mode_steps(B, m, args.steps) for m in args.modes.split(",")}
        g = next(iter(res.values()))[0]
        print(f"3B + 1B, K={K}, {B} row(s), bf16, T={T}: " + ", ".join(
            f"{m} {ms:.3f} ms/step (x{ms / g:.3f}, last accept length {a:.2f})" for m, (ms, a) in res.items()), flush=True)
elif args.leg == "decode":
    for B in [int(x) for x in args.rows.split(",")]:
        out = {}
        for backend in ("device", "host"):
            pipe = pipeline("rejection", {"backend": backend, "temperature": T, "seed": 7})
            pipe.generate_batch(prompts(B), max_tokens=8)           # engines, capture
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = pipe.generate_batch(prompts(B), max_tokens=args.max_tokens)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            n = sum(len(x["generated_tokens"]) for x in r)
            out[backend] = (n / dt, n, sum(x["accepted"] for x in r) / max(sum(x["proposed"] for x in r), 1))
            del pipe
            torch.cuda.empty_cache()
        print(f"generate_batch(policy='rejection'), 3B + 1B, K={K}, {B} row(s), T={T}, max_tokens={args.max_tokens}: " + ", ".join(
            f"{b} {tps:.1f} tokens/s ({n} tokens, accepted/proposed {ar:.2f})" for b, (tps, n, ar) in out.items())
            + f" -> device / host = {out['device'][0] / out['host'][0]:.2f}", flush=True)
else:
    mode = "shaped" if args.leg == "trace-shaped" else "speculative"
    ms, _ = mode_steps(1, mode, 20)
    print(f"trace leg: {mode} step {ms:.3f} ms/step under the profiler", flush=True)
