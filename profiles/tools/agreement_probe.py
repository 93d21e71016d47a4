"""Time of SpeculativePipeline.draft_agreement on the synthetic 3B + 1B pair (score_logits of both models through the native prefill
route + sd_spec_agreement per chunk) against what the library offered before it: forward(want_logits) of both models, log_softmax
and the min / KL expressions in torch. Then the agreement kernels alone at n = 256, V = 128256 against the bytes they read.
`python profiles/tools/agreement_probe.py [L ...] [--weight-dtype bf16,fp8]`. Warm-up call first, then best and median of `reps`
timings between HIP events; every figure of a table comes from one run."""
import argparse
import dataclasses
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "llm-inference-lab_amd"))
import torch  # noqa: E402

from specdec_hip import ops  # noqa: E402
from specdec_hip import weights as W  # noqa: E402
from src.specdec import HipLM, SpeculativePipeline  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("lens", type=int, nargs="*", default=[512, 2048])
ap.add_argument("--weight-dtype", default="bf16,fp8")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()


def timed(fn, reps):
    fn()   # warm-up: workspaces, plans, allocator
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts), statistics.median(ts)


# ---- the kernels alone
n, V = 256, 128256
g = torch.Generator(device="cuda").manual_seed(0)
p = (torch.randn((n, V), generator=g, device="cuda") * 3.0).bfloat16()
q = (p.float() + 0.5 * torch.randn((n, V), generator=g, device="cuda")).bfloat16()
for T in (1.0, 0.7):
    best, med = timed(lambda: ops.spec_agreement(q, p, T), 20)
    nbytes = 2 * (2 * n * V * 2)   # two passes over both blocks
    print(f"sd_spec_agreement n={n} V={V} T={T}: best {best * 1e3:7.1f} us, median {med * 1e3:7.1f} us (three launches + the wrapper's "
          f"allocations) = {best * 1e3 / n:5.2f} us per position; {nbytes / 1e6:.0f} MB read -> {nbytes / (best * 1e-3) / 1e12:.2f} TB/s = "
          f"{nbytes / (best * 1e-3) / 8e12 * 100:.0f} % of 8 TB/s", flush=True)
del p, q

# ---- draft_agreement against the logits path
cfg_t = dataclasses.replace(W.LLAMA_3_2_3B, max_pos=4096)
cfg_d = dataclasses.replace(W.LLAMA_3_2_1B, max_pos=4096)
tgt = W.synthetic_llama(cfg_t, seed=0, device="cuda")
drf = W.synthetic_llama(cfg_d, seed=1, device="cuda", embed_from=tgt, flip_fraction=0.25)
for wd in args.weight_dtype.split(","):
    kw = dict(weight_dtype=wd, prefill_backend="native", max_len=max(args.lens) + 64)
    pipe = SpeculativePipeline(base_lm=HipLM(tgt, **kw), draft_lm=HipLM(drf, **kw), seed=1234)
    for L in args.lens:
        seq = torch.randint(4, cfg_t.vocab, (L,), generator=torch.Generator().manual_seed(L), dtype=torch.int32)
        ids = seq.tolist()
        r = pipe.draft_agreement(ids)
        t_new = timed(lambda: pipe.draft_agreement(ids), args.reps)
        engines = [lm._model for lm in (pipe.base_lm, pipe.draft_lm)]
        dev_seq = seq[:-1].cuda().view(1, -1)
        zero = torch.zeros(1, dtype=torch.int32, device="cuda")

        def via_logits():
            (_, lp), (_, lq) = [e.forward(dev_seq, zero, 0, want_logits=True) for e in engines]
            a, b = torch.log_softmax(lp[0], dim=-1), torch.log_softmax(lq[0], dim=-1)
            alpha = torch.minimum(a.exp(), b.exp()).sum(-1)
            kl = (a.exp() * (a - b)).sum(-1)
            agree = lp[0].argmax(-1) == lq[0].argmax(-1)
            return alpha.cpu(), kl.cpu(), agree.cpu()

        ref = via_logits()
        t_old = timed(via_logits, args.reps)
        print(f"3B + 1B {wd} L={L:5d}: draft_agreement best {t_new[0]:8.2f} ms median {t_new[1]:8.2f} ms | forward(logits) x 2 + torch "
              f"best {t_old[0]:8.2f} ms median {t_old[1]:8.2f} ms | mean alpha {r['mean_alpha']:.4f} (torch fp32: "
              f"{float(ref[0].double().mean()):.4f}), greedy agreement {r['greedy_agreement']:.4f} ({float(ref[2].double().mean()):.4f})",
              flush=True)
    del pipe
    torch.cuda.empty_cache()
