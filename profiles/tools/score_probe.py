"""Time to score a sequence on the 3B model: HipModel.score (sd_model_score: layers through the prefill route, lm_head GEMM with a
log-softmax / argmax epilogue) against forward(logits F32) + torch.log_softmax, and the head kernel alone (score_head_kernel, timed with
a rocprofv3 kernel trace when one is wanted: the figure here is score minus forward(skip_head)). Then the perplexity of one synthetic
sequence under the bf16 and fp8 copies of the same model. `python profiles/tools/score_probe.py [L ...] [--weight-dtype bf16,fp8]`."""
import argparse
import dataclasses
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "llm-inference-lab_amd"))
import torch  # noqa: E402

from specdec_hip import weights as W  # noqa: E402
from specdec_hip.engine import HipModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("lens", type=int, nargs="*", default=[512, 2048])
ap.add_argument("--weight-dtype", default="bf16,fp8")
args = ap.parse_args()
cfg = dataclasses.replace(W.LLAMA_3_2_3B, max_pos=4096)
mw = W.synthetic_llama(cfg, seed=0, device="cuda")


def best(fn, reps=3):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return min(ts)


ppl = {}
for wd in args.weight_dtype.split(","):
    eng = HipModel(mw, batch=1, l_max=max(args.lens) + 64, weight_dtype=wd, prefill_backend="native")
    for L in args.lens:
        g = torch.Generator().manual_seed(L)
        seq = torch.randint(4, cfg.vocab, (L,), generator=g, dtype=torch.int32).cuda()
        zero = torch.zeros(1, dtype=torch.int32, device="cuda")
        eng.score(seq)   # workspace, plan
        t_score = best(lambda: eng.score(seq))
        t_layers = best(lambda: eng.forward(seq.view(1, -1), zero, 0, skip_head=True))

        def via_logits():
            _, lg = eng.forward(seq.view(1, -1), zero, 0, want_logits=True)
            torch.log_softmax(lg[0, :-1], dim=-1).gather(1, seq[1:].long().view(-1, 1))

        t_logits = best(via_logits)
        t_head = t_score - t_layers
        flop = 2.0 * L * cfg.vocab * cfg.d_model
        print(f"3B {wd} L={L:5d}: score {t_score:8.2f} ms | forward(logits) + log_softmax {t_logits:8.2f} ms | layers alone (native, "
              f"skip_head) {t_layers:8.2f} ms -> head + norm + finalize {t_head:6.2f} ms = {flop / (t_head * 1e-3) / 1e12:6.1f} TFLOP/s",
              flush=True)
    lp, _ = eng.score(torch.randint(4, cfg.vocab, (512,), generator=torch.Generator().manual_seed(1), dtype=torch.int32).cuda())
    ppl[wd] = -float(lp.double().mean())   # loss; a synthetic model's perplexity of random ids can exceed the double range
    del eng
    torch.cuda.empty_cache()
print("one 512-token sequence of random ids: " + ", ".join(
    f"{k} loss {v:.4f} (perplexity {math.exp(v) if v < 700 else float('inf'):.4g})" for k, v in ppl.items()), flush=True)
