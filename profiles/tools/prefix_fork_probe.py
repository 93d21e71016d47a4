"""What sharing a prompt between cache rows saves: session set-up time (DecodeSession construction until the first step can
launch, device drained) for B rows that hold the same prompt with share_prefix off and on, and the fork kernel by itself
(HIP events around HipModel.fork_row: duration and achieved bytes/s). 3B + 1B synthetic pair, bf16, dense and paged KV.
`python profiles/tools/prefix_fork_probe.py [--root DIR] [--lens 512,...] [--rows 8] [--page-len 64] [--reps 7]`
--root: the repository tree to import the package from (a checkout of another commit, for the comparison; a tree without
share_prefix measures the unshared set-up only). Prints one JSON line per measurement."""
import argparse
import inspect
import json
import os
import statistics
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
ap.add_argument("--lens", default="512")
ap.add_argument("--rows", type=int, default=8)
ap.add_argument("--page-len", type=int, default=64)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--label", default="")
args = ap.parse_args()
sys.path.insert(0, os.path.join(os.path.abspath(args.root), "llm-inference-lab_amd"))
sys.path.insert(0, os.path.join(os.path.abspath(args.root), "llm-inference-lab_amd", "src"))
import torch  # noqa: E402

from specdec_hip import weights as W  # noqa: E402
from specdec_hip.engine import HipSpecDec  # noqa: E402
from src.specdec import HipLM, SpeculativePipeline  # noqa: E402
from src.specdec.core.pipeline import DecodeSession  # noqa: E402

can_share = "share_prefix" in inspect.signature(DecodeSession.__init__).parameters
tgt = W.synthetic_llama(W.LLAMA_3_2_3B, seed=0, device="cuda")
drf = W.synthetic_llama(W.LLAMA_3_2_1B, seed=1, device="cuda", embed_from=tgt, flip_fraction=0.2)
B, K = args.rows, 4


def out(**kw):
    print(json.dumps({"label": args.label, "rows": B, **kw}), flush=True)


def setup_ms(pipe, prompts, share):
    kw = {"share_prefix": True} if share else {}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sess = pipe.start_session(prompts, max_tokens=64, emit_mode=HipSpecDec.EMIT_BONUS, **kw)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3
    stats = dict(sess.stats)
    sess.finish()
    return ms, stats


for kv in ("dense", "paged"):
    lm_kw = {"kv_page_len": args.page_len} if kv == "paged" else {}
    pipe = SpeculativePipeline(base_lm=HipLM(tgt, **lm_kw), draft_lm=HipLM(drf, **lm_kw), draft_model="none", controller="fixed",
                               controller_params={"k": K}, seed=1234)
    for L in [int(x) for x in args.lens.split(",")]:
        g = torch.Generator().manual_seed(1234)
        prompt = torch.randint(4, tgt.config.vocab, (L,), generator=g, dtype=torch.int64).tolist()
        prompts = [prompt] * B
        modes = [False, True] if can_share else [False]
        for share in modes:                      # first use: engines, loop, graph-free warm-up of both routes
            setup_ms(pipe, prompts, share)
        ts = {m: [] for m in modes}
        for _ in range(args.reps):               # interleaved rounds in one process
            for share in modes:
                ms, stats = setup_ms(pipe, prompts, share)
                ts[share].append(ms)
        for share in modes:
            out(what="session_setup_ms", kv=kv, prompt_len=L, share_prefix=share, median=round(statistics.median(ts[share]), 3),
                min=round(min(ts[share]), 3), reps=args.reps)
        if not can_share:
            continue
        rt = next(iter(pipe._runtimes.values()))
        for role in ("target", "draft"):
            eng = rt[role]
            c = eng.cfg
            n = L - 1
            for b in range(B):
                eng.release(b)
            eng.reserve(0, n)
            dsts = list(range(1, B))
            durs = []
            for i in range(args.reps + 2):
                a, b_ = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                eng.fork_row(0, dsts, n)
                b_.record()
                torch.cuda.synchronize()
                if i >= 2:
                    durs.append(a.elapsed_time(b_) * 1e3)
            if kv == "dense":
                moved = (1 + len(dsts)) * 2 * c.n_layers * c.n_kv_heads * n * c.head_dim * 2
            else:                                # only the pages from position n - 2 on are copied, once per destination
                P = eng.page_len
                copied = n - max(n - 2, 0) // P * P
                moved = 2 * len(dsts) * 2 * c.n_layers * c.n_kv_heads * copied * c.head_dim * 2
            us = statistics.median(durs)
            out(what="fork_row_us", kv=kv, prompt_len=L, engine=role, median=round(us, 2), min=round(min(durs), 2),
                bytes_moved=moved, gb_per_s=round(moved / us / 1e3, 1), pages_in_use=eng.pages_in_use() if kv == "paged" else None)
            for b in range(B):
                eng.release(b)
