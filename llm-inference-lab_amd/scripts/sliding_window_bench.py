"""What sliding-window attention (HipModel(sliding_window=W), csrc/attention_window.hip) costs and saves on an MI355X, written to
profiles/sliding_window.md.

Decode-shaped launches: the 3B-head target (Hq 24, Hkv 8, D 128) and the 1B-head draft (Hq 32, Hkv 8, D 64) with --layers layers,
M = 5 and M = 1 tokens of one row at 64, 4 K, 8 K and 32 K cached keys, W = 4096 against window off (the plain kernel: with no
window a launch takes the code it always took), alternating in one process, layers only, launch path. A forward is GEMVs plus one
attention launch per layer, and only the latter depends on the context: the table gives us per layer and, as the attention term,
the excess over the same engine's forward at 64 keys.

Prompts: --layers 2 models, one prompt of 8 K and 32 K tokens through the native GEMM route with tiled prompt attention, W = 4096
against off, alternating.

    python scripts/sliding_window_bench.py [--out profiles/sliding_window.md] [--layers 4]

Needs a GPU; there is no fallback. Unwritten caches: the launches do not depend on the values."""

import argparse
import dataclasses
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

WINDOW, CTX, L_MAX = 4096, (64, 4096, 8192, 32768), 33024


def _timed(eng, tok, pos, iters):
    """us per forward between device events"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        eng.forward(tok, pos, want_ids=False, skip_head=True)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def _alternate(engines, tok, pos, rounds, iters):
    """{key: (median, min, max)} of `rounds` alternating windows"""
    for e in engines.values():
        _timed(e, tok, pos, 2)
    t = {k: [] for k in engines}
    for _ in range(rounds):
        for k, e in engines.items():
            t[k].append(_timed(e, tok, pos, iters))
    return {k: (statistics.median(v), min(v), max(v)) for k, v in t.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sliding_window.md"))
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sliding_window_bench needs a GPU")
    from specdec_hip import weights as W
    from specdec_hip.engine import HipModel

    fmt = lambda s: f"{s[0]:.0f} ({s[1]:.0f}-{s[2]:.0f})"     # noqa: E731
    lines = ["# Sliding-window attention: measurements", "",
             f"{torch.cuda.get_device_name(0)}; scripts/sliding_window_bench.py --layers {args.layers}. Nothing here is a gate.", "",
             f"## Decode-shaped launches, W = {WINDOW}", "",
             f"us per forward (layers only, {args.layers} layers) between device events, median (min-max) of {args.rounds} alternating windows of "
             f"{args.iters} forwards; one row, launch path. Attention term = (forward - the same engine's forward at 64 keys) / layers.", "",
             "| model | M | cached keys | off | W on | attention term off, us per layer | on | on / off's 4 K term |", "|---|---|---|---|---|---|---|---|"]
    shapes = {"llama-3.2-3b": W.LLAMA_3_2_3B, "llama-3.2-1b": W.LLAMA_3_2_1B}
    for name, base in shapes.items():
        mw = W.synthetic_llama(dataclasses.replace(base, max_pos=L_MAX, n_layers=args.layers), seed=0, device="cuda")
        eng = {w: HipModel(mw, batch=1, l_max=L_MAX, sliding_window=w) for w in (0, WINDOW)}
        for e in eng.values():
            e.set_persist_tokens(0)
        for M in (5, 1):
            tok = torch.randint(4, mw.config.vocab, (1, M), device="cuda", dtype=torch.int32)
            res = {n: _alternate(eng, tok, torch.tensor([n], dtype=torch.int32, device="cuda"), args.rounds, args.iters) for n in CTX}
            term = {n: {w: (res[n][w][0] - res[64][w][0]) / args.layers for w in eng} for n in CTX}
            for n in CTX[1:]:
                lines.append(f"| {name} heads, D = {mw.config.head_dim} | {M} | {n} | {fmt(res[n][0])} | {fmt(res[n][WINDOW])} | {term[n][0]:.1f} | "
                             f"{term[n][WINDOW]:.1f} | {term[n][WINDOW] / term[4096][0]:.2f} |")
                print(lines[-1], flush=True)
        del eng, mw
        torch.cuda.empty_cache()
    lines += ["", f"## Prompts, tiled prompt attention, W = {WINDOW}", "",
              "ms per prompt (2 layers, layers only, native GEMM route, one row) between device events, median (min-max) of 3 alternating windows of "
              "2 prompts.", "", "| model | prompt tokens | off | W on | on / off |", "|---|---|---|---|---|"]
    for name, base in shapes.items():
        mw = W.synthetic_llama(dataclasses.replace(base, max_pos=L_MAX, n_layers=2), seed=0, device="cuda")
        eng = {w: HipModel(mw, batch=1, l_max=L_MAX, prefill_backend="native", prefill_attention="tiled", sliding_window=w) for w in (0, WINDOW)}
        for L in (8192, 32768):
            tok = torch.randint(4, mw.config.vocab, (1, L), device="cuda", dtype=torch.int32)
            res = _alternate(eng, tok, torch.zeros(1, dtype=torch.int32, device="cuda"), 3, 2)
            off, on = ((v[0] / 1e3, v[1] / 1e3, v[2] / 1e3) for v in (res[0], res[WINDOW]))
            lines.append(f"| {name} heads, D = {mw.config.head_dim} | {L} | {off[0]:.1f} ({off[1]:.1f}-{off[2]:.1f}) | "
                         f"{on[0]:.1f} ({on[1]:.1f}-{on[2]:.1f}) | {on[0] / off[0]:.3f} |")
            print(lines[-1], flush=True)
        del eng, mw
        torch.cuda.empty_cache()
    lines.append("")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
