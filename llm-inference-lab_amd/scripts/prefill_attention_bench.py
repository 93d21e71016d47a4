"""What the tiled prompt-attention kernel (prefill_attention="tiled", csrc/attention_prefill.hip) changes on an MI355X, written to
profiles/prefill_attention.md:

  (a) prefill of 512, 2048, 8192 and 32768 tokens at the Llama-3.2-3B and 1B head geometries (--layers layers of each, seeded
      weights), the mode off ("passes") and on ("tiled") alternating in one process: ms per prefill between device synchronisations,
      median (min-max) over --rounds rounds after a warm-up of every shape and mode.
  (b) the causal attention FLOPs of each prefill from shapes alone, 2 * 2 * D * Hq * sum of visible keys per layer. Divided by the
      kernel time of a `rocprofv3 --kernel-trace --stats -- python scripts/prefill_attention_bench.py --trace-only --mode M
      --context N --shape S` run of its own they give the achieved FLOP/s; those figures go into the document by hand.

    python scripts/prefill_attention_bench.py [--out profiles/prefill_attention.md] [--layers 2] [--rounds 5]

Needs a GPU; there is no fallback."""

import argparse
import dataclasses
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
PKG = os.path.dirname(HERE)
ROOT = os.path.dirname(PKG)
for p in (PKG, ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

CONTEXTS = (512, 2048, 8192, 32768)
MODES = ("passes", "tiled")


def _weights(name, layers):
    from specdec_hip import weights as W

    base = {"llama-3.2-1b": W.LLAMA_3_2_1B, "llama-3.2-3b": W.LLAMA_3_2_3B}[name]
    return W.synthetic_llama(dataclasses.replace(base, n_layers=layers, max_pos=33024), seed=0, device="cuda")


def causal_flops(cfg, L):
    """per layer: QK^T and PV over the L (L + 1) / 2 visible (query, key) pairs of every query head"""
    return 2 * 2 * cfg.head_dim * cfg.n_heads * L * (L + 1) // 2


def prefill_ms(eng, tok):
    zero = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.forward(tok, zero, skip_head=True)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prefill_attention.md"))
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--trace-only", action="store_true", help="one warm-up and one prefill of --shape / --context in --mode, nothing written")
    ap.add_argument("--mode", choices=MODES, default="tiled")
    ap.add_argument("--context", type=int, default=8192)
    ap.add_argument("--shape", choices=["llama-3.2-3b", "llama-3.2-1b"], default="llama-3.2-3b")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("prefill_attention_bench needs a GPU")
    from specdec_hip.engine import HipModel

    shapes = (args.shape,) if args.trace_only else ("llama-3.2-3b", "llama-3.2-1b")
    contexts = (args.context,) if args.trace_only else CONTEXTS
    modes = (args.mode,) if args.trace_only else MODES
    lines = ["# Tiled prompt attention: measurements", "",
             f"{torch.cuda.get_device_name(0)}; scripts/prefill_attention_bench.py --layers {args.layers}. Nothing here is a gate.", "",
             "## (a) prefill, the mode off and on alternating", "",
             f"ms per prefill of one row (native GEMM backend, {args.layers} layers, no lm_head), median (min-max) of {args.rounds} alternating rounds.", "",
             "| shape | tokens | passes ms | tiled ms | tiled / passes | causal attention GFLOP per layer |", "|---|---|---|---|---|---|"]
    for name in shapes:
        mw = _weights(name, args.layers)
        gen = torch.Generator(device="cuda").manual_seed(11)
        for L in contexts:
            tok = torch.randint(4, mw.config.vocab, (1, L), generator=gen, device="cuda", dtype=torch.int32)
            engines = {m: HipModel(mw, batch=1, l_max=L + 64, prefill_backend="native", prefill_attention=m) for m in modes}
            for e in engines.values():
                prefill_ms(e, tok)                      # warm-up of this shape in this mode
            samples = {m: [] for m in modes}
            for _ in range(1 if args.trace_only else args.rounds):
                for m, e in engines.items():            # alternating
                    samples[m].append(prefill_ms(e, tok))
            if not args.trace_only:
                p, t = (samples[m] for m in MODES)
                assert engines["tiled"].prefill_tiled_launches() > 0 and engines["passes"].prefill_tiled_launches() == 0
                lines.append(f"| {name} | {L} | {statistics.median(p):.2f} ({min(p):.2f}-{max(p):.2f}) | {statistics.median(t):.2f} "
                             f"({min(t):.2f}-{max(t):.2f}) | {statistics.median(t) / statistics.median(p):.3f} | {causal_flops(mw.config, L) / 1e9:.1f} |")
                print(lines[-1], flush=True)
            del engines
            torch.cuda.empty_cache()
        del mw
        torch.cuda.empty_cache()
    if args.trace_only:
        return
    lines.append("")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
