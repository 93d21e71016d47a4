"""What an e4m3 KV cache (kv_cache_dtype fp8) buys on an MI355X, written to profiles/kv_fp8.md:

  (a) the forwards a K = 4 step of the 3B / 1B pair is made of — the target's 5-token verify pass and the draft's 1-token pass, both on
      the launch path — at 128, 8192 and 32768 cached positions, bf16 and fp8 KV alternating in one session (sd_model_probe_forward:
      device events around `iters` forwards of one row), and the step they add up to: verify + 5 draft forwards.
  (b) the same passes without their attention launches' share: --trace-only runs just the forwards, for a
      `rocprofv3 --kernel-trace --stats -- python scripts/kv_fp8_bench.py --trace-only --context N` run of its own per length, whose average
      attention_mfma_kernel / attention_mfma_kv8_kernel durations go into the document by hand.
  (c) RMS and maximum difference of the last position's logits between the two cache types over a 512-token prompt at the full-depth
      Llama-3.2-1B and 3B shapes (random_init weights), as a fraction of RMS(logits). A record, not a gate.

    python scripts/kv_fp8_bench.py [--out profiles/kv_fp8.md] [--trace-only] [--skip-logits]

Needs a GPU; there is no fallback."""

import argparse
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

CONTEXTS = (128, 8192, 32768)
SHAPES = {"llama-3.2-3b": ("target", 5), "llama-3.2-1b": ("draft", 1)}     # role, tokens per pass of the K = 4 step


def _cfg(W, name, max_pos=None):
    import dataclasses

    base = {"llama-3.2-1b": W.LLAMA_3_2_1B, "llama-3.2-3b": W.LLAMA_3_2_3B}[name]
    return dataclasses.replace(base, max_pos=max_pos) if max_pos else base


def measure_forwards(lines, rounds, iters, trace_only, contexts=CONTEXTS):
    from specdec_hip import weights as W
    from specdec_hip.engine import HipModel

    table = {}
    for name, (role, M) in SHAPES.items():
        mw = W.synthetic_llama(_cfg(W, name, 33024), seed=0, device="cuda")
        for ctx in contexts:
            engines = {d: HipModel(mw, batch=1, l_max=ctx + 256, kv_dtype=d) for d in ("bf16", "fp8")}
            for e in engines.values():
                e.set_persist_tokens(0)           # both on the launch path (where an 8 K or 32 K session is anyway)
                e.set_length_hint(ctx + 64)
                e.probe_forward(M, 3, pos0=ctx)
            samples = {d: [] for d in engines}
            for _ in range(1 if trace_only else rounds):      # alternating
                for d, e in engines.items():
                    samples[d].append(e.probe_forward(M, iters, pos0=ctx)[0])
            table[(role, ctx)] = {d: (statistics.median(v), min(v), max(v)) for d, v in samples.items()}
            del engines
            torch.cuda.empty_cache()
        del mw
        torch.cuda.empty_cache()
    if trace_only:
        return
    lines += ["## (a) the forwards of a K = 4 step, one row", "",
              f"us per forward between device events, median (min-max) of {rounds} alternating windows of {iters} forwards; launch path.", "",
              "| pass | cached positions | bf16 KV | fp8 KV | fp8 / bf16 |", "|---|---|---|---|---|"]
    for (role, ctx), r in table.items():
        b, f = r["bf16"], r["fp8"]
        lines.append(f"| {role} ({'5-token verify' if role == 'target' else '1-token draft'}) | {ctx} | {b[0]:.0f} ({b[1]:.0f}-{b[2]:.0f}) | "
                     f"{f[0]:.0f} ({f[1]:.0f}-{f[2]:.0f}) | {f[0] / b[0]:.3f} |")
    lines += ["", "The step these add up to (verify + 5 draft forwards; the captured step also holds the accept / record launches, which do not "
              "depend on the cache):", "", "| cached positions | bf16 KV ms | fp8 KV ms | saved ms |", "|---|---|---|---|"]
    for ctx in CONTEXTS:
        s = {d: (table[("target", ctx)][d][0] + 5 * table[("draft", ctx)][d][0]) / 1e3 for d in ("bf16", "fp8")}
        lines.append(f"| {ctx} | {s['bf16']:.3f} | {s['fp8']:.3f} | {s['bf16'] - s['fp8']:.3f} |")
    lines.append("")


def measure_logits(lines):
    from specdec_hip import weights as W
    from specdec_hip.engine import HipModel

    lines += ["## (c) last-position logits, fp8 KV against bf16 KV", "",
              "Full-depth shapes, random_init weights, one 512-token prompt then its last position's logits (fp32 read-out); scales (1, 1).", "",
              "| shape | RMS(logits) | RMS difference | max difference | RMS difference / RMS(logits) | max / RMS(logits) |", "|---|---|---|---|---|---|"]
    for name in ("llama-3.2-1b", "llama-3.2-3b"):
        mw = W.random_init(_cfg(W, name), seed=3, device="cuda")
        tok = torch.randint(4, mw.config.vocab, (1, 512), generator=torch.Generator(device="cuda").manual_seed(5), device="cuda", dtype=torch.int32)
        out = {}
        for d in ("bf16", "fp8"):
            e = HipModel(mw, batch=1, l_max=1024, kv_dtype=d, prefill_backend="passes")
            zero = torch.zeros(1, dtype=torch.int32, device="cuda")
            e.forward(tok[:, :-1], zero, skip_head=True)
            out[d] = e.forward(tok[:, -1:], zero + 511, want_logits=True)[1].double().flatten()
            del e
        diff, rms = out["fp8"] - out["bf16"], float(out["bf16"].pow(2).mean().sqrt())
        d_rms, d_max = float(diff.pow(2).mean().sqrt()), float(diff.abs().max())
        lines.append(f"| {name} | {rms:.4f} | {d_rms:.5f} | {d_max:.5f} | {d_rms / rms:.4f} | {d_max / rms:.4f} |")
        del mw, out
        torch.cuda.empty_cache()
    lines.append("")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kv_fp8.md"))
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--trace-only", action="store_true")
    ap.add_argument("--context", type=int, help="--trace-only: this context length alone (one rocprofv3 run per length)")
    ap.add_argument("--skip-logits", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("kv_fp8_bench needs a GPU")
    lines = ["# FP8 (e4m3) KV cache: measurements", "", f"{torch.cuda.get_device_name(0)}; scripts/kv_fp8_bench.py. Nothing here is a gate.", ""]
    measure_forwards(lines, args.rounds, args.iters, args.trace_only, (args.context,) if args.trace_only and args.context else CONTEXTS)
    if args.trace_only:
        return
    if not args.skip_logits:
        measure_logits(lines)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
