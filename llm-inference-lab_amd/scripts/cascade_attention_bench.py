"""What cascade attention (HipModel(cascade=True), csrc/attention_cascade.hip) buys on an MI355X, written to
profiles/cascade_attention.md: the forwards a K = 4 step of the 3B / 1B pair is made of — the target's 5-token verify pass and the
draft's 1-token pass, on the launch path — for 2, 4 and 8 rows that share 2 K, 8 K and 32 K positions (each row 64 positions past
the shared prefix), cascade on against cascade off alternating in one process. The models keep their layer shapes but only
--layers layers (the attention term is per layer; the table gives the difference per layer), with unwritten caches: the launches
do not depend on the values.

    python scripts/cascade_attention_bench.py [--out profiles/cascade_attention.md] [--layers 4]

Needs a GPU; there is no fallback."""

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

ROWS, SHARED = (2, 4, 8), (2048, 8192, 32768)
SHAPES = {"llama-3.2-3b": ("target, 5-token verify", 5), "llama-3.2-1b": ("draft, 1 token", 1)}


def _window(eng, tok, pos, iters):
    """us per forward between device events"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(iters):
        eng.forward(tok, pos, want_ids=False, skip_head=True)
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cascade_attention.md"))
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cascade_attention_bench needs a GPU")
    from specdec_hip import weights as W
    from specdec_hip.engine import HipModel

    lines = ["# Cascade attention: measurements", "", f"{torch.cuda.get_device_name(0)}; scripts/cascade_attention_bench.py --layers {args.layers}. "
             "Nothing here is a gate.", "", f"us per forward (layers only) between device events, median (min-max) of {args.rounds} alternating windows of "
             f"{args.iters} forwards; every row holds the shared positions + 64; launch path.", "",
             "| pass | rows | shared positions | cascade off | cascade on | on / off | saved us per layer |", "|---|---|---|---|---|---|---|"]
    for name, (what, M) in SHAPES.items():
        base = {"llama-3.2-1b": W.LLAMA_3_2_1B, "llama-3.2-3b": W.LLAMA_3_2_3B}[name]
        mw = W.synthetic_llama(dataclasses.replace(base, max_pos=33024, n_layers=args.layers), seed=0, device="cuda")
        for rows in ROWS:
            for shared in SHARED:
                eng = {on: HipModel(mw, batch=rows, l_max=shared + 256, cascade=on) for on in (False, True)}
                tok = torch.randint(4, mw.config.vocab, (rows, M), device="cuda", dtype=torch.int32)
                pos = torch.full((rows,), shared + 64, dtype=torch.int32, device="cuda")
                eng[True].set_shared_prefix(0, 0, shared)
                for b in range(1, rows):
                    eng[True].set_shared_prefix(b, 0, shared)
                for e in eng.values():
                    e.set_persist_tokens(0)
                    _window(e, tok, pos, 3)
                t = {on: [] for on in eng}
                for _ in range(args.rounds):
                    for on, e in eng.items():
                        t[on].append(_window(e, tok, pos, args.iters))
                off, on = (statistics.median(t[k]) for k in (False, True))
                lines.append(f"| {what} | {rows} | {shared} | {off:.0f} ({min(t[False]):.0f}-{max(t[False]):.0f}) | "
                             f"{on:.0f} ({min(t[True]):.0f}-{max(t[True]):.0f}) | {on / off:.3f} | {(off - on) / args.layers:.1f} |")
                print(lines[-1], flush=True)
                del eng
                torch.cuda.empty_cache()
        del mw
        torch.cuda.empty_cache()
    lines.append("")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
