"""Measurements of the rolling context window on an MI355X, written to profiles/rolling_context.md:

  (a) one evict_row (csrc/kv_evict.hip) at the cache geometries of Llama-3.2-1B and 3B (layers x KV heads x head_dim; the weights
      of the stand-in models are small, the launch reads none), n_pos 4096 and 32768, 4 sinks, the default drop: graph replays
      between device events, beside a torch restatement of the same move and rotation on kv_view() of the same tensors; bytes
      moved (every moved position read once and written once, K and V) per second against the HBM peak.
  (b) ms per step of a session whose window is never reached against the same session without a window, alternating.
  (c) the amortised cost of the rolls per generated token at context_window=4096.

    python scripts/rolling_context_bench.py [--out profiles/rolling_context.md] [--skip-session]

Needs a GPU; there is no fallback."""

import argparse
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

HBM_PEAK, HBM_ACHIEVABLE = 8.0e12, 6.3e12      # bytes / s: the spec figure, and what a streaming kernel reaches
GEOMETRIES = {"llama-3.2-1b": (16, 8, 64), "llama-3.2-3b": (28, 8, 128)}      # layers, KV heads, head_dim


def moved_bytes(layers, hkv, d, keep, drop, n_pos):
    """K and V of every moved position, read once and written once"""
    return 2 * 2 * layers * hkv * d * 2 * max(n_pos - keep - drop, 0)


def torch_evict(model, row, keep, drop, n_pos):
    """the same move and rotation with torch ops on kv_view(): per layer a strided copy of V, and K through fp32 temporaries"""
    k, v = model.kv_view()
    w = model.weights
    half = model.cfg.head_dim // 2
    c, s = w.rope_cos[drop], w.rope_sin[drop]
    for li in range(model.cfg.n_layers):
        src = k[li, row, :, keep + drop:n_pos].float()
        a, b = src[..., :half], src[..., half:]
        k[li, row, :, keep:n_pos - drop] = torch.cat([a * c + b * s, b * c - a * s], -1).to(torch.bfloat16)
        v[li, row, :, :, keep:n_pos - drop] = v[li, row, :, :, keep + drop:n_pos].clone()


def time_ms(fn, reps, rounds=5):
    """median over `rounds` windows of `reps` calls between two device events -> ms per call, (min, max)"""
    out = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / reps)
    return statistics.median(out), (min(out), max(out))


def measure_evict(lines):
    from specdec_hip import weights as W
    from specdec_hip.engine import HipModel
    from src.specdec.core.rolling import drop_of

    lines += ["## (a) one evict_row", "",
              "| cache geometry | n_pos | drop | moved MB (read + write) | evict_row ms (min-max) | TB/s | of 8 TB/s peak | of 6.3 TB/s | torch ms | torch / kernel |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for name, (layers, hkv, d) in GEOMETRIES.items():
        cfg = W.ModelConfig(arch=W.ARCH_LLAMA, n_layers=layers, d_model=hkv * d // 4, n_heads=hkv, n_kv_heads=hkv, head_dim=d, d_ff=256,
                            vocab=512, max_pos=32768, rope_theta=500000.0, rope_scaling=None, tie_embeddings=False, name=f"geometry-{name}")
        mw = W.random_init(cfg, seed=1, device="cuda")
        for n_pos in (4096, 32768):
            m = HipModel(mw, batch=1, l_max=n_pos)
            k, v = m.kv_view()
            k.normal_()
            v.normal_()
            keep, drop = 4, drop_of(n_pos, 4)
            stream = torch.cuda.Stream()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(stream):
                m.evict_row(0, keep, drop, n_pos, stream=stream)          # (code object loaded before the capture)
                stream.synchronize()
                with torch.cuda.graph(graph, stream=stream):
                    m.evict_row(0, keep, drop, n_pos, stream=stream)
            torch.cuda.synchronize()
            for _ in range(3):
                graph.replay()
            torch.cuda.synchronize()
            nbytes = moved_bytes(layers, hkv, d, keep, drop, n_pos)
            reps = 200 if n_pos == 4096 else 40
            ms, (lo, hi) = time_ms(graph.replay, reps)
            torch_evict(m, 0, keep, drop, n_pos)
            torch.cuda.synchronize()
            t_ms, _ = time_ms(lambda: torch_evict(m, 0, keep, drop, n_pos), 5, rounds=3)
            rate = nbytes / (ms * 1e-3)
            lines.append(f"| {name} ({layers} x {hkv} x {d}) | {n_pos} | {drop} | {nbytes / 1e6:.1f} | {ms:.4f} ({lo:.4f}-{hi:.4f}) | "
                         f"{rate / 1e12:.2f} | {rate / HBM_PEAK:.1%} | {rate / HBM_ACHIEVABLE:.1%} | {t_ms:.3f} | {t_ms / ms:.1f} x |")
            del m, k, v, graph
            torch.cuda.empty_cache()
    lines += ["", "Bytes are the algorithm's (every moved position of K and V read once and written once), over graph-replay time between "
              "device events (median of 5 windows). At 4096 positions both models' rows fit the 256 MiB Infinity Cache, so replays "
              "there are served on-die; the 32768-position rows (268 MB and 940 MB per cache) are not.", ""]


def measure_session(lines, steps, k=4):
    from src.specdec import SpeculativePipeline

    pipe = SpeculativePipeline(controller="fixed", controller_params={"k": k}, seed=1234)       # the flagship synthetic 3B / 1B pair
    V = pipe.base_lm.vocab_size
    g = torch.Generator().manual_seed(1234)
    short = [torch.randint(4, V - 1, (64,), generator=g).tolist() for _ in range(1)]

    def per_step(**kw):
        t0 = time.time()
        r = pipe.generate_batch(short, max_tokens=steps, do_sample=False, **kw)[0]
        torch.cuda.synchronize()
        m = r["batch_metrics"]
        return m["total_verification_time_ms"] / max(m["total_steps"], 1), m["total_steps"], (time.time() - t0) * 1e3

    per_step()
    per_step(context_window=4096)                     # warm both runtimes (the windowed one has its own caches and captured step)
    rows = {"no window": [], "context_window=4096 (never reached)": []}
    for _ in range(3):                                # alternating
        rows["no window"].append(per_step())
        rows["context_window=4096 (never reached)"].append(per_step(context_window=4096))
    lines += ["## (b) a window that is never reached", "", f"One row, a 64-token prompt, {steps} tokens, K = {k}, the synthetic 3B / 1B pair; "
              "three alternating runs each, ms per step (device time of the session / steps).", "",
              "| run | ms per step (three runs) | steps |", "|---|---|---|"]
    for name, rs in rows.items():
        lines.append(f"| {name} | {', '.join(f'{r[0]:.3f}' for r in rs)} | {rs[0][1]} |")
    lines.append("")
    # (c) rolls at W = 4096: a prompt that starts close to the window, enough tokens for two rolls
    long_prompt = [torch.randint(4, V - 1, (3900,), generator=g).tolist()]
    n_tokens = 2 * 2040 + 400
    pipe.generate_batch(long_prompt, max_tokens=64, do_sample=False, context_window=4096)        # warm-up at this shape
    t0 = time.time()
    r = pipe.generate_batch(long_prompt, max_tokens=n_tokens, do_sample=False, context_window=4096)[0]
    torch.cuda.synchronize()
    wall = (time.time() - t0) * 1e3
    ev = r["evictions"]
    # the cost of one roll of this session, measured on its own engines: both evictions between events
    rt = next(rt for key, rt in pipe._runtimes.items() if "window" in key)
    drop = ev[0][1] if ev else 2040

    def both():
        for e in (rt["target"], rt["draft"]):
            e.evict_row(0, 4, drop, 4060)
    both()
    torch.cuda.synchronize()
    roll_ms, _ = time_ms(both, 20)
    n = len(r["generated_tokens"])
    lines += ["## (c) amortised cost at context_window=4096", "",
              f"One row, a 3900-token prompt, {n} tokens generated in {wall:.0f} ms wall ({wall / n:.3f} ms per token), {len(ev)} rolls of {drop} "
              f"positions at {[g for g, _ in ev]} tokens. One roll (evict_row on both engines at 4060 cached positions, between events): "
              f"{roll_ms:.3f} ms of device time, once per {drop} tokens: {roll_ms / drop * 1e3:.3f} us per generated token "
              f"({roll_ms / drop / (wall / n):.4%} of the time per token). A roll also drains the launch queue: the steps in flight "
              "(at most two) are void for the row and run again.", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rolling_context.md"))
    ap.add_argument("--skip-session", action="store_true")
    ap.add_argument("--steps", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rolling_context_bench needs a GPU")
    lines = ["# Rolling context window: measurements", "",
             f"{torch.cuda.get_device_name(0)}; scripts/rolling_context_bench.py. Nothing here is a gate.", ""]
    measure_evict(lines)
    if not args.skip_session:
        measure_session(lines, args.steps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    main()
