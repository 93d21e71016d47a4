"""The native prefill GEMM (csrc/prefill_mfma.hip) alone at the 3B matrix shapes — run under `rocprofv3 --kernel-trace --stats`:
`python profiles/tools/prefill_native_kernel.py [--weight-dtype bf16|fp8] [--tokens 512] [--iters 5]`. A 2-layer model of Llama-3.2-3B
dimensions absorbs one prompt of `tokens` positions `iters` times with SD_PREFILL_NATIVE; the kernel statistics then hold
2 * iters launches of each of the four matrix products (qkv, out, gate / up, down). Prints the FLOPs per prompt for the TFLOP/s figure."""
import argparse
import dataclasses
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "llm-inference-lab_amd"))
import torch  # noqa: E402

from specdec_hip import weights as W  # noqa: E402
from specdec_hip.engine import HipModel  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--weight-dtype", default="bf16", choices=["bf16", "fp8"])
ap.add_argument("--tokens", type=int, default=512)
ap.add_argument("--iters", type=int, default=5)
args = ap.parse_args()
cfg = dataclasses.replace(W.LLAMA_3_2_3B, n_layers=2, vocab=32000)
mw = W.random_init(cfg, seed=11, device="cuda")
hm = HipModel(mw, batch=1, l_max=args.tokens + 64, weight_dtype=args.weight_dtype, prefill_backend="native")
toks = torch.randint(4, cfg.vocab, (1, args.tokens), dtype=torch.int32, device="cuda")
zero = torch.zeros(1, dtype=torch.int32, device="cuda")
for _ in range(args.iters):
    hm.forward(toks, zero, 0, skip_head=True)
torch.cuda.synchronize()
d, ff, hqd, nqkv = cfg.d_model, cfg.d_ff, cfg.n_heads * cfg.head_dim, (cfg.n_heads + 2 * cfg.n_kv_heads) * cfg.head_dim
per_layer = {"qkv": nqkv * d, "out": d * hqd, "gate/up": 2 * ff * d, "down": d * ff}
print({"weight_dtype": args.weight_dtype, "tokens": args.tokens, "launches_per_matrix": cfg.n_layers * args.iters,
       "gflop_per_launch": {k: round(2.0 * v * args.tokens / 1e9, 3) for k, v in per_layer.items()},
       "prefill_counts": hm.prefill_counts()})
