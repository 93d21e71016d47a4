"""Inputs and call protocols shared by the self-drafting tests (tests/test_selfdraft_bounds.py on the CPU emulations,
tests/test_hip_selfdraft_fp64_gpu.py on the kernels): test infrastructure, no conftest."""

import torch

import stage_ref as R


def random_heads(n, V, d, seed, device="cpu"):
    """N(0, 0.02) heads, every row of every head at a magnitude of its own (2^U(-2, 2)): no two heads share row scales"""
    g = torch.Generator(device=device).manual_seed(seed)
    out = torch.empty(n, V, d, dtype=torch.bfloat16, device=device)
    for j in range(n):      # one head at a time: a full-vocabulary head is 1 GiB in float32
        h = torch.randn(V, d, generator=g, device=device) * 0.02
        out[j] = (h * torch.exp2(torch.rand(V, 1, generator=g, device=device) * 4 - 2)).bfloat16()
    return out


def hidden_rows(n, d, seed, device="cpu"):
    """residual rows ~ N(0, 0.8) (N(0, 0.02) embeddings grown by a stack of layers), no structure"""
    return (torch.randn(n, d, generator=torch.Generator(device=device).manual_seed(seed), device=device) * 0.8).bfloat16()


def eagle_protocol(run, x, prev, has_prev, w, b, eps, alpha, K, rms, what):
    """the two calls of the GPU test: has_prev = 0 over garbage state exposes h_t (row 0), checked against the fp64 norm; then
    the call under test, checked bit for bit from that h_t. `run`: the kernel or its emulation. -> check_eagle_norm's (flips, worst share of the allowed error)"""
    B = x.shape[0]
    garbage = (prev.float() * 3 + 1).bfloat16()
    H0, e0, f0 = run(x, garbage, torch.zeros(B, dtype=torch.int32, device=x.device), w, b, eps, alpha, K, rms)
    h_t = H0[:, 0].contiguous()
    res = R.check_eagle_norm(h_t, x, w, b, eps, rms, f"{what}: norm")
    R.check_eagle_exact(H0, e0, f0, h_t, garbage, torch.zeros(B, dtype=torch.int32, device=x.device), alpha, f"{what}: first step")
    H, e, f = run(x, prev, has_prev, w, b, eps, alpha, K, rms)
    R.check_eagle_exact(H, e, f, h_t, prev, has_prev, alpha, what)
    return res


def eagle_inputs(B, d, seed, form="plain", device="cpu"):
    """(x, prev, w, b): residual rows in one of three forms — plain N(0, 1); a few channels x 100 (the massive activations
    trained decoders carry); a common offset of 8 standard deviations (a CHOICE: nobody has measured what the residual rows
    of real checkpoints carry; it is where a one-pass variance loses digits) — random state rows, norm weights 1 + N(0, 0.1)
    and offsets N(0, 0.1)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, d, generator=g)
    if form == "spikes":
        x[:, torch.randperm(d, generator=g)[:3]] *= 100
    elif form == "offset":
        x = x + 8.0
    prev = torch.randn(B, d, generator=g)
    w = 1 + 0.1 * torch.randn(d, generator=g)
    b = 0.1 * torch.randn(d, generator=g)
    return tuple(t.bfloat16().to(device) for t in (x, prev, w, b))
