"""Inputs of the recorded-bits test of the vocabulary-row kernels (tests/test_hip_row_kernels_bits_gpu.py), and its recorder.

Every kernel that walks a vocabulary-sized row and reduces over it (csrc/sample.hip, spec_sample.hip, spec_agree.hip,
logit_proc.hip, verify_prefix.hip) takes its walkers, reductions and selection pieces from csrc/common.h and
csrc/sample_device.h. tests/golden/row_kernels_bits.npz holds what each case below returned on the commit BEFORE those pieces
were shared (9ba3408); the test asks for the same bits, so a change to a shared piece that alters any output shows up here
whatever the CPU restatements tolerate.

Inputs come from numpy.random.Generator(PCG64(seed)) alone and are rounded to bf16 / f16 by torch on the CPU, so they are the
same on every machine. The fixture holds outputs only: ids, accept lengths, flags and counters as integers, float64 outputs as
their uint64 bit patterns. The processed rows of the two V = 32000 logit-processor cases are 384 KB each, more than the fixture
may weigh: they are held as the CRC-32 of every complete row plus the first and last 512 words of each as uint16.

    python tests/row_kernel_cases.py --record     # on the GPU, with the library of the commit to record from

Shapes are the smallest at which each shared piece can go wrong; the case functions say which piece. Two remarks on what a
shape reaches, from reading the kernels:
  * topk/const8192: the composite key carries the index, so the thread maxima of a constant row are 1024 different keys and
    the fast path keeps 393 candidates; the row checks "tie at the cut" (50 equal values, lowest ids win), not the radix fallback.
    The fallback is reached by topk/planted65536, which asserts so.
  * agreement V = 4104 has two slices of 2056 and 2048 elements, both whole 8-element chunks; V = 4100 is added for a last
    slice that ends in a 4-element chunk.
"""

import sys
import zlib
from pathlib import Path

import numpy as np
import torch

FIXTURE = Path(__file__).resolve().parent / "golden" / "row_kernels_bits.npz"


def _rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def _t(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dtype)


def _i32(x):
    return torch.from_numpy(np.asarray(x, dtype=np.int32))


def _np(t):
    return t.cpu().numpy()


def _bits64(t):
    return t.cpu().numpy().view(np.uint64)


def _bits16(t):
    return t.cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


# ---------------------------------------------------------------------------------------------------- 1-3: sd_sample_token
def _draws(logits, dev, **kw):
    """three draws of every row: int32 [3][rows]"""
    from specdec_hip.ops import sample_token_hip

    d = logits.to(dev)
    return {"ids": np.stack([_np(sample_token_hip(d, seed=0x1234ABCD5678, draw=j, **kw)) for j in range(3)])}


def _composite_keys(x):
    """csrc/sample_device.h: composite_key of a float32 row (no NaN, no zero)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    okey = np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint64)
    return (okey << np.uint64(20)) | (np.uint64((1 << 20) - 1) - np.arange(x.size, dtype=np.uint64))


def topk_v1000_f32(dev):        # fewer elements than threads; k equals V
    return _draws(_t(_rng(11).normal(0, 3.0, (1, 1000)), torch.float32), dev, temperature=0.8, top_k=1000)


def topk_v4099_f16(dev):        # element walker, odd V
    return _draws(_t(_rng(12).normal(0, 3.0, (1, 4099)), torch.float16), dev, temperature=0.7, top_k=50, top_p=0.9)


def topk_const8192(dev):        # every value equal: the cut is decided by the index half of the key
    return _draws(_t(np.full((1, 8192), 1.5), torch.bfloat16), dev, temperature=1.0, top_k=50, top_p=0.9)


def topk_planted65536(dev):     # thread maxima concentrated in 70 threads: the radix fallback, stopped early
    V, k = 65536, 300
    rng = _rng(14)
    x = rng.normal(0, 0.1, V)
    hot = (np.arange(V) // 8) % 1024 < 70
    x[hot] = rng.uniform(5.0, 8.0, int(hot.sum()))
    row = _t(x[None], torch.bfloat16)
    keys = _composite_keys(row[0].float().numpy())
    thread_max = keys.reshape(V // 8 // 1024, 1024, 8).max(axis=(0, 2))      # vector v = i // 8 belongs to thread v % 1024
    tau = np.sort(thread_max)[::-1][k - 1]
    assert int(hot.sum()) == 4480 and int((keys >= tau).sum()) > 4096, "the fast path must overflow its 4096 candidates"
    return _draws(row, dev, temperature=0.9, top_k=k)


def nucleus_v300(dev):          # one rank block
    return _draws(_t(_rng(21).normal(0, 3.0, (1, 300)), torch.bfloat16), dev, temperature=0.8, top_p=0.9)


def nucleus_v5000_flat(dev):    # several rank blocks, re-walked in phase B
    return _draws(_t(_rng(22).normal(0, 0.2, (1, 5000)), torch.bfloat16), dev, temperature=1.0, top_p=0.6)


def nucleus_inf_on_top(dev):
    x = _rng(23).normal(0, 3.0, (1, 300))
    x[0, 137] = np.inf
    return _draws(_t(x, torch.bfloat16), dev, temperature=0.8, top_p=0.9)


def _with_nan_row(x, at):
    x = np.concatenate([x, x], 0)
    x[1, at] = np.nan
    return x


def gumbel_v50_f32(dev):
    return _draws(_t(_with_nan_row(_rng(31).normal(0, 3.0, (1, 50)), 17), torch.float32), dev, temperature=0.8)


def gumbel_v50257_bf16(dev):
    return _draws(_t(_with_nan_row(_rng(32).normal(0, 3.0, (1, 50257)), 40001), torch.bfloat16), dev, temperature=1.3)


# ------------------------------------------------------------------------------------------ 4-5: sd_spec_sample_accept[_shaped]
def _accept(V, T, dev, seed, top_k=None, top_p=None):
    """B = 2, K = 3. Position (0, 0): q == p bitwise; position (1, 1): a NaN in p; then the same call with row 1 inactive."""
    from specdec_hip.ops import spec_sample_accept_hip

    B, K = 2, 3
    rng = _rng(seed)
    p = _t(rng.normal(0, 3.0, (B, K + 1, V)), torch.bfloat16)
    q = _t(p[:, :K].float().numpy() + rng.normal(0, 0.5, (B, K, V)), torch.bfloat16)
    q[0, 0] = p[0, 0]
    p[1, 1, V // 3] = float("nan")
    ids = q.float().argmax(-1).to(torch.int32)          # in every kept set of q; ...
    ids[:, K - 1] = _i32(rng.integers(0, V, B))         # ... the last position's is anywhere
    out = {}
    for tag, active in (("", None), ("/row1_inactive", [1, 0])):
        ctr = _i32([5, 9]).to(dev)
        acc, nxt, ratios = spec_sample_accept_hip(q.to(dev), p.to(dev), ids.to(dev), T, seed=0xC0FFEE12345, draw_counters=ctr,
                                                  active=None if active is None else _i32(active).to(dev), return_ratios=True,
                                                  top_k=top_k, top_p=top_p)
        out.update({"accept" + tag: _np(acc), "next" + tag: _np(nxt), "ratios" + tag: _bits64(ratios), "counters" + tag: _np(ctr)})
    return out


def _accept_case(V, T, seed, **kw):
    return lambda dev: _accept(V, T, dev, seed, **kw)


# ---------------------------------------------------------------------------------------------------- 6: sd_spec_agreement
def _agreement(V, T, dev, seed):
    """n = 3, a tied maximum in row 1; then the same rows through views offset by one element (the element-load path)"""
    from specdec_hip.ops import spec_agreement

    n = 3
    rng = _rng(seed)
    p = rng.normal(0, 3.0, (n, V))
    q = p + rng.normal(0, 0.5, (n, V))
    p[1, [V // 5, V - 3]] = 17.0
    p, q = _t(p, torch.bfloat16), _t(q, torch.bfloat16)
    out = {}
    for tag, off in (("", 0), ("@offset", 1)):
        bufs = [torch.zeros(n * V + 8, dtype=torch.bfloat16, device=dev) for _ in range(2)]
        views = [b[off:off + n * V].view(n, V) for b in bufs]
        views[0].copy_(p)
        views[1].copy_(q)
        alpha, kl, agree, p_arg, q_arg = spec_agreement(views[1], views[0], T)
        out.update({"alpha" + tag: _bits64(alpha), "kl" + tag: _bits64(kl), "agree" + tag: _np(agree).astype(np.uint8),
                    "p_arg" + tag: _np(p_arg), "q_arg" + tag: _np(q_arg)})
    return out


def _agreement_case(V, T, seed):
    return lambda dev: _agreement(V, T, dev, seed)


# ----------------------------------------------------------------------------------------------- 7: sd_logit_process[_fsm]
def _row_digest(rows):
    """uint16 [B][R][V] -> the CRC-32 of each row, and its first and last 512 words"""
    flat = rows.reshape(-1, rows.shape[-1])
    crc = np.array([zlib.crc32(np.ascontiguousarray(r).tobytes()) for r in flat], dtype=np.uint32)
    return {"rows_crc": crc, "rows_head": flat[:, :512].copy(), "rows_tail": flat[:, -512:].copy()}


def _logit_process(V, dev, seed, with_bias, fsm, keep_rows):
    """B = 2, R = 3 (row r conditioned on r in-step tokens), ids out; then the same call with row 1 inactive"""
    from specdec_hip.ops import fsm_build_masks, logit_process, logit_process_fsm

    B, R = 2, 3
    rng = _rng(seed)
    rows = _t(rng.normal(0, 3.0, (B, R, V)), torch.bfloat16)
    counts = np.where(rng.random((B, V)) < 0.05, rng.integers(1, 4, (B, V)), 0).astype(np.uint16)
    counts |= np.where(rng.random((B, V)) < 0.03, 0x8000, 0).astype(np.uint16)
    counts = torch.from_numpy(counts.view(np.int16))
    bias = _t(rng.normal(0, 1.0, (B, V)), torch.float32) if with_bias else None
    toks = rows[:, :R - 1].float().argmax(-1).to(torch.int32)      # penalising these moves the argmax of the later rows
    kw = dict(repetition_penalty=1.3, presence_penalty=0.5, frequency_penalty=0.2, bias=None if bias is None else bias.to(dev),
              tokens=toks.to(dev), return_ids=True)
    if fsm:     # 3 states; about a quarter of the tokens not allowed; row 0 starts in state 0, row 1 in state 2
        nxt = np.where(rng.random((3, V)) < 0.25, 0xFFFF, rng.integers(0, 3, (3, V))).astype(np.uint16)
        d_nxt = torch.from_numpy(nxt.view(np.int16)).to(dev)
        d_allow, d_state = fsm_build_masks(d_nxt), _i32([0, 2]).to(dev)
    out = {}
    for tag, active in (("", None), ("/row1_inactive", [1, 0])):
        d_rows = rows.to(dev)
        kw["active"] = None if active is None else _i32(active).to(dev)
        if fsm:
            ids = logit_process_fsm(d_rows, counts.to(dev), d_nxt, d_allow, d_state, 2, **kw)
        else:
            ids = logit_process(d_rows, counts.to(dev), **kw)
        out["ids" + tag] = _np(ids)
        if keep_rows:
            out.update({k + tag: v for k, v in _row_digest(_bits16(d_rows)).items()})
    return out


# ------------------------------------------------------------------------------------------------------ 8: sd_verify_prefix
def _verify_prefix(dtype, dev):
    """B = 2, K = 4, V = 50257. A row is cut into 7 (bf16) / 13 (fp32) chunks of 7184 / 3868 elements: the maximum is tied across
    the first chunk boundary of either layout in rows (0, 1) and (1, 2); row (1, 0) holds a NaN, the maximum of its row."""
    from specdec_hip.ops import verify_prefix_hip

    B, K, V = 2, 4, 50257
    x = _rng(81).normal(0, 3.0, (B, K, V))
    x[0, 1, [7183, 7184]] = 19.0
    x[1, 2, [3867, 3868, 30000]] = 19.0
    x[1, 0, 12345] = np.nan
    logits = _t(x, dtype)
    ids = logits.float().argmax(-1).to(torch.int32)
    ids[0, 3] += 1
    ids[1, 1] += 1
    acc, mask, pred = verify_prefix_hip(logits.to(dev), ids.to(dev), return_pred=True)
    return {"accept": _np(acc), "mask": _np(mask), "pred": _np(pred)}


CASES = {
    "topk/v1000_f32_k_is_V": topk_v1000_f32,
    "topk/v4099_f16": topk_v4099_f16,
    "topk/const8192": topk_const8192,
    "topk/planted65536": topk_planted65536,
    "nucleus/v300": nucleus_v300,
    "nucleus/v5000_flat": nucleus_v5000_flat,
    "nucleus/inf_on_top": nucleus_inf_on_top,
    "gumbel/v50_f32": gumbel_v50_f32,
    "gumbel/v50257_bf16": gumbel_v50257_bf16,
    "accept/v32000_T1": _accept_case(32000, 1.0, 41),
    "accept/v32000_T0.7": _accept_case(32000, 0.7, 42),
    "accept/v50257_T1": _accept_case(50257, 1.0, 43),
    "accept/v50257_T0.7": _accept_case(50257, 0.7, 44),
    "accept_shaped/v32000_k50_p0.9": _accept_case(32000, 0.8, 51, top_k=50, top_p=0.9),
    "accept_shaped/v1000_k1024": _accept_case(1000, 0.8, 52, top_k=1024),
    "agreement/v4104_T1": _agreement_case(4104, 1.0, 61),
    "agreement/v4104_T0.7": _agreement_case(4104, 0.7, 62),
    "agreement/v4100_T1": _agreement_case(4100, 1.0, 65),
    "agreement/v50257_T1": _agreement_case(50257, 1.0, 63),
    "agreement/v50257_T0.7": _agreement_case(50257, 0.7, 64),
    "logit_process/v32000_bias": lambda dev: _logit_process(32000, dev, 71, True, False, True),
    "logit_process/v50257": lambda dev: _logit_process(50257, dev, 72, False, False, False),
    "logit_process/v32000_fsm": lambda dev: _logit_process(32000, dev, 71, True, True, True),
    "verify_prefix/bf16": lambda dev: _verify_prefix(torch.bfloat16, dev),
    "verify_prefix/f32": lambda dev: _verify_prefix(torch.float32, dev),
}


def run_case(name, dev="cuda"):
    """{fixture key: array} of one case"""
    return {f"{name}:{k}": v for k, v in CASES[name](dev).items()}


if __name__ == "__main__":
    if sys.argv[1:] != ["--record"]:
        sys.exit(__doc__)
    root = Path(__file__).resolve().parents[1]
    sys.path[:0] = [str(root / "llm-inference-lab_amd"), str(root)]
    recorded = {}
    for case in CASES:
        recorded.update(run_case(case))
    torch.cuda.synchronize()
    FIXTURE.parent.mkdir(exist_ok=True)
    np.savez_compressed(FIXTURE, **recorded)
    print(f"recorded {len(recorded)} arrays of {len(CASES)} cases: {FIXTURE} ({FIXTURE.stat().st_size} bytes)")
