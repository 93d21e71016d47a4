"""CPU restatement of csrc/logit_proc.hip (the contract is in include/specdec_hip.h at sd_logit_process): the transform of one
stored bf16 logits row, the argmax rule of its fused output, and the two count updates. numpy float32 throughout — every line
of the formula is one IEEE float32 operation, which numpy rounds correctly, so the device must reproduce these bits.

A row is carried as the uint16 words of its bf16 values; counts as uint16 words (bit 15: the token occurs in the row's prompt,
bits 0..14: times generated, saturating at 32767)."""

import numpy as np

PROMPT_BIT = 0x8000
COUNT_MASK = 0x7FFF
NAN_BF16 = 0x7FC0


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def f32_to_bf16(x):
    """round to nearest even; a NaN becomes 0x7fc0"""
    x = np.asarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    r = ((u + np.uint32(0x7FFF) + ((u >> 16) & np.uint32(1))) >> 16).astype(np.uint16)   # (uint32 wrap-around cannot occur below NaN)
    return np.where(np.isnan(x), np.uint16(NAN_BF16), r).astype(np.uint16)


def process_row(row_bits, counts_row, in_step=(), rp=1.0, presence=0.0, frequency=0.0, bias_row=None):
    """row_bits uint16 [V], counts_row uint16 [V], in_step: the tokens t_1..t_i this row is conditioned on -> uint16 [V]"""
    V = len(row_bits)
    rp, presence, frequency = np.float32(rp), np.float32(presence), np.float32(frequency)
    x = bf16_to_f32(row_bits).copy()
    cw = np.asarray(counts_row, dtype=np.uint16)
    c = (cw & COUNT_MASK).astype(np.int64)
    for t in in_step:
        if 0 <= int(t) < V:
            c[int(t)] += 1
    seen = ((cw & PROMPT_BIT) != 0) | (c > 0)
    with np.errstate(all="ignore"):
        if rp != np.float32(1.0):
            x = np.where(seen, np.where(x < 0, x * rp, x / rp), x).astype(np.float32)
        gen = c > 0
        x = np.where(gen, x - presence, x).astype(np.float32)
        prod = (frequency * c.astype(np.float32)).astype(np.float32)
        x = np.where(gen, x - prod, x).astype(np.float32)
        if bias_row is not None:
            x = (x + np.asarray(bias_row, dtype=np.float32)).astype(np.float32)
    return f32_to_bf16(x)


def argmax_bits(row_bits):
    """the fused lm_head argmax rule: a NaN is the maximum, then the larger value; ties and several NaNs: the lowest index"""
    x = bf16_to_f32(row_bits)
    nan = np.isnan(x)
    if nan.any():
        return int(np.argmax(nan))
    return int(np.argmax(x))


def process_rows(rows_bits, counts, tokens=None, n_tokens=None, rp=1.0, presence=0.0, frequency=0.0, bias=None, active=None):
    """rows_bits uint16 [B][R][V]; tokens int [B][n]; n_tokens None: row (b, r) uses the first r tokens, else the first n_tokens.
    -> (processed uint16 [B][R][V], ids int [B][R]); rows of an inactive b are returned as they are, with their own argmax"""
    rows_bits = np.asarray(rows_bits, dtype=np.uint16)
    B, R, V = rows_bits.shape
    out = rows_bits.copy()
    ids = np.zeros((B, R), dtype=np.int64)
    for b in range(B):
        for r in range(R):
            if active is None or active[b]:
                n = r if n_tokens is None else n_tokens
                toks = [] if tokens is None else [int(t) for t in tokens[b][:n]]
                out[b, r] = process_row(rows_bits[b, r], counts[b], toks, rp, presence, frequency, None if bias is None else bias[b])
            ids[b, r] = argmax_bits(out[b, r])
    return out, ids


def counts_set(V, prompt_ids, generated_ids=()):
    row = np.zeros(V, dtype=np.uint16)
    for t in prompt_ids:
        if 0 <= int(t) < V:
            row[int(t)] = PROMPT_BIT
    for t in generated_ids:
        if 0 <= int(t) < V and (row[int(t)] & COUNT_MASK) != COUNT_MASK:
            row[int(t)] += 1
    return row


def counts_add(counts, tokens, n_new, active=None):
    """counts uint16 [B][V] -> a new table with row b's first n_new[b] tokens counted (inactive rows unchanged)"""
    out = np.asarray(counts, dtype=np.uint16).copy()
    B, V = out.shape
    for b in range(B):
        if active is not None and not active[b]:
            continue
        n = max(0, min(int(n_new[b]), len(tokens[b])))
        for t in tokens[b][:n]:
            if 0 <= int(t) < V and (out[b, int(t)] & COUNT_MASK) != COUNT_MASK:
                out[b, int(t)] += 1
    return out
