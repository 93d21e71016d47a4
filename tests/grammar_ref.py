"""CPU restatement of csrc/grammar.hip and of the grammar line of csrc/logit_proc.hip (the contract is in include/specdec_hip.h
at sd_logit_process_fsm): the mask table, the walk over in-step tokens, the advance after a step, and the transform of a row —
logit_proc_ref.process_row followed by the mask. Integers and bf16 words throughout: the device must reproduce them exactly.

A state is -1 (unconstrained), 0..S-1, or DEAD (stored as 0xFFFF; any value >= S reads as DEAD)."""

import numpy as np

import logit_proc_ref as L

NONE = 0xFFFF
DEAD = 0xFFFF
NEG_INF_BF16 = 0xFF80


def build_masks(nxt):
    """next uint16 [S][V] -> uint32 [S][ceil(V / 32)]: bit v % 32 of word v / 32 = next[s][v] != 0xFFFF, pad bits 0"""
    nxt = np.asarray(nxt, dtype=np.uint16)
    S, V = nxt.shape
    W = (V + 31) // 32
    bits = np.zeros((S, W * 32), dtype=np.uint64)
    bits[:, :V] = nxt != NONE
    return (bits.reshape(S, W, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def step(nxt, s, tok):
    S, V = nxt.shape
    s = int(s)
    if s < 0:
        return -1
    if s >= S or not 0 <= int(tok) < V:
        return DEAD
    n = int(nxt[s, int(tok)])
    return DEAD if n >= S else n


def walk(nxt, s, tokens):
    s = int(s)
    if s >= nxt.shape[0]:
        s = DEAD
    for t in tokens:
        s = step(nxt, s, t)
    return s


def advance(nxt, state, tokens, n_new, active=None):
    """state int [B] -> a new vector: every active row with a state >= 0 walks its first n_new[b] tokens"""
    out = [int(s) for s in state]
    for b in range(len(out)):
        if (active is not None and not active[b]) or out[b] < 0:
            continue
        n = max(0, min(int(n_new[b]), len(tokens[b])))
        out[b] = walk(nxt, out[b], tokens[b][:n])
    return np.array(out, dtype=np.int64)


def allowed_row(nxt, s, eos_id):
    """bool [V]: what state s allows (everything at -1, eos alone in DEAD)"""
    S, V = nxt.shape
    if s < 0:
        return np.ones(V, dtype=bool)
    if s >= S:
        m = np.zeros(V, dtype=bool)
        m[eos_id] = True
        return m
    return nxt[s] != NONE


def process_row_fsm(row_bits, counts_row, nxt, state, eos_id, in_step=(), rp=1.0, presence=0.0, frequency=0.0, bias_row=None):
    """the processors' row, then the mask of walk(state, in_step): a disallowed element is -inf, whatever it was (a NaN too)"""
    out = L.process_row(row_bits, counts_row, in_step, rp, presence, frequency, bias_row)
    if int(state) < 0:
        return out
    ok = allowed_row(nxt, walk(nxt, state, in_step), eos_id)
    return np.where(ok, out, np.uint16(NEG_INF_BF16)).astype(np.uint16)


def process_rows_fsm(rows_bits, counts, nxt, state, eos_id, tokens=None, n_tokens=None, rp=1.0, presence=0.0, frequency=0.0, bias=None,
                     active=None):
    """logit_proc_ref.process_rows with the mask line -> (processed uint16 [B][R][V], ids int [B][R])"""
    rows_bits = np.asarray(rows_bits, dtype=np.uint16)
    B, R, V = rows_bits.shape
    out = rows_bits.copy()
    ids = np.zeros((B, R), dtype=np.int64)
    for b in range(B):
        for r in range(R):
            if active is None or active[b]:
                n = r if n_tokens is None else n_tokens
                toks = [] if tokens is None else [int(t) for t in tokens[b][:n]]
                out[b, r] = process_row_fsm(rows_bits[b, r], counts[b], nxt, state[b], eos_id, toks, rp, presence, frequency,
                                            None if bias is None else bias[b])
            ids[b, r] = L.argmax_bits(out[b, r])
    return out, ids
