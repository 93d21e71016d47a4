"""One case of tests/gemm_body_cases.py on the GPU: the pass, its plan, the fp64 stage checks of tests/test_hip_stage_fp64_gpu.py
and the checks only these cases make (fused argmax, untouched cache outside the new positions, cross-layer statistics).

Imported by tests/test_hip_gemm_bodies_gpu.py, and run as a program by its knob driver:

    python tests/gemm_body_run.py FLAGS

runs every KNOB_CASES entry with that `flags` value in this process — which must have been started with the matching
SPECDEC_NO_DIRECT / SPECDEC_NO_PIPE environment, read once per process by the library — and prints one JSON line
{"cases": {id: {stage: worst error / bound}}, "worst": {stage: ...}}."""

import dataclasses
import json
import os
import random
import sys

if __name__ == "__main__":   # as a program: the import paths tests/conftest.py gives the suite
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_root, "llm-inference-lab_amd"), _root):
        if _p not in sys.path:
            sys.path.insert(0, _p)

import torch

import gemm_body_cases as G
import stage_ref as R
from specdec_hip import _abi
from specdec_hip.engine import _stream
from test_hip_stage_fp64_gpu import _check_pass, _engine, _matrices, _weights, _write_prefix

CANARY = 0x3F9D        # bf16 1.2265625: finite (masked keys are still multiplied) and not a value a kernel would store by chance
IDS_SENTINEL = -7


def _fill_canary(eng):
    k, v = eng.kv_view()
    k.view(torch.int16).fill_(CANARY)
    v.view(torch.int16).fill_(CANARY)


def _changed(eng, snap_k, snap_v):
    """positions whose K or V bits differ from the snapshot, any layer / head / channel: dense [B][Lmax], paged [n_pages][P]"""
    k, v = eng.kv_view()
    dk = (k.view(torch.int16) != snap_k.view(torch.int16))
    dv = (v.view(torch.int16) != snap_v.view(torch.int16))
    return dk.any(4).any(2).any(0), dv.any(3).any(2).any(0)      # K [L][.][Hkv][pos][D], V [L][.][Hkv][D][pos]


def _written_mask(eng, case):
    """the positions the pass may write: [pos_base[b], pos_base[b] + M) of rows row0 .. row0 + B - 1"""
    if eng.page_len is None:
        mask = torch.zeros(eng.batch, eng.l_max, dtype=torch.bool, device=eng.device)
        for b, p0 in enumerate(case.bases):
            mask[case.row0 + b, p0:p0 + case.M] = True
        return mask
    P = eng.page_len
    mask = torch.zeros(eng.n_pages, P, dtype=torch.bool, device=eng.device)
    table = eng.block_table.cpu()
    for b, p0 in enumerate(case.bases):
        for pos in range(p0, p0 + case.M):
            mask[int(table[case.row0 + b, pos // P]), pos % P] = True
    return mask


def _forward(eng, case, tok, pos_base, ids_stride):
    """sd_model_forward with an ids row stride of its own (HipModel.forward always passes M) -> (ids [B][ids_stride], logits)"""
    B, M = tok.shape
    if eng.page_len is not None:
        for b, p0 in enumerate(case.bases):
            eng.reserve(case.row0 + b, p0 + M)
    ids = torch.full((B, ids_stride), IDS_SENTINEL, dtype=torch.int32, device=eng.device)
    logits = torch.empty((B, M, eng.cfg.vocab), dtype=torch.float32, device=eng.device)
    with torch.cuda.device(eng.device):
        rc = eng.lib.sd_model_forward(eng.handle, tok.data_ptr(), M, pos_base.data_ptr(), 0, case.row0, B, M, ids.data_ptr(), ids_stride,
                                      logits.data_ptr(), _abi.SD_F32, 0, _stream(None, eng.device))
    _abi.check(rc, "sd_model_forward")
    return ids, logits


def _first_argmax(logits):
    """argmax over the last dimension, the lowest index on ties"""
    V = logits.shape[-1]
    top = logits.amax(-1, keepdim=True)
    idx = torch.arange(V, device=logits.device).expand_as(logits)
    return torch.where(logits == top, idx, torch.full_like(idx, V)).amin(-1)


def _planned_bodies(eng, case):
    """the knobs of this process must be the ones the case was planned under, and the plan the one the case list recorded"""
    T = case.T
    assert eng.pass_plan(T) == case.names() == eng.pass_plan(T, case.flags), (case.id, eng.pass_plan(T), case.names())


def run_case(case: G.Case, check_plan=_planned_bodies):
    """-> {stage: worst error / bound}; raises AssertionError on any failed check. check_plan(engine, case): the assertion that
    the kernels the engine is about to run are the ones the case records (tests/test_hip_gemv_instances_gpu.py passes its own)"""
    cfg, wd, B, M, T = case.cfg, case.wd, case.B, case.M, case.T
    what = case.id
    mw = _weights(cfg)
    l_max = max(case.bases) + M + 64
    eng = _engine(mw, case.row0 + B + 1, l_max, wd, page_len=case.page_len)       # one cache row more than the pass uses
    eng.set_persist_tokens(0)
    assert T <= eng.pass_tokens, (what, T, eng.pass_tokens)                          # one pass
    check_plan(eng, case)
    if case.page_len is not None:
        random.Random(T).shuffle(eng._free)                                           # pages handed out in a scrambled order
    gen = torch.Generator(device="cuda").manual_seed(1000 * T + case.row0)
    _fill_canary(eng)
    for b, p0 in enumerate(case.bases):
        _write_prefix(eng, case.row0 + b, p0, gen, spikes=(p0 - 1, 31, 32))
    tok = torch.randint(4, cfg.vocab, (B, M), generator=gen, device="cuda", dtype=torch.int32)
    pos_base = torch.tensor(case.bases, dtype=torch.int32, device="cuda")
    if case.page_len is not None:                                                      # the new positions' pages, before the snapshot
        for b, p0 in enumerate(case.bases):
            eng.reserve(case.row0 + b, p0 + M)
    k, v = eng.kv_view()
    snap_k, snap_v = k.clone(), v.clone()
    ids_stride = M if B == 1 else M + 3
    ids, logits = _forward(eng, case, tok, pos_base, ids_stride)

    positions = torch.tensor([p + m for p in case.bases for m in range(M)], device="cuda")
    rows = torch.tensor([case.row0 + b for b in range(B) for _ in range(M)])
    if not case.two_layer:
        res = _check_pass(eng, mw, _matrices(mw, wd), tok.reshape(-1).long(), positions, rows, logits.reshape(T, -1), R.chain_hip, what)
    else:
        # The taps are the last layer's. The same tokens through a one-layer engine over layer 0's weights leave, as its hidden
        # rows, the exact bf16 rows that enter layer 1 here (same kernels, same inputs); layer 1 is then checked from them. Its
        # QKV launch normalises with the statistics that layer 0's down-projection published.
        assert cfg.n_layers == 2 and B == 1 and case.bases == (0,) and case.page_len is None
        mw0 = dataclasses.replace(mw, config=dataclasses.replace(cfg, n_layers=1, name=cfg.name + "-layer0"), layers=[mw.layers[0]], meta={})
        e0 = _engine(mw0, 1, l_max, wd)
        e0.set_persist_tokens(0)
        check_plan(e0, case)
        e0.forward(tok, pos_base, skip_head=True)
        x_in = e0.hidden_rows(T)
        res = _check_pass(eng, mw, _matrices(mw, wd, layer=1), tok.reshape(-1).long(), positions, rows, logits.reshape(T, -1), R.chain_hip,
                          what, layer=1, x_in=x_in)

    # fused argmax: the ids of the launch that stored these logits, at the caller's row stride
    want = _first_argmax(logits).to(torch.int32)
    assert torch.equal(ids[:, :M], want), f"{what}: fused argmax differs from the stored logits at {(ids[:, :M] != want).nonzero().tolist()[:8]}"
    assert bool((ids[:, M:] == IDS_SENTINEL).all()), f"{what}: ids written past M of a row"

    # nothing but the new positions of the used rows changed: the extra row, the other rows, the prefixes, (paged) the free pages
    mask = _written_mask(eng, case)
    ck, cv = _changed(eng, snap_k, snap_v)
    assert not bool((ck & ~mask).any()), f"{what}: K written outside the pass's positions at {(ck & ~mask).nonzero().tolist()[:8]}"
    assert not bool((cv & ~mask).any()), f"{what}: V written outside the pass's positions at {(cv & ~mask).nonzero().tolist()[:8]}"
    assert bool(ck[mask].all()) and bool(cv[mask].all()), f"{what}: a new position kept the canary"
    return res


def _main(flags: int) -> int:
    want = {G.PLAN_NO_DIRECT: "SPECDEC_NO_DIRECT", G.PLAN_NO_PIPE: "SPECDEC_NO_PIPE"}
    for bit, var in want.items():
        assert (var in os.environ) == bool(flags & bit), f"{var} does not match flags={flags}"
    out, worst = {}, {}
    for case in sorted((c for c in G.KNOB_CASES if c.flags == flags), key=lambda c: c.model):
        res = run_case(case)
        out[case.id] = res
        for k, r in res.items():
            worst[k] = max(worst.get(k, 0.0), r)
    torch.cuda.synchronize()
    print(json.dumps({"flags": flags, "cases": out, "worst": worst}))
    return 0


if __name__ == "__main__":
    sys.exit(_main(int(sys.argv[1])))
