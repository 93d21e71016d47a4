"""One case of tests/persist_cases.py on the GPU: the pass on the persistent launch, its plan, the fp64 stage checks of
tests/test_hip_stage_fp64_gpu.py (`_check_pass`) and the checks every case makes besides: health word, fused argmax at the
caller's ids stride, and a cache in which nothing but the pass's new positions changed, in any layer.

Deep models are checked at their LAST layer from `x_in`, the hidden rows of an engine over the first n - 1 layers run on the same
path with the same tokens. That rests on the launch being bit-reproducible, which `run_deep` asserts first."""

import dataclasses

import torch

import persist_cases as P
import stage_ref as R
from gemm_body_run import IDS_SENTINEL, _fill_canary, _first_argmax, _forward, _written_mask
from test_hip_stage_fp64_gpu import _check_pass, _engine, _matrices, _weights, _write_prefix

_ENGINES = {}


def bind(mw, batch, l_max, fresh=True):
    """an engine at the largest token count the persistent launch takes for the model. A cache whose rows are not whole 32-key
    blocks (HipModel rounds up: the launch path's attention walks whole blocks) is bound again at its exact size."""
    key = (mw.config.name, batch, l_max)
    if not fresh and key in _ENGINES:
        return _ENGINES[key]
    eng = _engine(mw, batch, l_max)
    if eng.l_max != l_max:
        assert l_max % 8 == 0
        eng.l_max = l_max
        eng._bind_dense()
    eng.set_persist_tokens(8)
    if not fresh:
        if mw.config.d_model >= 2048:
            _ENGINES.clear()          # one large model's engines at a time
        _ENGINES[key] = eng
    return eng


def shallower(mw):
    """the same weights without the last layer (its own packed copy)"""
    c = mw.config
    return dataclasses.replace(mw, config=dataclasses.replace(c, n_layers=c.n_layers - 1, name=f"{c.name}-first{c.n_layers - 1}"),
                               layers=mw.layers[:-1], meta={})


def prepare(eng, case, seed=0):
    """canary everywhere, the case's prefixes in every layer, tokens -> (tok [B][M], pos_base [B], snapshot of K, of V)"""
    cfg, B, M = case.cfg, case.B, case.M
    gen = torch.Generator(device="cuda").manual_seed(7919 * case.T + 31 * case.bases[0] + case.row0 + seed)
    _fill_canary(eng)
    k, v = eng.kv_view()
    for b, p0 in enumerate(case.bases):
        row = case.row0 + b
        if case.prefix == "stale":       # x 256 V at every stale position behind the prefix: the new ones and the 64 after them
            n = min(eng.l_max, p0 + M + 64)
            _write_prefix(eng, row, n, gen, spikes=tuple(range(p0, n)))
        else:
            n = p0
            _write_prefix(eng, row, n, gen, peaked=case.prefix == "peaked", spikes=(p0 - 1, 31, 32))
        if n > 0 and cfg.n_layers > 1:   # (_write_prefix fills layer 0)
            k[1:, row, :, :n] = k[0, row, :, :n]
            v[1:, row, :, :, :n] = v[0, row, :, :, :n]
    tok = torch.randint(4, cfg.vocab, (B, M), generator=gen, device="cuda", dtype=torch.int32)
    pos_base = torch.tensor(case.bases, dtype=torch.int32, device="cuda")
    return tok, pos_base, k.clone(), v.clone()


def check_cache(eng, case, snap_k, snap_v, what):
    """no K / V bit outside the pass's new positions changed in any layer, row or head, and every new position did, in every layer"""
    k, v = eng.kv_view()
    ck = (k.view(torch.int16) != snap_k.view(torch.int16)).any(4).any(2)      # [L][B][pos]
    cv = (v.view(torch.int16) != snap_v.view(torch.int16)).any(3).any(2)
    mask = _written_mask(eng, case)
    assert not bool((ck & ~mask).any()), f"{what}: K written outside the pass's positions at {(ck & ~mask).nonzero().tolist()[:8]}"
    assert not bool((cv & ~mask).any()), f"{what}: V written outside the pass's positions at {(cv & ~mask).nonzero().tolist()[:8]}"
    assert bool(ck[:, mask].all()) and bool(cv[:, mask].all()), f"{what}: a new position kept the canary"


def check_ids(case, ids, logits, what):
    """the fused ids are the first argmax of the stored fp32 logits, at the caller's stride, and nothing is written past M"""
    want = _first_argmax(logits).to(torch.int32)
    assert torch.equal(ids[:, :case.M], want), f"{what}: fused argmax differs from the stored logits at {(ids[:, :case.M] != want).nonzero().tolist()[:8]}"
    assert bool((ids[:, case.M:] == IDS_SENTINEL).all()), f"{what}: ids written past M of a row"


def run_pass(eng, case, persistent=True, seed=0, skip_head=False):
    """the case's pass on `eng` -> (tok, ids, logits); the common checks that need no reference"""
    what = case.id
    T, M, B = case.T, case.M, case.B
    if persistent:
        cap = eng.persist_plan().max_tokens
        assert eng.persist_tokens == cap and T <= cap, (what, eng.persist_tokens, cap)
        assert eng.persist_active(T), what
        assert eng.persist_plan(T).name == P.plan(eng.cfg, T).name != "none", (what, eng.persist_plan(T))
    tok, pos_base, snap_k, snap_v = prepare(eng, case, seed)
    if skip_head:
        eng.forward(tok, pos_base, skip_head=True, row0=case.row0)
        ids = logits = None
    else:
        ids, logits = _forward(eng, case, tok, pos_base, M if B == 1 else M + 3)
        check_ids(case, ids, logits, what)
    assert eng.engine_status() == 0, f"{what}: the launch gave up (status {eng.engine_status():#x})"
    check_cache(eng, case, snap_k, snap_v, what)
    return tok, ids, logits


def _where(case):
    positions = torch.tensor([p + m for p in case.bases for m in range(case.M)], device="cuda")
    rows = torch.tensor([case.row0 + b for b in range(case.B) for _ in range(case.M)])
    return positions, rows


def run_case(case, persistent=True):
    """a one-layer case -> ({stage: worst error / bound}, the engine, (tok, ids, logits)). persistent = False: a pass the engine must route to the launch path; it
    is run with the stage-row stores of the persistent launch switched off, so that rows that pass the stage checks can only
    be the launch path's."""
    assert case.cfg.n_layers == 1
    mw = _weights(case.cfg)
    eng = bind(mw, case.row0 + case.B + 1, case.l_max, fresh=False)                  # one cache row more than the pass uses
    eng.set_persist_taps(persistent)
    assert case.name() == (eng.persist_plan(case.T).name)
    tok, ids, logits = run_pass(eng, case, persistent)
    positions, rows = _where(case)
    res = _check_pass(eng, mw, _matrices(mw, "bf16"), tok.reshape(-1).long(), positions, rows, logits.reshape(case.T, -1), R.chain_hip, case.id)
    eng.set_persist_taps(True)
    return res, eng, (tok, ids, logits)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16)) if a.dtype == torch.bfloat16 else torch.equal(a, b)


def run_deep(case, persistent=True, engines=None, seed=0):
    """a case of a model of n > 1 layers -> ({stage: worst / bound} of its last layer, the deep engine, (tok, ids, logits)).
    engines: (deep, shallow) to continue on (a run of launches); default: fresh ones, and the reproducibility of the pass is
    asserted on a second fresh deep engine first."""
    cfg, T, what = case.cfg, case.T, case.id
    n = cfg.n_layers
    assert n > 1
    mw = _weights(cfg)
    batch = case.row0 + case.B + 1

    def fresh(w, launch_path=False):
        e = bind(w, batch, case.l_max)
        if launch_path:
            e.set_persist_tokens(0)
        return e

    deep, shallow = engines or (fresh(mw), fresh(shallower(mw), not persistent))
    if not persistent:   # the model itself is refused (nothing was switched off on the deep engine); its first layers follow it
        assert deep.persist_tokens == 0 and not deep.persist_active(T) and not shallow.persist_active(T), what
    tok, ids, logits = run_pass(deep, case, persistent, seed)
    x_deep = deep.hidden_rows(T)
    taps = [deep.debug_rows(w, T) for w in (deep.DEBUG_Q, deep.DEBUG_ATTN, deep.DEBUG_ACT)]
    kd, vd = deep.kv_view()
    if engines is None:
        # the same pass on a second fresh engine: bit-equal hidden rows, logits and cache
        twin = fresh(mw, not persistent)
        tok2, ids2, logits2 = run_pass(twin, case, persistent, seed)
        kt, vt = twin.kv_view()
        assert torch.equal(tok, tok2) and torch.equal(ids, ids2) and torch.equal(logits, logits2), f"{what}: two engines, two results"
        assert _same_bits(x_deep, twin.hidden_rows(T)) and _same_bits(kd, kt) and _same_bits(vd, vt), f"{what}: two engines, two caches"
        del twin
    # the first n - 1 layers alone, same path, same tokens: their K / V rows are the deep engine's, bit for bit
    tok_s, _, _ = run_pass(shallow, case, persistent, seed, skip_head=True)
    ks, vs = shallow.kv_view()
    assert torch.equal(tok, tok_s)
    assert _same_bits(ks, kd[:n - 1]) and _same_bits(vs, vd[:n - 1]), f"{what}: layers 0..{n - 2} differ between the {n - 1}- and the {n}-layer engine"
    x_in = shallow.hidden_rows(T)
    # (the deep engine's taps are still those of its pass: each engine has its own workspace)
    assert _same_bits(x_deep, deep.hidden_rows(T)) and all(_same_bits(t, deep.debug_rows(w, T)) for t, w in zip(taps, (1, 2, 3)))
    positions, rows = _where(case)
    res = _check_pass(deep, mw, _matrices(mw, "bf16", layer=n - 1), tok.reshape(-1).long(), positions, rows, logits.reshape(T, -1), R.chain_hip,
                      what, layer=n - 1, x_in=x_in)
    return res, deep, (tok, ids, logits)


def run_notaps(case, twin, twin_out):
    """the case's pass on the instantiation without the stage-row stores, on a fresh engine: logits, ids and every layer's K / V
    bit-equal to `twin`'s (the instantiation with the stores, which fp64 has just vouched for)."""
    what = case.id + " (no taps)"
    mw = _weights(case.cfg)
    eng = bind(mw, case.row0 + case.B + 1, case.l_max)
    # a pass of other tokens WITH the stores first: the rows it leaves must survive the pass under test, or that pass did not run
    # the instantiation it is meant to
    run_pass(eng, case, seed=1)
    stale = [eng.debug_rows(w, case.T) for w in (eng.DEBUG_X, eng.DEBUG_Q, eng.DEBUG_ATTN, eng.DEBUG_ACT)]
    eng.set_persist_taps(False)
    tok, ids, logits = run_pass(eng, case)
    for w, s in enumerate(stale):
        assert _same_bits(s, eng.debug_rows(w, case.T)), f"{what}: stage rows {w} were written"
    assert not _same_bits(stale[1], twin.debug_rows(twin.DEBUG_Q, case.T))
    t_tok, t_ids, t_logits = twin_out
    assert torch.equal(tok, t_tok)
    assert torch.equal(ids, t_ids) and torch.equal(logits, t_logits), f"{what}: logits / ids differ from the instantiation with the stores"
    (k, v), (kt, vt) = eng.kv_view(), twin.kv_view()
    assert _same_bits(k, kt) and _same_bits(v, vt), f"{what}: K / V differ from the instantiation with the stores"
    # a pass that skips the head keeps its stores whatever the switch says: hidden rows are what it is run for
    run_pass(eng, case, skip_head=True)
    assert _same_bits(eng.hidden_rows(case.T), twin.hidden_rows(case.T)), f"{what}: a pass without the head did not store its hidden rows"
