"""sd_persist_plan on a machine without a GPU: the query itself, the pins of the models the GPU cases use and of the models
the persistent forward must refuse, and the closure of the GPU case list (tests/persist_cases.py) over every instantiation, token
count and (B, M) class.

The planner asks the functions the bind (persist_model_ok, persist_max_tokens) and the launch (its LDS carve, its instantiation
switch) ask, so a change to the work split or the carve that moves a model on or off the kernel, or a pass to another
instantiation, fails here first."""

import ctypes
import dataclasses

import pytest

import persist_cases as P
from gemm_body_cases import S1B_V, S8B
from specdec_hip import _abi
from specdec_hip import weights as W
from specdec_hip.ops import persist_plan


def test_query_and_argument_validation():
    lib = _abi.load()
    for name in ("sd_persist_plan", "sd_model_set_persist_taps"):
        assert hasattr(lib, name) and name in _abi.SIGNATURES
    p = P.plan(P.TOY, 3)
    assert p == (True, 8, "persist<64,1>", p.ring_bytes, "") and p.ring_bytes % 1024 == 0 and p.ring_bytes >= 64 * 1024
    out = [ctypes.c_int(0) for _ in range(3)]
    refs = [ctypes.byref(x) for x in out]
    name, reason = ctypes.create_string_buffer(32), ctypes.create_string_buffer(96)
    dims = (W.ARCH_LLAMA, 1, 256, 4, 2, 64, 512, 512, 1, _abi.SD_BF16, 0)
    assert lib.sd_persist_plan(*dims, 3, *refs, name, 32, reason, 96) == 0 and name.value == b"persist<64,1>" and reason.value == b""
    assert lib.sd_persist_plan(*dims, 3, None, refs[1], refs[2], name, 32, reason, 96) != 0 and "NULL" in _abi.last_error()
    assert _abi.last_error().startswith("persist_plan:")
    assert lib.sd_persist_plan(*dims, 3, *refs, None, 32, reason, 96) != 0 and "NULL" in _abi.last_error()
    assert lib.sd_persist_plan(*dims, 0, *refs, name, 32, reason, 96) != 0 and "T=0" in _abi.last_error()
    assert lib.sd_persist_plan(*dims, 3, *refs, name, len("persist<64,1>"), reason, 96) != 0 and "too short" in _abi.last_error()
    assert lib.sd_persist_plan(*dims, 3, *refs, name, len("persist<64,1>") + 1, reason, 1) == 0       # "" and its NUL
    assert lib.sd_persist_plan(*dims, 9, *refs, name, 32, reason, 8) != 0 and "too short" in _abi.last_error()
    assert lib.sd_persist_plan(*dims[:9], 3, 0, 3, *refs, name, 32, reason, 96) != 0 and "weight_dtype" in _abi.last_error()   # SD_I32
    assert lib.sd_persist_plan(W.ARCH_LLAMA, 1, -256, *dims[3:], 3, *refs, name, 32, reason, 96) != 0 and "dimension" in _abi.last_error()
    assert lib.sd_persist_plan(W.ARCH_LLAMA, 1, 0, *dims[3:], 3, *refs, name, 32, reason, 96) != 0 and "dimension" in _abi.last_error()
    assert lib.sd_persist_plan(*dims[:7], 0, *dims[8:], 3, *refs, name, 32, reason, 96) != 0 and "dimension" in _abi.last_error()      # vocab
    assert lib.sd_model_set_persist_taps(None, 1) != 0 and "NULL" in _abi.last_error()


# ---- pins ------------------------------------------------------------------------------------------------------------------------
# (instantiation, tokens per pass, ring KiB at T = 1 and at the limit). Instantiation and tokens per pass were worked out by hand
# from the LDS carve (per token a staged row of max(d_model, Hq * D, d_ff) bf16 and its share of the residual and attention
# scratch, next to a ring of at least 64 KiB); the ring sizes are the library's own, pinned so that a change of the carve shows
PINS = {
    "toy-d64": ("persist<64,1>", 8, 151, 137), "toy-d128-v3001": ("persist<128,1>", 8, 148, 120), "1b-layer": ("persist<64,1>", 5, 136, 68),
    "3b-layer": ("persist<128,2>", 4, 134, 80), "wide-d64": ("persist<64,2>", 6, 140, 75), "widest": ("persist<128,2>", 3, 126, 74),
    "heads64": ("persist<64,1>", 8, 144, 81),
}


@pytest.mark.parametrize("model", sorted(PINS))
def test_table_of_the_case_models(model):
    cfg = P.MODELS[model]
    name, cap, ring1, ring_cap = PINS[model]
    if model in P.TABLE:
        assert P.TABLE[model] == (name, cap)
    rings = []
    for T in range(1, cap + 1):
        p = P.plan(cfg, T)
        assert (p.eligible, p.max_tokens, p.name, p.reason) == (True, cap, name, ""), (model, T, p)
        rings.append(p.ring_bytes)
    assert (rings[0] // 1024, rings[-1] // 1024) == (ring1, ring_cap), (model, rings)
    assert all(a > b for a, b in zip(rings, rings[1:])) and rings[-1] >= 64 * 1024, (model, rings)   # every token's rows shrink the ring
    print(f"[persist plan] {model}: {name} cap {cap} ring KiB " + " ".join(str(r // 1024) for r in rings))


def test_tokens_above_the_limit_are_refused():
    for model, (_, cap, _, _) in PINS.items():
        for T in sorted({cap + 1, 9, 64}):
            p = P.plan(P.MODELS[model], T)
            assert p.eligible and p.max_tokens == cap and p.name == "none" and p.ring_bytes == 0, (model, T, p)
            assert p.reason.startswith(f"tokens: T={T} above the {cap} "), (model, T, p)


def _refused(p, rule):
    assert (p.eligible, p.max_tokens, p.name, p.ring_bytes) == (False, 0, "none", 0) and p.reason.startswith(rule), (p, rule)


def test_eligibility_rules_are_pinned():
    # 1B dimensions at the full vocabulary: the lm_head is cut for 256 workgroups like every other matrix
    p = P.plan(S1B_V, 5)
    assert (p.eligible, p.max_tokens, p.name) == (True, 5, "persist<64,1>"), p
    assert P.plan(P.S1B_TIED, 5)[:3] == p[:3]
    assert P.plan(W.LLAMA_3_2_1B, 2).name == "persist<64,1>" and P.plan(W.LLAMA_3_2_3B, 4).name == "persist<128,2>"
    # the 8B layer: d_ff = 14336 gives 56 gate / up pairs per workgroup in 8 tiles of 7, and an activation granule holds two
    # neighbouring pairs of one tile. Nothing else refuses it: with d_ff = 14336 + 2048 = 16384 (8 tiles of 8) it is eligible
    _refused(P.plan(S8B), "gate / up:")
    _refused(P.plan(W.LLAMA_3_8B), "gate / up:")
    assert P.plan(dataclasses.replace(S8B, d_ff=16384)).eligible
    _refused(persist_plan(W.ARCH_LLAMA, 1, 128, 4, 2, 32, 256, 512), "head_dim:")                       # the stage tests' tiny-d32
    _refused(P.plan(W.GPT2_SMALL), "architecture:")
    _refused(P.plan(P.TOY, weight_dtype="fp8"), "weights: fp8")
    _refused(P.plan(P.TOY, packed=False), "weights: row-major")
    _refused(P.plan(P.TOY, has_bias=True), "bias:")
    _refused(persist_plan(W.ARCH_LLAMA, 1, 4224, 33, 3, 128, 8448, 512), "d_model:")
    assert P.plan(P.WIDEST).eligible                                                                   # 4096 itself
    _refused(persist_plan(W.ARCH_LLAMA, 1, 320, 5, 1, 64, 512, 512), "rows:")                            # 320 is no multiple of 128
    _refused(P.plan(dataclasses.replace(P.TOY, n_layers=0)), "layers:")
    _refused(P.plan(P.TOY_61L), "layers:")
    assert P.plan(P.TOY_60L, 8).name == "persist<64,1>"
    # QKV tiles per workgroup: 8192 pairs are 32 per workgroup in 4 tiles of 8; 9216 are 36 in 8 tiles of 5 (the work split makes
    # 1, 2, 4 or 7..8 tiles: a shape with exactly 5 does not exist)
    assert P.plan(dataclasses.replace(P.WIDEST, n_heads=96, n_kv_heads=16)).eligible
    _refused(P.plan(dataclasses.replace(P.WIDEST, n_heads=128, n_kv_heads=8)), "QKV:")


def test_no_persist_switch_reaches_the_planner(monkeypatch):
    monkeypatch.setenv("SPECDEC_NO_PERSIST", "1")
    _refused(P.plan(P.TOY), "SPECDEC_NO_PERSIST")


# ---- coverage of the GPU case list ------------------------------------------------------------------------------------------------
def test_cases_are_persistent_passes_with_unique_ids():
    ids = [c.id for c in P.PERSIST_CASES + P.LAUNCH_CASES + [P.DEPTH_LAUNCH_CASE]]
    assert len(ids) == len(set(ids))
    for c in P.PERSIST_CASES:
        assert c.name() in P.INSTANCES, (c.id, P.plan(c.cfg, c.T))
        assert c.B * c.cfg.n_heads <= 256 and c.l_max <= 1280 and c.l_max % 8 == 0 and len(c.bases) == c.B, c.id
        assert all(0 <= p and p + c.M <= c.l_max for p in c.bases), c.id
    # the passes that must take the launch path: refused by the planner (tokens, layers) or by the attention units of the pass
    for c in P.LAUNCH_CASES + [P.DEPTH_LAUNCH_CASE]:
        assert c.name() == "none" or c.B * c.cfg.n_heads > 256, c.id


def test_every_instantiation_at_every_token_count():
    seen = {}
    for c in P.GRID_CASES:
        if c.B == 1:
            seen.setdefault((c.model, c.name()), set()).add(c.T)
    by_instance = {}
    for (model, name), Ts in seen.items():
        cap = P.plan(P.MODELS[model]).max_tokens
        if Ts == set(range(1, cap + 1)):
            by_instance.setdefault(name, []).append((model, cap))
    assert sorted(by_instance) == sorted(P.INSTANCES), by_instance
    # and every model of the table is swept whole
    for model, (name, cap) in P.TABLE.items():
        assert (model, cap) in by_instance[name], (model, by_instance)


def test_every_batch_shape_class():
    for model in ("toy-d64", "toy-d128-v3001"):
        have = {(c.B, c.M) for c in P.GRID_CASES if c.model == model}
        assert have >= set(P.CLASSES), (model, set(P.CLASSES) - have)
        for c in P.GRID_CASES:
            if c.model == model and c.B > 1:
                assert len(set(c.bases)) == c.B, c.id                       # ragged: no two rows at the same length
    assert set(P.CLASSES) >= {(1, M) for M in range(1, 9)} | {(B, 1) for B in (2, 3, 5, 8)} | {(2, 2), (2, 3), (3, 2), (2, 4), (4, 2)}
    # both parities of M >= 3: the last new position staged by the gatherer (odd M) and by the third consumer (even M), in the
    # one-row sweeps, the batched shapes, the attention edges, the causality cases and the deep models
    for group in (P.GRID_CASES, [c for c in P.GRID_CASES if c.B > 1], P.EDGE_CASES, P.END_CASES, P.CAUSAL_CASES, P.DEPTH_CASES):
        assert {c.M % 2 for c in group if c.M >= 3} == {0, 1}, group[0].id
    # a pass at row0 > 0 of a larger bound batch
    assert any(c.row0 > 0 and c.B > 1 and c.M > 1 for c in P.GRID_CASES) and any(c.row0 > 0 for c in P.DEPTH_CASES)
    # 256 attention units, and the first count beyond them at a token count the model holds
    assert any(c.B * c.cfg.n_heads == 256 for c in P.GRID_CASES)
    assert any(c.B * c.cfg.n_heads > 256 and c.name() != "none" for c in P.LAUNCH_CASES)


def test_attention_edge_and_depth_lists():
    for (model, M) in P.EDGE_SHAPES:
        for kind in ("spikes", "peaked"):
            assert {c.bases[0] for c in P.EDGE_CASES if (c.model, c.M, c.prefix) == (model, M, kind)} == set(P.EDGE_LENGTHS)
            assert any((c.model, c.M, c.prefix, c.bases[0] + c.M, c.l_max) == (model, M, kind, 1280, 1280) for c in P.END_CASES)
    assert {(c.bases[0], c.M) for c in P.END_CASES if c.l_max == 8} == {(0, 8), (7, 1)}
    assert {c.M for c in P.CAUSAL_CASES} == {3, 5, 8}
    assert {(c.model, c.T) for c in P.DEPTH_CASES if c.B == 1} == {(m, T) for m in ("toy-d64-3l", "toy-d128-v3001-2l") for T in (1, 3, 8)} | {("toy-d64-60l", 2)}
    assert {(c.model, c.T) for c in P.NOTAPS_CASES} == {(m, T) for m in ("toy-d64-3l", "toy-d128-v3001", "1b-layer") for T in (1, 2, 5)}
    assert any(c.cfg.n_layers > 1 for c in P.NOTAPS_CASES)
    assert P.VOCAB_CASE.cfg.vocab == 128256 and P.VOCAB_CASE.cfg.tie_embeddings and P.VOCAB_CASE.T == 5
    assert P.RUN_LAUNCHES == 20 and P.RUN_MS == (1, 3, 8, 2, 5) and P.MODELS[P.RUN_MODEL].n_layers == 3
