"""The persistent forward (csrc/persist.hip) against plain fp64 computations of its stages, at every token count, instantiation
and depth it serves, within the derived bounds of tests/stage_ref.py. No bound here is fitted: every ratio printed is an error
over a bound that follows from the arithmetic, and must be <= 1.

The cases are data (tests/persist_cases.py; tests/test_persist_plan_cpu.py proves what they cover), the checks of one case are
tests/persist_run.py. Every case binds at most 1280 cache rows, raises the model to the most tokens its passes hold, asserts
that the pass runs the instantiation the planner names, and then checks: the health word; q, the new K / V rows, attention,
activation, residual and logits against fp64 (`_check_pass`; a deep model at its last layer, from the bit-reproducible hidden
rows of its first n - 1 layers); the fused ids against the first argmax of the stored logits at the caller's stride; and,
after a canary fill of the whole cache, that exactly the new positions changed, in every layer.

What is NOT here: the `SEL` instantiations (a skip word for adaptive K) are the same code under another name and can only be
reached inside the captured step; they stay with the pipeline tests (tests/test_hip_pipeline_gpu.py). Run with -s for the
table of profiles/persist_fp64_coverage.md."""


import pytest
import torch

import persist_cases as P
import persist_run as X

pytestmark = pytest.mark.gpu


def _by_model(cases):
    order = list(P.MODELS)
    return sorted(cases, key=lambda c: order.index(c.model))          # one set of large weights at a time


def _ok(res, what):
    assert res and all(r <= 1.0 for r in res.values()), (what, res)


# ---- 1. tokens and rows; 2. attention edges; 3. in-pass causality -----------------------------------------------------------------
@pytest.mark.parametrize("case", _by_model(P.GRID_CASES), ids=lambda c: c.id)
def test_tokens_and_rows(case):
    """every (B, M) class on the toys at ragged lengths, every token count of every instantiation, 256 attention units"""
    _ok(X.run_case(case)[0], case.id)


@pytest.mark.parametrize("case", P.LAUNCH_CASES, ids=lambda c: c.id)
def test_passes_beyond_the_launch_take_the_launch_path(case):
    """more attention units than CUs (B * Hq <= 256), or more tokens than a pass of the model holds: not persistent, and right"""
    _ok(X.run_case(case, persistent=False)[0], case.id)


@pytest.mark.parametrize("case", _by_model(P.EDGE_CASES + P.END_CASES), ids=lambda c: c.id)
def test_attention_edges(case):
    """cached lengths around the 32-key blocks and their round-robin over three waves, the end of the cache (the K row and V^T
    vector clamps), spiked and peaked prefixes"""
    _ok(X.run_case(case)[0], case.id)


@pytest.mark.parametrize("case", P.CAUSAL_CASES, ids=lambda c: c.id)
def test_in_pass_causality(case):
    """x 256 V at every stale position from pos0 on: query m may see the new keys <= m only, and no stale one"""
    _ok(X.run_case(case)[0], case.id)


def test_kernel_info_reports_the_plan():
    """get_kernel_info(model): what a bound model's persistent passes would run, and why not when they would not"""
    import src.kernels as K

    eng = X.bind(X._weights(P.TOY), 1, 64)
    info = K.get_kernel_info(eng)["persist"]
    assert info == {"eligible": True, "max_tokens": 8, "tokens": 8, "instance": "persist<64,1>", "ring_bytes": P.plan(P.TOY, 8).ring_bytes,
                    "reason": "", "active": True}, info
    eng.set_persist_tokens(0)
    info = K.get_kernel_info(eng)["persist"]
    assert (info["eligible"], info["max_tokens"], info["tokens"], info["active"]) == (True, 8, 0, False), info
    assert "persist" not in K.get_kernel_info()


# ---- 4. depth --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.DEPTH_CASES, ids=lambda c: c.id)
def test_depth(case):
    """layer parity of the granule buffers, tags up to the 60-layer limit, attention-unit numbers carried across layers: the
    pass is bit-reproducible, its first n - 1 layers are those of the (n - 1)-layer engine, and the last layer matches fp64"""
    _ok(X.run_deep(case)[0], case.id)


def test_61_layers_take_the_launch_path():
    case = P.DEPTH_LAUNCH_CASE
    _ok(X.run_deep(case, persistent=False)[0], case.id)


# ---- 5. the production instance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", P.NOTAPS_CASES, ids=lambda c: c.id)
def test_instance_without_stage_rows(case):
    """a loop's draft runs the instantiation without the stage-row stores. They are stores and nothing else, so its logits, ids
    and K / V are those of the instantiation with them, which the fp64 checks have just vouched for on the same pass"""
    res, twin, out = X.run_deep(case) if case.cfg.n_layers > 1 else X.run_case(case)
    _ok(res, case.id)
    X.run_notaps(case, twin, out)


# ---- 6. full vocabulary ----------------------------------------------------------------------------------------------------------------
def test_full_vocabulary():
    """1B dimensions, tied embedding, 128256 rows of lm_head: logits and the fused argmax over 256 workgroups' partials"""
    _ok(X.run_case(P.VOCAB_CASE)[0], P.VOCAB_CASE.id)


# ---- 7. a run of launches ----------------------------------------------------------------------------------------------------------------
def test_run_of_launches():
    """twenty consecutive passes on one 3-layer engine, M cycling 1, 3, 8, 2, 5 at advancing positions: tags, buffer parities and
    the LDS carve change from launch to launch; each pass is checked at the last layer like a depth case"""
    cfg = P.MODELS[P.RUN_MODEL]
    mw = X._weights(cfg)
    engines = (X.bind(mw, 2, 1280), X.bind(X.shallower(mw), 2, 1280))
    pos = 29
    for i in range(P.RUN_LAUNCHES):
        M = P.RUN_MS[i % len(P.RUN_MS)]
        case = P.Case(P.RUN_MODEL, 1, M, (pos,))
        res, _, _ = X.run_deep(case, engines=engines, seed=i)
        _ok(res, f"launch {i}: {case.id}")
        pos += M
    torch.cuda.synchronize()
