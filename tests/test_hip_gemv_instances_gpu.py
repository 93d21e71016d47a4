"""Every kernel a launch-path pass of 1..9 tokens can run — the fixed-geometry instances and the generic instantiations of
csrc/gemv.hip, and the csrc/gemm_skinny.hip bodies that rows too long to stage are handed to — each against the fp64 stage
references of tests/stage_ref.py (error / bound <= 1 at every stage), by name: a case first asserts that
`HipModel.small_pass_instances` names the kernels the case list (tests/gemv_cases.py) records for it, so a changed chooser fails
the case instead of silently testing another kernel. tests/test_gemv_instance_cpu.py proves without a GPU that the list
reaches every name the models the project runs can reach.

The pass, the stage checks and the further checks are those of tests/gemm_body_run.py: the fused argmax against the logits the
same launch stored, ids untouched past M at a row stride of the caller's, and the canary-filled KV cache bitwise unchanged
outside the new positions with every new position written (a padded token column of a tt5 / tt9 instantiation that stored
anything would land beside a row's new positions or in the spare cache row). Batched cases run the t -> (row, position) map at
ragged lengths and row0 > 0, dense and paged. No tolerance is introduced here: the bounds are stage_ref's.

SPECDEC_GEMV_GENERIC is read at every launch, so the switch cases run in this process. The worst error / bound per stage and
per case family is printed when the module is done (run with -s)."""

import pytest

import gemv_cases as V
from gemm_body_run import run_case

pytestmark = pytest.mark.gpu

# by model: one large weight set is resident at a time (the cache of tests/test_hip_stage_fp64_gpu.py)
_CASES = sorted(V.GPU_CASES + V.SWITCH_CASES, key=lambda c: (c.model, c.wd, c.generic, c.B, c.T))
_WORST = {}


def _family(case, names):
    if case.generic:
        return "switch"
    if case.B > 1:
        return "batched"
    if any(n.startswith("skinny:") for n in names):
        return "hand-over"
    return "fixed" if names[0].startswith("fixed<") else "generic"


def _named_instances(eng, case):
    """the drift check: the engine, in this process's environment, runs the kernels the case list recorded"""
    assert eng.small_pass_instances(case.T) == case.names(), (case.id, eng.small_pass_instances(case.T), case.names())


@pytest.fixture(scope="module", autouse=True)
def _print_worst():
    yield
    for fam, res in sorted(_WORST.items()):
        print(f"\n[gemv instances] {fam}: worst error / bound per stage: " + " ".join(f"{k} {v:.3f}" for k, v in res.items()), end="")
    print()


def test_shared_models_are_the_stage_suite_s():
    """the weight cache is keyed by model name: the models this case list defines under the stage suite's names are equal"""
    import test_hip_stage_fp64_gpu as S
    assert (V.GPT2, V.TOY128, V.MODELS["toy-d64"], V.MODELS["8b-layer"]) == (S.GPT2, S.TOY128, S.TOY, S.S8B)


@pytest.mark.parametrize("case", _CASES, ids=[c.id for c in _CASES])
def test_named_instance(case, monkeypatch):
    if case.generic:
        monkeypatch.setenv(V.SWITCH, "1")
    else:
        monkeypatch.delenv(V.SWITCH, raising=False)
    res = run_case(case, _named_instances)
    worst = _WORST.setdefault(_family(case, case.names()), {})
    for k, r in res.items():
        worst[k] = max(worst.get(k, 0.0), r)
    assert set(res) == {"q", "k", "v", "attn", "act", "x", "logits"} and all(r <= 1.0 for r in res.values()), res
