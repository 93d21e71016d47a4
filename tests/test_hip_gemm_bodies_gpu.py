"""Every instantiation of the multi-token weight-streaming kernels (csrc/gemm_skinny.hip, csrc/gemm_pipe.hip) that a pass can
reach, each against the fp64 stage references of tests/stage_ref.py (error / bound <= 1 at every stage), by plan: a case first
asserts that `HipModel.pass_plan` names the instantiations the case list (tests/gemm_body_cases.py) records for it, so a
changed chooser fails the case instead of silently testing another kernel. tests/test_gemm_plan_cpu.py proves without a GPU
that the list reaches every name the models the project runs can reach.

Beyond the stage checks (tests/gemm_body_run.py): the fused argmax against the logits the same launch stored, the KV cache
bitwise untouched outside the new positions (a padded token column t in T..16 TG - 1 that stored anything would land in the
spare cache row or beside a row's new positions), batched ragged rows at row0 > 0 on dense and paged caches, and the row
statistics a down-projection hands to the next layer's QKV launch. The bodies only SPECDEC_NO_DIRECT / SPECDEC_NO_PIPE reach
run in one fresh child process per knob setting: the library reads the knobs once per process."""

import json
import os
import subprocess
import sys

import pytest

import gemm_body_cases as G
from gemm_body_run import run_case

pytestmark = pytest.mark.gpu

_CASES = sorted(G.GPU_CASES + G.BATCHED_CASES, key=lambda c: (c.model, c.wd, c.T))


@pytest.mark.parametrize("case", _CASES, ids=[c.id for c in _CASES])
def test_planned_body(case):
    res = run_case(case)
    assert res and all(r <= 1.0 for r in res.values()), res


@pytest.mark.parametrize("case", G.TWO_LAYER_CASES, ids=[c.id for c in G.TWO_LAYER_CASES])
def test_cross_layer_statistics(case):
    res = run_case(case)
    assert res and all(r <= 1.0 for r in res.values()), res


_KNOBS = [(G.PLAN_NO_DIRECT, {"SPECDEC_NO_DIRECT": "1"}), (G.PLAN_NO_PIPE, {"SPECDEC_NO_PIPE": "1"}),
          (G.PLAN_NO_DIRECT | G.PLAN_NO_PIPE, {"SPECDEC_NO_DIRECT": "1", "SPECDEC_NO_PIPE": "1"})]


def test_knob_only_bodies():
    """one child per knob setting, one at a time; a child that does not end with status 0 fails the test at once and no
    further child is started"""
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gemm_body_run.py")
    base = {k: v for k, v in os.environ.items() if k not in ("SPECDEC_NO_DIRECT", "SPECDEC_NO_PIPE")}
    for flags, knobs in _KNOBS:
        n = sum(1 for c in G.KNOB_CASES if c.flags == flags)
        assert n > 0, flags
        try:
            p = subprocess.run([sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [script, str(flags)], env={**base, **knobs},
                               capture_output=True, text=True, timeout=60 + 30 * n)
        except subprocess.TimeoutExpired as e:
            pytest.fail(f"knob child flags={flags} did not finish in {e.timeout} s; no further child started\n{e.stdout}\n{e.stderr}")
        print(p.stdout)
        assert p.returncode == 0, f"knob child flags={flags} ended with status {p.returncode}; no further child started\n{p.stdout[-4000:]}\n{p.stderr[-4000:]}"
        rec = json.loads(p.stdout.strip().splitlines()[-1])
        assert rec["flags"] == flags and len(rec["cases"]) == n, rec
        assert all(r <= 1.0 for res in rec["cases"].values() for r in res.values()), rec
        print(f"[knob flags={flags}] worst error / bound per stage: " + " ".join(f"{k} {v:.3f}" for k, v in rec["worst"].items()))
