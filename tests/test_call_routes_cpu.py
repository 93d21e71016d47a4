"""What every call resolves to — route, expanded prompts, step options, or the refusal with its full message — against the
outcomes recorded before the resolution moved to src/specdec/core/step_options.py (tests/call_route_cases.py has the cases, the
stand-ins and the recorder; tests/golden/call_routes.json the recording). Runs without a device."""

import json

import pytest

import call_route_cases as C


@pytest.fixture(scope="module")
def recorded():
    return json.loads(C.FIXTURE.read_text())


@pytest.fixture(scope="module")
def run():
    hits = set()
    return C.run_all(hits), hits


def test_the_fixture_holds_exactly_the_cases(recorded):
    assert recorded["stand_ins"] == list(C.STAND_INS) and recorded["entries"] == list(C.ENTRIES) and recorded["args"] == list(C.ARGS)
    assert sorted(C.unpack(recorded)) == sorted(C.cases())
    assert C.FIXTURE.stat().st_size < 100_000


def test_every_case_resolves_as_recorded(recorded, run):
    want, (got, _) = C.unpack(recorded), run
    wrong = [c for c in C.cases() if got[c] != want[c]]
    assert not wrong, f"{len(wrong)} of {len(want)} cases differ; the first: {wrong[0]}\n  recorded {want[wrong[0]]}\n  now      {got[wrong[0]]}"


def test_every_refusal_of_the_resolution_is_produced_by_a_case(run):
    _, hits = run
    assert C.raise_sites(), "no raise found in scope: the scope names no function of this tree"
    assert C.raise_coverage(hits) == sorted(C.KNOWN_UNREACHED)


def test_a_sampling_description_becomes_step_options():
    from src.specdec.core.step_options import Processors, StepOptions

    o = StepOptions.from_sampling({"temperature": 0.7, "top_k": 50, "top_p": 0.9, "seed": 3})
    assert (o.mode, o.temperature, o.top_k, o.top_p, o.seed) == ("sampled", 0.7, 50, 0.9, 3)
    assert StepOptions.from_sampling(None).mode == "greedy" and StepOptions.from_sampling({"spec": True, "temperature": 1.0, "top_k": None,
                                                                                          "top_p": None, "seed": 0}).mode == "spec"
    assert Processors.IDENTITY == Processors(1.0, 0.0, 0.0, None)
