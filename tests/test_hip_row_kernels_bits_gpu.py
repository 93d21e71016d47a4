"""The vocabulary-row kernels, bit for bit against recorded outputs (tests/golden/row_kernels_bits.npz, recorded on the commit
before their device pieces were shared; tests/row_kernel_cases.py holds the cases, the inputs and the recorder).

The other GPU tests compare ids exactly with the CPU restatements and float64 outputs within derived bounds; this one asks for
equality of every bit, which is what a change to a shared walker, reduction or selection piece has to keep.
"""

import functools

import numpy as np
import pytest

import row_kernel_cases as C

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _fixture():
    with np.load(C.FIXTURE) as z:
        return {k: z[k] for k in z.files}


def test_fixture_holds_exactly_the_cases():
    assert {k.split(":")[0] for k in _fixture()} == set(C.CASES)
    assert C.FIXTURE.stat().st_size < 100 * 1024


@pytest.mark.parametrize("name", list(C.CASES))
def test_outputs_are_the_recorded_bits(name):
    want = {k: v for k, v in _fixture().items() if k.split(":")[0] == name}
    got = C.run_case(name)
    assert set(got) == set(want)
    for k, v in got.items():
        assert v.dtype == want[k].dtype and np.array_equal(v, want[k]), k
        if k.endswith("@offset"):   # sd_spec_agreement: the bits do not depend on the rows' alignment
            assert np.array_equal(v, got[k[:-len("@offset")]]), k
