"""The absolute bits of the training-step tail (csrc/step_tail.hip, csrc/grad_clip.hip, csrc/lars.hip through
slowfast/models/step_tail.py): every output of tests/golden/make_golden_tail_bits.py::compute() — loss gradients, ring
rows, parameters, optimizer state, trust ratios, norms, clipped gradients — has the SHA-256 digest recorded in
tests/golden/tail_bits.json.  The kernels sum in a fixed order, so the digests hold run to run; one that moves means the
order of a sum or an fma moved.  The fixture is not regenerated to make this pass."""
import json
import os

import pytest

import make_golden_tail_bits as golden

pytestmark = pytest.mark.gpu


def test_tail_outputs_keep_their_recorded_bits():
    with open(os.path.join(os.path.dirname(os.path.abspath(golden.__file__)), "tail_bits.json")) as f:
        want = json.load(f)
    got = golden.compute()
    assert sorted(got) == sorted(want), "outputs missing or new: %s" % sorted(set(got) ^ set(want))
    differ = sorted(k for k in want if got[k] != want[k])
    print("%d digests compared, %d differ" % (len(want), len(differ)))
    assert not differ, "bits differ from the recorded ones in: %s" % ", ".join(differ)
