"""lmi_token_logprobs pinned to recorded bits: tests/golden/token_logprobs_bits.npz holds what the kernel gave through the host emulator (the device bits are not
recorded yet) before its row scan became the device functions it now shares with lmi_decode_logprobs (tests/token_logprobs_case.py builds
the inputs).  The scan's arithmetic must not move by a bit."""
import os

import numpy as np
import pytest

from tests.token_logprobs_case import CASES, run_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "token_logprobs_bits.npz")


def compare(got, prefix):
    z = np.load(GOLDEN)
    for key, val in got.items():
        assert np.array_equal(val, z[prefix + key]), (prefix + key, val, z[prefix + key])


@pytest.mark.parametrize("name", sorted(CASES))
def test_emulator_bits_are_the_recorded_ones(name):
    from tests.emu_util import emu_ops
    compare(run_case(emu_ops(), name), "emu_")

