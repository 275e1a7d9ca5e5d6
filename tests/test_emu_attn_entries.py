"""The attention entries pinned to recorded emulator bits.  tests/golden/attn_entries_emu_bits.json holds a SHA-256 of every output tensor of the calls in
tests/attn_entries_case.py, as the emulator build (``make emu``) of the commit BEFORE the attention host side was unified gave them — generated from a
checkout of that commit, never from the tree under test:

    make emu && LEOPARD_AMD_LIB=$PWD/tools/hipemu/libleopard_amd_emu.so python -m tests.attn_entries_case > attn_entries_emu_bits.json

with tests/attn_entries_case.py copied into that checkout.  The kernels are untouched, so a digest moves only if an entry hands a kernel other
arguments or another grid.  Shown by mutation of the split-KV launcher when the test was added: the merge told a wrong split count, the own pass a
wrong split_base, the merge a wrong lo_rows, and the own pass launched as the non-causal instantiation each fail cases here.  What NO digest can see is
the streaming own-pass instantiation launched in place of the plain one (or the reverse): the two differ in the cache policy of their K / V loads and
give the same bits, here and on the device (profiles/attn_host_device_bits.txt compares the launched kernel symbols instead)."""
import json
import os

import pytest

from tests.attn_entries_case import CASES, DTYPES, run_case

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "attn_entries_emu_bits.json")


@pytest.fixture(scope="module")
def ops():
    from tests.emu_util import emu_ops
    return emu_ops()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_fixture_lists_exactly_these_cases(golden):
    assert sorted(golden) == sorted(f"{name}/{dtype}" for name in CASES for dtype in DTYPES)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", sorted(CASES))
def test_emulator_bits_are_the_recorded_ones(ops, golden, name, dtype):
    assert run_case(ops, name, dtype) == golden[f"{name}/{dtype}"]
