"""The attention entries against an fp64 reference on the CPU emulator: every call of tests/attn_entries_case.py (CASES, whose bits
tests/test_emu_attn_entries.py pins, and the value-only EXTRA cases) in f16 and bf16, on value inputs and on edge probes.  The model of what a
row sees, the reference, the inputs and every bound are in tests/attn_entries_ref.py; tests/test_gpu_attn_entries.py asks the same of the device.

Bounds (fixed, not tuned per case): 16-bit rows and fp32 rows within 3 eps(T) of fp64 (eps = 2^-10 / 2^-7: the project's attention bound; P
enters the P.V MFMA in 16 bits, so the fp32 rows carry that rounding too); fp8 rows (scale 16) within max(2^-4 |ref|, 2^-10 / 16) + 3 eps(T) —
half an e4m3 step plus the 16-bit kernel's bound; hl and lo4 forms as tests/decode_hl_ref.py and tests/test_gpu_lowbit.py define them.

varlen_register_staged (attn.dma = 0) gets the value checks only: the register-staged kernel is a cross-check kernel with its own tile walk and
nothing in the code promises the LDS-DMA kernel's bits.  The attn.stream_kv = 0 cases must give the bits of the default.

The two-range prefill has no fp32 form, so its lo4 cases are checked for everything but the image's host rule (hi == the plain launch,
padding, unselected rows, hi + image no farther from fp64 than hi).

FOUND BY THESE TESTS AND FIXED WITH THEM (both files failed before the fix, with the same figures on the emulator and the device):
* attn.rows64 = 1 in f16 (attention64.h, NBLK == 2): 1004.78 eps on the x 4 values, probe rows up to 163.8 eps.  The kernel took its softmax
  reference over the UNMASKED scores of a step; a hidden key ~11 above every visible key made the visible keys' P underflow in f16.  It now
  masks before it takes the maxima, as the NBLK == 1 variant always did.
* the lo4 image on the device, x 4 values: 5.8e-3 .. 4.1e-2 of the elements off the host rule (cap 2e-3) and hi + image farther from fp64 than
  hi (4.4e-4 against 3.5e-4).  hipcc fused the multiply o * inv with the 16-bit conversion inside the residual (one rounding) but not in the
  stored row (two): on a 16-bit midpoint the image was taken against the other neighbour.  The epilogue now separates the two (sep_rn); the
  image equals the host rule in every element of these cases."""
import pytest

from tests import attn_entries_ref as R
from tests.attn_entries_case import DTYPES

NAMES = sorted(R.all_cases())
DEV = "cpu"


@pytest.fixture(scope="module")
def ops():
    from tests.emu_util import emu_ops
    return emu_ops()


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", NAMES)
def test_probes_are_sharp(name, dtype):
    """No kernel: at EVERY row a probe applies to, the reference with the target key's visibility flipped differs from the true one by more
    than 10 x the tolerance that row is checked with; and the case has rows for every edge kind its arguments give it."""
    spec = R.all_cases()[name]
    R.check_edges_present(spec)
    sharp = R.sharpness(spec, dtype)
    assert sharp
    for key, (rows, ratio, _) in sharp.items():
        print(f"{name}/{dtype} {key}: {rows} rows, mutant at least {ratio:.1f} x tolerance")
        assert rows > 0 and ratio > 10, f"{name}/{dtype} {key}: a row moves by only {ratio:.2f} x its tolerance"


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", NAMES)
def test_values(ops, name, dtype):
    for family in R.FAMILIES:
        R.check_values(ops, R.all_cases()[name], dtype, DEV, family)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", NAMES)
def test_edge_probes(ops, name, dtype):
    assert R.check_probes(ops, R.all_cases()[name], dtype, DEV)


@pytest.mark.parametrize("dtype", sorted(DTYPES))
@pytest.mark.parametrize("name", R.stream_twins())
def test_no_stream_gives_the_streamed_bits(ops, name, dtype):
    fn, kw, opts = R.all_cases()[name]
    R.check_same_bits(ops, dtype, DEV, (fn, kw, opts), (fn, kw, {k: v for k, v in opts.items() if k != "attn.stream_kv"}))


@pytest.mark.parametrize("dtype", sorted(DTYPES))
def test_windows_that_hide_nothing_or_all_but_one(ops, dtype):
    R.check_window_above_all(ops, dtype, DEV)
    R.check_window_one(ops, dtype, DEV)
