"""-m gpu: the small row kernels that run in every layer or decode step, on the MI355X — lmi_add_rmsnorm(_lo4), lmi_rmsnorm_rows,
lmi_decode_advance, the edges of lmi_decode_sample, lmi_split_hi_lo, rectangular lmi_preprocess_images and lmi_gemm_bias_act.  The cases
and references are those of tests/row_kernels_ref.py (float64 / torch on the CPU), shared with tests/test_emu_row_kernels.py; what the
device adds is what the emulator cannot vouch for: wave-64 butterflies, the cross-wave LDS reduction of a 1024-thread workgroup, the quad
exchanges of lo4_encode8, 16-byte vector paths chosen by pointer alignment, and the compiler's choice of conversion instructions.

Device errors of the norm outputs against fp64, in the measure max |out - ref| / (1 + |ref|) (bound 2 eps(T), not tightened to what was seen):
printed by the tests; the largest seen on the MI355X were 0.442 eps (fp16) and 0.468 eps (bf16)."""
import pytest
import torch

from tests import row_kernels_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DTYPES = R.DTYPES


@pytest.fixture(scope="module")
def ops():
    from leopard_amd.ops import Ops
    assert torch.cuda.is_available()
    return Ops()


# ---- 1. add_rmsnorm / add_rmsnorm_lo4 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", R.ADD_NORM_D)
def test_add_rmsnorm(ops, dtype, D):
    worst = max(R.check_add_rmsnorm(ops, DEV, dtype, dd, M, D) for dd in (torch.float32, dtype) for M in R.ADD_NORM_M)
    print(f"[add_rmsnorm gpu {dtype} D={D}] max rel err vs fp64 = {worst / R.eps(dtype):.3f} eps")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", R.LO4_D)
def test_add_rmsnorm_lo4(ops, dtype, D):
    worst = max(R.check_add_rmsnorm_lo4(ops, DEV, dtype, dd, M, D) for dd in (torch.float32, dtype) for M in R.ADD_NORM_M)
    print(f"[add_rmsnorm_lo4 gpu {dtype} D={D}] max rel err vs fp64 = {worst / R.eps(dtype):.3f} eps")


@pytest.mark.parametrize("D", [8, 1544])
def test_add_only_changes_x_alone(ops, D):
    for dd in (torch.float32, torch.float16, torch.bfloat16):
        for M in (1, 5):
            R.check_add_only(ops, DEV, dd, M, D)


# ---- 2. rmsnorm_rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", R.ROWS_D)
def test_rmsnorm_rows(ops, dtype, D):
    worst = max(R.check_rmsnorm_rows(ops, DEV, dtype, n, D) for n in R.ROWS_N)
    worst = max(worst, max(R.check_rmsnorm_rows(ops, DEV, dtype, n, D, S=20) for n in (1, 5)))       # a short stream: the tolerance alone
    print(f"[rmsnorm_rows gpu {dtype} D={D}] max rel err vs fp64 = {worst / R.eps(dtype):.3f} eps")


# ---- 3. decode_advance ---------------------------------------------------------------------------------------------------------------------
def test_decode_advance_argmax_stop_rule_and_history(ops):
    R.check_decode_advance_stop_rule_and_history(ops, DEV)


@pytest.mark.parametrize("V,ld", [(1003, 1024), (1003, 1005), (128256, 128260)])
def test_decode_advance_rows(ops, V, ld):
    R.check_decode_advance_rows(ops, DEV, V, ld)


def test_decode_advance_full_batch(ops):
    R.check_decode_advance_full_batch(ops, DEV)


# ---- 4. decode_sample edges ----------------------------------------------------------------------------------------------------------------
# (set and identity checks only: the device's logf / expf differ from the emulator's, so a near tie of two Gumbel scores may flip a draw)
def test_kept_set_ties_keep_the_lower_indices(ops):
    R.check_kept_set_ties_keep_the_lower_indices(ops, DEV)


def test_suppressed_ids_are_never_drawn(ops):
    R.check_suppressed_ids_are_never_drawn(ops, DEV)


def test_top_k_1_is_decode_advance_and_shares_its_stop_rule(ops):
    R.check_top_k_1_is_decode_advance_and_shares_its_stop_rule(ops, DEV)


def test_rows_without_a_drawable_token_give_token_zero(ops):
    R.check_rows_without_a_drawable_token_give_token_zero(ops, DEV)


def test_draw_depends_on_seed_step_and_row_only(ops):
    R.check_draw_depends_on_seed_step_and_row_only(ops, DEV)


@pytest.mark.parametrize("T,k,p", [(1.0, 5, 1.0), (1.0, 0, 0.8), (0.7, 6, 0.7)])
def test_kept_set_on_unaligned_rows(ops, T, k, p):
    R.check_kept_set_on_unaligned_rows(ops, DEV, T, k, p)


# ---- 5. split_hi_lo, rectangular preprocess_images, gemm_bias_act --------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,K", R.SPLIT_SHAPES)
def test_split_hi_lo(ops, dtype, M, K):
    R.check_split_hi_lo(ops, DEV, dtype, M, K)


@pytest.mark.parametrize("dtype", DTYPES)
def test_preprocess_rectangular_image(ops, dtype):
    R.check_preprocess_rectangular_image(ops, DEV, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_gemm_bias_act(ops, dtype):
    R.check_gemm_bias_act(ops, DEV, dtype)
