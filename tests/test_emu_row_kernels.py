"""The small row kernels on the CPU emulator: the cases of tests/row_kernels_ref.py (shared with tests/test_gpu_row_kernels.py, which runs
them on the MI355X) plus the argument checks of the norm entry points, which need no device."""
import pytest
import torch

from leopard_amd.ops import Lo4Act, lo4_k4
from tests import row_kernels_ref as R
from tests.emu_util import emu_ops

DEV = "cpu"
DTYPES = R.DTYPES


@pytest.fixture(scope="module")
def ops():
    return emu_ops()


# ---- 1. add_rmsnorm / add_rmsnorm_lo4 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", R.ADD_NORM_D)
def test_add_rmsnorm(ops, dtype, D):
    worst = max(R.check_add_rmsnorm(ops, DEV, dtype, dd, M, D) for dd in (torch.float32, dtype) for M in R.ADD_NORM_M)
    print(f"[add_rmsnorm emu {dtype} D={D}] max rel err vs fp64 = {worst / R.eps(dtype):.3f} eps")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", R.LO4_D)
def test_add_rmsnorm_lo4(ops, dtype, D):
    worst = max(R.check_add_rmsnorm_lo4(ops, DEV, dtype, dd, M, D) for dd in (torch.float32, dtype) for M in R.ADD_NORM_M)
    print(f"[add_rmsnorm_lo4 emu {dtype} D={D}] max rel err vs fp64 = {worst / R.eps(dtype):.3f} eps")


@pytest.mark.parametrize("D", [8, 1544])
def test_add_only_changes_x_alone(ops, D):
    for dd in (torch.float32, torch.float16, torch.bfloat16):
        for M in (1, 5):
            R.check_add_only(ops, DEV, dd, M, D)


def test_add_rmsnorm_rejects_bad_arguments(ops):
    def call(D, delta_dtype=torch.float32, dtype=torch.float16, M=3):
        x, d = torch.zeros(M, D), torch.zeros(M, D, dtype=delta_dtype)
        ops.add_rmsnorm(x, d, torch.ones(D), torch.zeros(M, D, dtype=dtype), R.RMS_EPS)
    call(16)
    for D in (12, 4104):                                                  # D % 8 != 0, D > 4096
        with pytest.raises(RuntimeError, match="lmi_add_rmsnorm: bad argument"):
            call(D)
    with pytest.raises(RuntimeError, match="delta_dtype must be LMI_F32 or dtype"):
        call(16, delta_dtype=torch.bfloat16, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="delta_dtype must be LMI_F32 or dtype"):
        call(16, delta_dtype=torch.float16, dtype=torch.bfloat16)


def test_add_rmsnorm_lo4_rejects_bad_arguments(ops):
    def call(D, k4=None, delta_dtype=torch.float32, dtype=torch.float16, M=3):
        k4 = k4 or lo4_k4(D)
        act = Lo4Act(torch.zeros(M, D, dtype=dtype), torch.zeros(M, k4 // 2, dtype=torch.uint8), torch.zeros(M, k4 // 32, dtype=torch.uint8))
        ops.add_rmsnorm_lo4(torch.zeros(M, D), torch.zeros(M, D, dtype=delta_dtype), torch.ones(D), act, R.RMS_EPS)
    call(32)
    for D, k4 in ((40, None), (4128, None), (32, 512), (512, 768)):       # D % 32 != 0, D > 4096, K4 other than D rounded up to 256
        with pytest.raises(RuntimeError, match="lmi_add_rmsnorm_lo4: bad argument"):
            call(D, k4)
    with pytest.raises(RuntimeError, match="delta_dtype must be LMI_F32 or dtype"):
        call(32, delta_dtype=torch.bfloat16, dtype=torch.float16)


# ---- 2. rmsnorm_rows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", R.ROWS_D)
def test_rmsnorm_rows(ops, dtype, D):
    worst = max(R.check_rmsnorm_rows(ops, DEV, dtype, n, D) for n in R.ROWS_N)
    worst = max(worst, max(R.check_rmsnorm_rows(ops, DEV, dtype, n, D, S=20) for n in (1, 5)))       # a short stream: the tolerance alone
    print(f"[rmsnorm_rows emu {dtype} D={D}] max rel err vs fp64 = {worst / R.eps(dtype):.3f} eps")


# ---- 3. decode_advance ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,ld", [(1003, 1024), (1003, 1005), (128256, 128260)])
def test_decode_advance_rows(ops, V, ld):
    R.check_decode_advance_rows(ops, DEV, V, ld)


def test_decode_advance_full_batch(ops):
    R.check_decode_advance_full_batch(ops, DEV)


# ---- 4. decode_sample edges (the cases of tests/test_emu_sampling.py run from there; here the one this file adds) ---------------------------
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
