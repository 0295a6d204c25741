"""CPU tier: the host side of the wide batched matvec (csrc/kernels_gemv_rows_wide.hip) -- the plan query, by the function the launch and
the model's step call, and the argument checks of the new entries."""
import ctypes as C

import pytest

SHAPES = [(48, 128), (272, 640), (8192, 640), (4096, 1152), (12288, 4096), (151936, 4096), (1024, 3072)]


@pytest.mark.parametrize("form", [0, 1, 2])
def test_plan_query_rows_per_pass_and_row_isolation(hip_lib, form):
    from aha_amd import ops
    for N, K in SHAPES:
        want = ops.plan_gemv_rows(N, K)
        for R in range(1, 129):
            rpp, cw, nks = ops.plan_gemv_rows_wide(N, K, R, form)
            assert (cw, nks) == want, (N, K, R)          # how a row is summed never depends on the rows beside it
            # at most 32 rows: the 32-row kernel; 33 .. 64: never the 8-tile kernel; a pass no wider than the kernel's 128
            assert rpp == 32 if R <= 32 else rpp in (32, 64) if R <= 64 else rpp in (32, 64, 128), (N, K, R, rpp)
    assert ops.plan_gemv_rows_wide(4096, 4096, 40, "mxfp8") == ops.plan_gemv_rows_wide(4096, 4096, 40, 1)


def test_bad_arguments_need_no_gpu(hip_lib):
    err = hip_lib.aha_hip_last_error
    a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
    plan = hip_lib.aha_hip_debug_plan_gemv_rows_wide
    assert plan(64, 64, 32, 0, C.byref(a), None, None) == 0 and a.value == 32          # cw, nks are optional
    for args in ((64, 64, 129, 0), (64, 64, 0, 0), (64, 64, 40, 3), (64, 64, 40, -1), (64, 40, 40, 1), (64, 36, 40, 0), (0, 64, 40, 0)):
        assert plan(*args, C.byref(a), C.byref(b), C.byref(c)) == -1 and b"debug_plan_gemv_rows_wide: bad argument" in err(), args
    assert plan(64, 64, 40, 0, None, C.byref(b), C.byref(c)) == -1
    assert hip_lib.aha_hip_debug_rows_wide(None, 1) == -1 and b"debug_rows_wide: null model" in err()
    buf = (C.c_uint8 * 64)()
    p = C.addressof(buf)
    for entry, name in ((hip_lib.aha_hip_gemv_rows_mxfp8, b"gemv_rows_mxfp8"), (hip_lib.aha_hip_gemv_rows_mxfp4, b"gemv_rows_mxfp4")):
        assert entry(p, p, p, p, 129, 32, 64, 0, None, None, None, None) == -1 and name + b": bad arguments" in err()          # R > 128
    assert hip_lib.aha_hip_gemv_rows(p, p, p, 129, 32, 64, 0, None, None, None, None) == -1 and b"1 <= R <= 128" in err()
    # host memory is no operand: a valid row count does not get a launch on it
    assert hip_lib.aha_hip_gemv_rows(p, p, p, 128, 32, 64, 0, None, None, None, None) == -1 and b"not device, pinned or managed memory" in err()
