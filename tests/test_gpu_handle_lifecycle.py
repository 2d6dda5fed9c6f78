"""Create / use / destroy cycles of the C ABI handle leak no device memory, and a handle built on
recycled memory steps exactly like the first. Free device memory is read with hipMemGetInfo from the HIP
runtime the library itself runs on."""
import ctypes

import pytest

import bos
from conftest import MINI

pytestmark = pytest.mark.gpu

WARMUP, CYCLES = 3, 20
KINDS = [(bos.BOS_SOLVER_SCHUR, bos.BOS_FP32), (bos.BOS_SOLVER_SUPERNODAL, bos.BOS_FP64),
         (bos.BOS_SOLVER_DENSE_CHOL, bos.BOS_FP64), (bos.BOS_SOLVER_ROCSOLVER_RF, bos.BOS_FP64)]


def _hip_runtime():
    with open("/proc/self/maps") as f:
        path = next(line.split()[-1] for line in f if "libamdhip64" in line)
    return ctypes.CDLL(path)


def _free_bytes(hip):
    free, total = ctypes.c_size_t(), ctypes.c_size_t()
    assert hip.hipMemGetInfo(ctypes.byref(free), ctypes.byref(total)) == 0
    return free.value


def _cycle(P, solver, precision, before_destroy=None):
    S = bos.Solver(P, precision=precision, solver=solver)
    try:
        chi2 = S.step()["chi2"]
        if solver in (bos.BOS_SOLVER_SCHUR, bos.BOS_SOLVER_SUPERNODAL):
            S.marginals()
            S.edge_covariances()
            S.pair_covariances([0, 1], [1, P.NP])   # a pose-pose and a pose-landmark pair
            S.cost()
        if before_destroy:
            before_destroy()
    finally:
        S.close()
    return chi2


@pytest.mark.parametrize("solver,precision", KINDS)
def test_cycles_leak_nothing_and_repeat_bitwise(solver, precision):
    P = bos.load_g2o(MINI)
    hip = _hip_runtime()
    chi2 = [_cycle(P, solver, precision) for _ in range(WARMUP)]   # absorbs the runtime's one-time caches
    f0 = _free_bytes(hip)
    live = []
    chi2.append(_cycle(P, solver, precision, lambda: live.append(_free_bytes(hip))))
    handle = f0 - live[0]
    chi2 += [_cycle(P, solver, precision) for _ in range(CYCLES)]
    f1 = _free_bytes(hip)
    print(f"lifecycle solver={solver} precision={precision}: F0-F1={f0 - f1} bytes, H={handle} bytes")
    assert handle > 0
    assert f0 - f1 < handle / 2   # half a handle leaked over all the cycles fails
    assert len({bos.np.float64(c).tobytes() for c in chi2}) == 1, chi2
