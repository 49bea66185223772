"""Argument and state errors of the block entry points (sparsh_solve_multi, sparsh_solve_multi_dev, sparsh_multi_info): every
SPARSH_EINVAL case is reported without a device and before the readiness check, SPARSH_ESTATE before sparsh_setup.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems

QUIET = dict(print_setup=0, print_solve=0)
DP, IP = C.POINTER(C.c_double), C.POINTER(C.c_int)


def raw_solve_multi(A, method, nrhs, B, ldb, X, ldx, hist_cap=4, iters=True, status=True, dev=False):
    """the C entry point itself: B / X numpy arrays or None (a NULL pointer)"""
    hist = np.zeros((8, hist_cap))
    it, st = np.zeros(8, dtype=np.int32), np.zeros(8, dtype=np.int32)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p if dev else DP)  # noqa: E731
    args = [A._h, method, nrhs, ptr(B), ldb, ptr(X), ldx]
    if dev:
        args.append(0)
    args += [hist.ctypes.data_as(DP), hist_cap, it.ctypes.data_as(IP) if iters else None, st.ctypes.data_as(IP) if status else None]
    if dev:
        args.append(None)
    return (sa.lib.sparsh_solve_multi_dev if dev else sa.lib.sparsh_solve_multi)(*args)


@pytest.fixture(scope="module")
def problem():
    rp, ci, v = problems.poisson2d(40)
    n = len(rp) - 1
    return rp, ci, v, n, np.ones((n, 8), order="F"), np.zeros((n, 8), order="F")


@pytest.mark.parametrize("dev", [False, True])
@pytest.mark.parametrize("prepared", ["fresh", "host_setup"])
def test_bad_arguments_are_einval_without_a_device(problem, dev, prepared):
    rp, ci, v, n, B, X = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    if prepared == "host_setup":
        A.setup(sa.default_params(**QUIET), host_only=True)
    pcg = sa.SPARSH_PCG
    for nrhs in (0, -1, 9, 100):
        assert raw_solve_multi(A, pcg, nrhs, B, n, X, n, dev=dev) == sa.SPARSH_EINVAL, nrhs
        assert b"nrhs" in sa.lib.sparsh_last_error()
    assert raw_solve_multi(A, pcg, 4, None, n, X, n, dev=dev) == sa.SPARSH_EINVAL
    assert raw_solve_multi(A, pcg, 4, B, n, None, n, dev=dev) == sa.SPARSH_EINVAL
    assert raw_solve_multi(A, pcg, 4, B, n, X, n, iters=False, dev=dev) == sa.SPARSH_EINVAL
    assert raw_solve_multi(A, pcg, 4, B, n, X, n, status=False, dev=dev) == sa.SPARSH_EINVAL
    assert b"NULL" in sa.lib.sparsh_last_error()
    assert raw_solve_multi(A, pcg, 4, B, n - 1, X, n, dev=dev) == sa.SPARSH_EINVAL
    assert raw_solve_multi(A, pcg, 4, B, n, X, n - 1, dev=dev) == sa.SPARSH_EINVAL
    assert raw_solve_multi(A, pcg, 4, B, 0, X, n, dev=dev) == sa.SPARSH_EINVAL
    assert b"ldb" in sa.lib.sparsh_last_error()
    for method in (sa.SPARSH_AMG, sa.SPARSH_CG, sa.SPARSH_BICG, sa.SPARSH_PBICG, sa.SPARSH_GMRES, sa.SPARSH_PGMRES, 17):
        assert raw_solve_multi(A, method, 4, B, n, X, n, dev=dev) == sa.SPARSH_EINVAL, method
        assert b"SPARSH_PCG" in sa.lib.sparsh_last_error()
    # valid arguments: the call order is what is wrong
    assert raw_solve_multi(A, pcg, 4, B, n, X, n, dev=dev) == sa.SPARSH_ESTATE
    assert raw_solve_multi(A, pcg, 1, B, n + 3, X, n + 5, dev=dev) == sa.SPARSH_ESTATE
    assert raw_solve_multi(A, pcg, 8, B, n, X, n, dev=dev) == sa.SPARSH_ESTATE


@pytest.mark.parametrize("dev", [False, True])
def test_handles_a_block_solve_cannot_run_on_are_einval(problem, dev):
    rp, ci, v, n, B, X = problem
    pcg = sa.SPARSH_PCG
    # a smoother other than Jacobi, selected before or after the host setup; Jacobi again lifts the refusal
    A = sa.sp_matrix_mg(rp, ci, v)
    for kind, order in (("sor", "symmetric"), ("sor", "forward"), ("chebyshev", "forward")):
        A.set_smoother(kind, 0, order)
        assert raw_solve_multi(A, pcg, 4, B, n, X, n, dev=dev) == sa.SPARSH_EINVAL, kind
        assert b"Jacobi" in sa.lib.sparsh_last_error()
    A.setup(sa.default_params(**QUIET), host_only=True)
    assert raw_solve_multi(A, pcg, 4, B, n, X, n, dev=dev) == sa.SPARSH_EINVAL
    A.set_smoother("jacobi")
    assert raw_solve_multi(A, pcg, 4, B, n, X, n, dev=dev) == sa.SPARSH_ESTATE
    # params.precond_fp32
    F = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, precond_fp32=1), host_only=True)
    assert raw_solve_multi(F, pcg, 4, B, n, X, n, dev=dev) == sa.SPARSH_EINVAL
    assert b"precond_fp32" in sa.lib.sparsh_last_error()
    # a handle with a multi-rank transport installed
    group = sa.comm_group_create(2)
    try:
        P = sa.sp_matrix_mg(rp, ci, v)
        P.comm_init_group(group, 0)
        assert raw_solve_multi(P, pcg, 4, B, n, X, n, dev=dev) == sa.SPARSH_EINVAL
        assert b"partitioned" in sa.lib.sparsh_last_error()
        P.close()
    finally:
        sa.comm_group_destroy(group)


def test_python_wrappers_raise_the_same_codes(problem):
    rp, ci, v, n, B, X = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    with pytest.raises(sa.SparshError) as e:
        A.solve_multi("pcg", B[:, :4], X[:, :4].copy())
    assert e.value.code == sa.SPARSH_ESTATE
    with pytest.raises(sa.SparshError) as e:
        A.solve_multi("pbicg", B[:, :4], X[:, :4].copy())
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:
        A.solve_multi("pcg", np.ones((n, 9)), np.zeros((n, 9)))
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:
        A.op_precond_multi(B[:, :3])
    assert e.value.code == sa.SPARSH_ESTATE
    with pytest.raises(sa.SparshError) as e:
        A.bench_op_multi("spmv_dot", 0, nrhs=0)
    assert e.value.code == sa.SPARSH_EINVAL


def test_multi_info_is_zero_on_a_fresh_handle(problem):
    rp, ci, v, n, _, _ = problem
    A = sa.sp_matrix_mg(rp, ci, v)
    assert A.multi_info() == dict(width=0, bytes=0)
    A.setup(sa.default_params(**QUIET), host_only=True)
    assert A.multi_info() == dict(width=0, bytes=0)
    assert sa.lib.sparsh_multi_info(None, None, None) == sa.SPARSH_EINVAL
