"""Restarted GMRES: exported symbols, constants and the arguments of its C ABI -- host only (sparsh_setup_host), no GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import ROOT

QUIET = dict(print_setup=0, print_solve=0)


def test_symbols_are_exported():
    out = subprocess.run(["nm", "-D", "-C", os.path.join(ROOT, "sparsh_amg_amd", "libsparsh_amg.so")], capture_output=True, text=True,
                         check=True).stdout
    for name in ("Solver_GMRES_1(", "Solver_PGMRES_1(", "sparsh_set_gmres", "sparsh_gmres_info", "sparsh_op_precond"):
        assert re.search(r" T " + re.escape(name), out), name


def test_header_python_constants_and_methods_agree():
    with open(os.path.join(ROOT, "include", "sparsh_amg.h")) as f:
        header = f.read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define SPARSH_(GMRES|PGMRES) (\d+)", header, re.M)}
    assert codes == {"GMRES": 5, "PGMRES": 6}
    assert (sa.SPARSH_GMRES, sa.SPARSH_PGMRES) == (5, 6)
    assert sa.METHODS["gmres"] == 5 and sa.METHODS["pgmres"] == 6
    assert sorted(sa.METHODS.values()) == list(range(7))
    assert callable(sa.Solver_GMRES_1) and callable(sa.Solver_PGMRES_1)
    for decl in ("void Solver_GMRES_1(sp_matrix_mg &A, double *&b, double *&x);", "void Solver_PGMRES_1(sp_matrix_mg &A, double *&b, double *&x);"):
        with open(os.path.join(ROOT, "include", "AMG.hpp")) as f:
            assert decl in f.read()


def test_set_gmres_and_info_on_a_host_only_handle():
    rp, ci, v = problems.poisson2d(30)
    A = sa.sp_matrix_mg(rp, ci, v)
    assert A.gmres_info() == dict(restart=30, basis_bytes=0)  # before any setup
    A.setup(sa.default_params(**QUIET), host_only=True)
    h = A._h
    for m in (1, 30, 64):
        assert sa.lib.sparsh_set_gmres(h, m) == sa.SPARSH_OK
        assert A.gmres_info() == dict(restart=m, basis_bytes=0)
    assert sa.lib.sparsh_set_gmres(h, 0) == sa.SPARSH_OK
    assert A.gmres_info()["restart"] == 30
    A.set_gmres(12)
    for bad in (-1, 65):
        assert sa.lib.sparsh_set_gmres(h, bad) == sa.SPARSH_EINVAL
        assert b"restart" in sa.lib.sparsh_last_error()
        assert A.gmres_info()["restart"] == 12  # a refused call changes nothing
    # any pointer may be NULL
    m, nbytes = C.c_int(), C.c_long(-1)
    assert sa.lib.sparsh_gmres_info(h, None, None) == sa.SPARSH_OK
    assert sa.lib.sparsh_gmres_info(h, C.byref(m), None) == sa.SPARSH_OK and m.value == 12
    assert sa.lib.sparsh_gmres_info(h, None, C.byref(nbytes)) == sa.SPARSH_OK and nbytes.value == 0
    assert sa.lib.sparsh_set_gmres(None, 5) == sa.SPARSH_EINVAL


def test_gmres_needs_the_device_setup():
    rp, ci, v = problems.poisson2d(30)
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET), host_only=True)
    n = len(rp) - 1
    b, x, hist, it = np.ones(n), np.zeros(n), np.zeros(8), C.c_int()
    for method in (sa.SPARSH_PGMRES, sa.SPARSH_GMRES):
        assert sa.lib.sparsh_solve(A._h, method, sa._dp(b), sa._dp(x), sa._dp(hist), 8, C.byref(it)) == sa.SPARSH_ESTATE
    assert sa.lib.sparsh_op_precond(A._h, sa._dp(b), sa._dp(x)) == sa.SPARSH_ESTATE
    # the stepwise interface stays with CG and PCG
    assert sa.lib.sparsh_krylov_init_dev(A._h, sa.SPARSH_PGMRES, None, None) in (sa.SPARSH_EINVAL, sa.SPARSH_ESTATE)
