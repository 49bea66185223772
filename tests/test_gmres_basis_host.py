"""Storage precision of the GMRES basis (sparsh_set_gmres_basis / sparsh_gmres_basis): exported symbols, constants and the
arguments of the C ABI -- host only (sparsh_setup_host), no GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import ROOT

QUIET = dict(print_setup=0, print_solve=0)


def handle(setup):
    rp, ci, v = problems.poisson2d(30)
    A = sa.sp_matrix_mg(rp, ci, v)
    return A.setup(sa.default_params(**QUIET), host_only=True) if setup else A


def precision(A):
    p = C.c_int(-7)
    assert sa.lib.sparsh_gmres_basis(A._h, C.byref(p)) == sa.SPARSH_OK
    return p.value


def test_symbols_and_constants():
    out = subprocess.run(["nm", "-D", "-C", os.path.join(ROOT, "sparsh_amg_amd", "libsparsh_amg.so")], capture_output=True, text=True,
                         check=True).stdout
    for name in ("sparsh_set_gmres_basis", "sparsh_gmres_basis"):
        assert re.search(r" T " + re.escape(name) + r"$", out, re.M), name
    with open(os.path.join(ROOT, "include", "sparsh_amg.h")) as f:
        header = f.read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"^#define SPARSH_BASIS_(FP64|FP32) (\d+)", header, re.M)}
    assert codes == {"FP64": 0, "FP32": 1}
    assert (sa.SPARSH_BASIS_FP64, sa.SPARSH_BASIS_FP32) == (0, 1)
    assert sa.GMRES_BASES == {"fp64": 0, "fp32": 1}
    for decl in ("int sparsh_set_gmres_basis(sparsh_handle h, int precision);", "int sparsh_gmres_basis(sparsh_handle h, int *precision);"):
        assert decl in header


@pytest.mark.parametrize("setup", [False, True], ids=["before_setup", "host_only_setup"])
def test_set_and_read_back(setup):
    A = handle(setup)
    h = A._h
    assert precision(A) == sa.SPARSH_BASIS_FP64  # the default
    A.set_gmres(12)
    for p in (1, 0, 1):
        assert sa.lib.sparsh_set_gmres_basis(h, p) == sa.SPARSH_OK
        assert precision(A) == p
        assert A.gmres_info()["restart"] == 12  # the restart length is left alone
        assert A.gmres_info()["basis_bytes"] == 0  # nothing is held until a solve
    for bad in (-1, 2):
        assert sa.lib.sparsh_set_gmres_basis(h, bad) == sa.SPARSH_EINVAL
        assert b"precision" in sa.lib.sparsh_last_error()
        assert precision(A) == 1 and A.gmres_info()["restart"] == 12  # a refused call changes nothing
    # the restart length does not touch the precision either
    assert sa.lib.sparsh_set_gmres(h, 7) == sa.SPARSH_OK
    assert precision(A) == 1 and A.gmres_info()["restart"] == 7
    assert sa.lib.sparsh_gmres_basis(h, None) == sa.SPARSH_OK  # the pointer may be NULL
    assert sa.lib.sparsh_set_gmres_basis(None, 1) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_gmres_basis(None, None) == sa.SPARSH_EINVAL


def test_python_interface():
    A = handle(True)
    assert A.gmres_basis() == "fp64"
    assert A.gmres_info() == dict(restart=30, basis_bytes=0)
    assert A.set_gmres(9, basis="fp32") is A
    assert A.gmres_basis() == "fp32"
    assert A.gmres_info() == dict(restart=9, basis_bytes=0, basis="fp32")
    A.set_gmres(11)  # basis=None leaves the precision alone
    assert A.gmres_info() == dict(restart=11, basis_bytes=0, basis="fp32")
    A.set_gmres(basis="fp64")  # restart=0: the default length
    assert A.gmres_basis() == "fp64"
    assert A.gmres_info() == dict(restart=30, basis_bytes=0)
    with pytest.raises(KeyError):
        A.set_gmres(basis="fp16")
    with pytest.raises(sa.SparshError) as e:
        A.set_gmres(basis=2)
    assert e.value.code == sa.SPARSH_EINVAL
    assert A.gmres_basis() == "fp64"


def test_bench_op_of_the_float_basis_needs_the_device_setup():
    A = handle(True).set_gmres(basis="fp32")
    sec = C.c_double()
    assert sa.lib.sparsh_bench_op(A._h, 15, 0, 1, C.byref(sec)) == sa.SPARSH_ESTATE
