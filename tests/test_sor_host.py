"""Colouring of the multicolour SOR smoother and its C ABI arguments -- host only (sparsh_setup_host), no GPU.

Contract ("Multicolour SOR smoother"): greedy first-fit over the rows in ascending order on the pattern of
A + A^T without the diagonal, colours numbered from 1.  For a structurally symmetric A the classes are those of the
reference's color_matrix_and_reorder (src/AMG_cpu_matrix.cpp:81-130), which looks at row i's own columns only.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import load_c0

QUIET = dict(print_setup=0, print_solve=0)


def reference_greedy(rp, ci):
    """color_matrix_and_reorder restated: row i takes the smallest colour >= 1 that none of its own (already coloured)
    columns holds."""
    n = len(rp) - 1
    color = np.zeros(n, dtype=np.int64)
    for i in range(n):
        used = set(color[ci[rp[i]:rp[i + 1]]].tolist())
        c = 1
        while c in used:
            c += 1
        color[i] = c
    return color


def coupled_pairs(rp, ci):
    """(i, j), i != j, of the pattern of A + A^T"""
    n = len(rp) - 1
    A = sp.csr_matrix((np.ones(len(ci)), ci, rp), shape=(n, n))
    S = (A + A.T).tocoo()
    off = S.row != S.col
    return S.row[off], S.col[off]


def unsymmetric_grid(m=64):
    """5-point grid operator whose every third row keeps only its diagonal and its east / south neighbours: structurally
    unsymmetric, and a row that looks at its own columns only sees none of its (already coloured) west / north
    neighbours, which refer to it"""
    rp, ci, v = problems.poisson2d(m)
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    keep = ~((ci < rows) & (rows % 3 == 0))
    rp2 = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=n))]).astype(np.int32)
    return rp2, ci[keep].astype(np.int32), v[keep]


def inputs():
    rp, ci, v, _ = load_c0()
    yield "c0", (rp, ci, v)
    yield "poisson2d", problems.poisson2d(120)
    yield "poisson3d", problems.poisson3d(24)
    yield "fem_unstructured", problems.fem_unstructured(20000)
    yield "random_spd", problems.random_spd(6000)


INPUTS = dict(inputs())


def host_handle(rp, ci, v, **kw):
    return sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, **kw), host_only=True)


@pytest.mark.parametrize("name", list(INPUTS))
def test_colour_classes_are_independent_and_match_the_reference_greedy(name):
    A = host_handle(*INPUTS[name])
    for l in range(A.nlevels):
        rp, ci, _, _ = A.level_csr(l)
        nc, counts, color = A.level_colors(l)
        assert color.min() == 1 and color.max() == nc and counts.sum() == len(rp) - 1
        assert np.array_equal(counts, np.bincount(color, minlength=nc + 1)[1:])
        i, j = coupled_pairs(rp, ci)
        assert not np.any(color[i] == color[j]), f"level {l}: two coupled rows share a colour"
        # structurally symmetric levels: the reference's greedy gives the same classes
        assert np.array_equal(color, reference_greedy(rp, ci)), f"level {l}"


def test_unsymmetric_pattern_gets_independent_classes():
    rp, ci, v = unsymmetric_grid()
    A = host_handle(rp, ci, v)
    i, j = coupled_pairs(rp, ci)
    row_only = reference_greedy(rp, ci)
    assert np.any(row_only[i] == row_only[j])  # the row-only greedy would update two coupled rows at once
    for l in range(A.nlevels):
        lrp, lci, _, _ = A.level_csr(l)
        _, _, color = A.level_colors(l)
        li, lj = coupled_pairs(lrp, lci)
        assert not np.any(color[li] == color[lj]), f"level {l}"


@pytest.mark.parametrize("gen", [lambda: problems.poisson2d(40), lambda: problems.poisson3d(14)], ids=["5pt", "7pt"])
def test_lexicographic_grids_are_red_black(gen):
    rp, ci, v = gen()
    A = host_handle(rp, ci, v)
    nc, counts, color = A.level_colors(0)
    assert nc == 2
    n = len(rp) - 1
    assert counts.tolist() == [(n + 1) // 2, n // 2]


def test_colours_need_the_host_setup():
    rp, ci, v = problems.poisson2d(16)
    A = sa.sp_matrix_mg(rp, ci, v)
    nc = C.c_int()
    assert sa.lib.sparsh_level_colors(A._h, 0, C.byref(nc), None) == sa.SPARSH_ESTATE


def test_smoother_argument_errors():
    rp, ci, v = problems.poisson2d(30)
    A = host_handle(rp, ci, v)
    h = A._h
    assert sa.lib.sparsh_set_smoother(h, 2, 0, 0) == sa.SPARSH_EINVAL  # unknown kind
    assert sa.lib.sparsh_set_smoother(h, -1, 0, 0) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_set_smoother(h, sa.SPARSH_SMOOTH_SOR, -1, 0) == sa.SPARSH_EINVAL  # negative sweeps
    assert sa.lib.sparsh_set_smoother(h, sa.SPARSH_SMOOTH_SOR, 0, 2) == sa.SPARSH_EINVAL  # unknown order
    with pytest.raises(KeyError):
        A.set_smoother("gauss-seidel")
    # PCG needs the symmetric cycle: refused as a bad argument, before (and whatever) the device state
    A.set_smoother("sor", 0, "forward")
    n = len(rp) - 1
    b, x, hist, it = np.ones(n), np.zeros(n), np.zeros(8), C.c_int()
    rc = sa.lib.sparsh_solve(h, sa.SPARSH_PCG, sa._dp(b), sa._dp(x), sa._dp(hist), 8, C.byref(it))
    assert rc == sa.SPARSH_EINVAL and b"SYMMETRIC" in sa.lib.sparsh_last_error()
    rc = sa.lib.sparsh_krylov_init_dev(h, sa.SPARSH_PCG, None, None)
    assert rc == sa.SPARSH_EINVAL
    # the other combinations pass the argument check (and then need sparsh_setup)
    A.set_smoother("sor", 0, "symmetric")
    assert sa.lib.sparsh_solve(h, sa.SPARSH_PCG, sa._dp(b), sa._dp(x), sa._dp(hist), 8, C.byref(it)) == sa.SPARSH_ESTATE
    A.set_smoother("sor", 3, "forward")
    assert sa.lib.sparsh_solve(h, sa.SPARSH_AMG, sa._dp(b), sa._dp(x), sa._dp(hist), 8, C.byref(it)) == sa.SPARSH_ESTATE
    A.set_smoother("jacobi")
    assert sa.lib.sparsh_solve(h, sa.SPARSH_PCG, sa._dp(b), sa._dp(x), sa._dp(hist), 8, C.byref(it)) == sa.SPARSH_ESTATE


def test_sor_refuses_the_fp32_preconditioner():
    rp, ci, v = problems.poisson2d(30)
    A = host_handle(rp, ci, v, precond_fp32=1)
    with pytest.raises(sa.SparshError) as e:
        A.set_smoother("sor", 0, "symmetric")
    assert e.value.code == sa.SPARSH_EINVAL
    A.set_smoother("jacobi")  # Jacobi stays available
