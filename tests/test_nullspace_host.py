"""Constant null space (SPARSH_NULLSPACE_CONSTANT), host half: defects, refusals, the pinned coarsest operator and the byte image.
No device needed: everything goes through setup(host_only=True)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems

QUIET = dict(print_setup=0, print_solve=0)
LIMITS = dict(limit_upper=300, limit_lower=100)


def neumann_handle(kind="constant", dims=(12, 10, 9), **kw):
    rp, ci, v = problems.poisson3d_neumann(*dims)
    A = sa.sp_matrix_mg(rp, ci, v)
    if kind is not None:
        A.set_nullspace(kind)
    return A.setup(sa.default_params(**QUIET, **LIMITS, **kw), host_only=True)


def pinned(AL, row):
    """AL with row and column `row` replaced by the unit row and column"""
    M = AL.toarray()
    M[row, :] = 0.0
    M[:, row] = 0.0
    M[row, row] = 1.0
    return M


def test_generator_is_the_neumann_stencil():
    rp, ci, v = problems.poisson3d_neumann(5, 4, 3)
    M = sp.csr_matrix((v, ci, rp))
    assert M.shape == (60, 60) and abs(M - M.T).max() == 0
    assert np.all(M @ np.ones(60) == 0.0)
    off = M - sp.diags(M.diagonal())
    assert set(np.unique(off.data)) == {-1.0}
    assert sorted(set(M.diagonal())) == [3.0, 4.0, 5.0, 6.0]
    assert all(np.all(np.diff(ci[rp[i]:rp[i + 1]]) > 0) for i in range(60))  # sorted columns
    r1, c1, v1 = problems.poisson3d_neumann(4)
    assert len(r1) - 1 == 64


def test_levels_pinned_row_and_defects():
    A = neumann_handle()
    assert [A.level_info(l)["nrow"] for l in range(A.nlevels)] == [1080, 540, 270]
    info = A.nullspace_info()
    assert info == dict(kind="constant", pinned_row=269, row_defect=0.0, col_defect=0.0)


def test_coarse_inverse_is_the_inverse_of_the_pinned_matrix():
    A = neumann_handle()
    AL = A.level_scipy(A.nlevels - 1)
    assert np.abs(AL @ np.ones(270)).max() == 0.0  # A_L itself stays singular and untouched on the level
    inv = A.coarse_inverse()
    M = pinned(AL, 269)
    assert np.abs(inv @ M - np.eye(270)).max() <= 1e-11
    assert np.abs(M @ inv - np.eye(270)).max() <= 1e-11
    # a condition: the inverse of the pinned matrix is O(n) in size; the "inverse" of the unpinned one is about 8e13
    assert np.abs(inv).max() < 1e4


def test_single_level_hierarchy_is_pinned_too():
    rp, ci, v = problems.poisson3d_neumann(6, 5, 4)
    A = sa.sp_matrix_mg(rp, ci, v).set_nullspace("constant").setup(sa.default_params(**QUIET), host_only=True)
    assert A.nlevels == 1 and A.nullspace_info()["pinned_row"] == 119
    M = pinned(A.level_scipy(0), 119)
    assert np.abs(A.coarse_inverse() @ M - np.eye(120)).max() <= 1e-11


def test_dirichlet_matrix_is_refused_with_its_defect():
    rp, ci, v = problems.poisson3d(8)
    A = sa.sp_matrix_mg(rp, ci, v).set_nullspace("constant")
    with pytest.raises(sa.SparshError) as e:
        A.setup(sa.default_params(**QUIET), host_only=True)
    assert e.value.code == sa.SPARSH_EINVAL
    msg = str(e.value)
    # corner rows: |6 - 3| / (6 + 3)
    assert "constant vector is not in the null space" in msg and "3.333e-01" in msg
    assert A.nullspace_info()["kind"] == "none"  # no hierarchy was built


def test_unsymmetric_column_defect_is_refused():
    rp, ci, v = problems.poisson3d_neumann(6)
    M = sp.csr_matrix((v, ci, rp)).tolil()
    M[0, 1] = -2.0  # with the diagonal raised by one every row still sums to zero: only the columns 0 and 1 are off
    M[0, 0] = M[0, 0] + 1.0
    M = M.tocsr()
    M.sort_indices()
    assert np.abs(M @ np.ones(216)).max() == 0.0
    A = sa.sp_matrix_mg(M.indptr.astype(np.int32), M.indices.astype(np.int32), M.data.copy()).set_nullspace("constant")
    with pytest.raises(sa.SparshError) as e:
        A.setup(sa.default_params(**QUIET), host_only=True)
    assert e.value.code == sa.SPARSH_EINVAL and "column defect" in str(e.value)


def test_refusals_name_the_null_space():
    rp, ci, v = problems.poisson3d_neumann(12, 10, 9)
    for kw in (dict(coarsening=1), dict(precond_fp32=1)):
        A = sa.sp_matrix_mg(rp, ci, v).set_nullspace("constant")
        with pytest.raises(sa.SparshError) as e:
            A.setup(sa.default_params(**QUIET, **LIMITS, **kw), host_only=True)
        assert e.value.code == sa.SPARSH_EINVAL and "null space" in str(e.value), kw
        # ... and the same parameters are fine without a null space
        A.set_nullspace("none").setup(sa.default_params(**QUIET, **LIMITS, **kw), host_only=True)
        A.close()
    group = sa.comm_group_create(2)
    try:
        P = sa.sp_matrix_mg(rp, ci, v).set_nullspace("constant")
        P.comm_init_group(group, 0)
        with pytest.raises(sa.SparshError) as e:
            P.setup(sa.default_params(**QUIET, **LIMITS), host_only=True)
        assert e.value.code == sa.SPARSH_EINVAL and "null space" in str(e.value)
        # the full setup refuses it before it looks for a device
        assert sa.lib.sparsh_setup(P._h, C.byref(sa.default_params(**QUIET, **LIMITS))) == sa.SPARSH_EINVAL
        assert b"null space" in sa.lib.sparsh_last_error()
        P.close()
    finally:
        sa.comm_group_destroy(group)


def test_solve_multi_is_refused_on_a_constant_handle():
    A = neumann_handle()
    n = A.nrow
    B, X = np.ones((n, 2), order="F"), np.zeros((n, 2), order="F")
    with pytest.raises(sa.SparshError) as e:
        A.solve_multi("pcg", B, X)
    assert e.value.code == sa.SPARSH_EINVAL and "null space" in str(e.value)
    with pytest.raises(sa.SparshError) as e:
        A.op_precond_multi(B)
    assert e.value.code == sa.SPARSH_EINVAL and "null space" in str(e.value)


def test_bad_kind_changes_nothing_and_info_takes_null_pointers():
    A = neumann_handle()
    for bad in (-1, 2, 7):
        assert sa.lib.sparsh_set_nullspace(A._h, bad) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_set_nullspace(None, 1) == sa.SPARSH_EINVAL
    A.setup(sa.default_params(**QUIET, **LIMITS), host_only=True)  # still CONSTANT
    assert A.nullspace_info()["pinned_row"] == 269
    assert sa.lib.sparsh_nullspace_info(A._h, None, None, None, None) == sa.SPARSH_OK
    row = C.c_int(-5)
    assert sa.lib.sparsh_nullspace_info(A._h, None, C.byref(row), None, None) == sa.SPARSH_OK and row.value == 269
    assert sa.lib.sparsh_nullspace_info(None, None, None, None, None) == sa.SPARSH_EINVAL
    fresh = sa.sp_matrix_mg(*problems.poisson3d_neumann(4))
    assert fresh.nullspace_info() == dict(kind="none", pinned_row=-1, row_defect=0.0, col_defect=0.0)


def test_none_restores_an_ordinary_setup():
    A = neumann_handle()
    inv_c = A.coarse_inverse()
    A.set_nullspace("none").setup(sa.default_params(**QUIET, **LIMITS), host_only=True)
    assert A.nullspace_info() == dict(kind="none", pinned_row=-1, row_defect=0.0, col_defect=0.0)
    B = neumann_handle(kind=None)
    assert np.array_equal(A.coarse_inverse(), B.coarse_inverse())  # the unpinned "inverse" of today, bit for bit
    assert not np.array_equal(A.coarse_inverse(), inv_c)
    assert A.hierarchy_roundtrip() == B.hierarchy_roundtrip()


def test_hierarchy_round_trip_carries_the_kind():
    A = neumann_handle()
    nbytes = A.hierarchy_roundtrip()
    assert nbytes == neumann_handle(kind="none").hierarchy_roundtrip()  # the kind rides in an existing word of the header
    for cut in (0, 8, nbytes // 2, nbytes - 1):
        with pytest.raises(sa.SparshError):
            A.hierarchy_roundtrip(cut)
    # above dense_limit the image holds no inverse; the kind still travels
    A = neumann_handle(dense_limit=100)
    assert A.nullspace_info()["pinned_row"] == 269
    assert A.hierarchy_roundtrip() > 0
