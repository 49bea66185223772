"""The pivoting paths of the three device Gauss-Jordan inverters of the coarse direct solvers.  GPU box only.

nd_invert_kernel (pivot blocks up to 80 rows in one workgroup's LDS), nd_gj_* (larger pivot blocks, one launch per step, two
ping-pong buffers) and bt_* (diagonal blocks of the block-tridiagonal form) pick the pivot of a step by partial pivoting.  On the
operators of test_gpu_coarse.py the pivot is the diagonal row but for a dozen isolated steps of two cases, so the row interchange,
the source-row redirection s = (i == p ? k : i), the lowest-index tie rule and the final column un-permutation hardly run there, and
a wrong order of the column map or a tie decided differently by two workgroups goes unnoticed.  The operators of
coarse_pivot_inputs.py make them run (test_host_setup.py shows it on the CPU), coarse_info() counts the pivot steps and the
interchanges the kernels took, and the solutions are compared with exactly known ones.
"""
import numpy as np
import pytest
import scipy.sparse as sp

import coarse_pivot_inputs as cp
import sparsh_amg_amd as sa
from sparsh_amg_amd import problems

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
ONE_LEVEL = dict(max_levels=1, coarse_limit=1 << 30, limit_upper=1 << 30)  # the whole matrix is the "coarsest level"


def _handle(csr, form, dense_limit, nd=(0, -1, -1), interface=True):
    A = sa.sp_matrix_mg(*csr).set_coarse_form(form, *nd)
    if form == "bt":
        A.set_coarse_interface(interface)
    return A.setup(sa.default_params(**QUIET, **ONE_LEVEL, dense_limit=dense_limit))


def _class_rows(sizes):
    return sum(s for s in sizes if s <= cp.LDS_LIMIT), sum(s for s in sizes if s > cp.LDS_LIMIT)


@pytest.fixture(scope="module")
def cliques():
    """The blocks, their CSR, an integer solution and its exact right-hand side; per block the error of the two references."""
    blocks = cp.clique_blocks()
    n = sum(cp.CLIQUE_SIZES)
    x_true = cp.integer_vector(n, 7)
    b = np.concatenate([Bk @ x_true[r0:r0 + Bk.shape[0]] for Bk, r0 in zip(blocks, np.cumsum((0,) + cp.CLIQUE_SIZES[:-1]))])
    ref_err = []
    r0 = 0
    for Bk in blocks:
        s = Bk.shape[0]
        xt, bb = x_true[r0:r0 + s], b[r0:r0 + s]
        inv, swaps, singular = cp.gauss_jordan_inverse(Bk)
        assert not singular
        err = lambda x: np.abs(x - xt).max() / np.abs(xt).max()  # noqa: E731
        ref_err.append(max(err(inv @ bb), err(np.linalg.solve(Bk, bb)), 2.0 ** -52))
        r0 += s
    return blocks, cp.block_diagonal_csr(blocks), x_true, b, ref_err


@pytest.mark.parametrize("nd", [(0, -1, -1), (16, 0, 0)], ids=["default_dissection", "plain_bisection"])
def test_nd_cliques_every_block_boundary_with_row_interchanges(cliques, nd):
    """Dense integer blocks of 1 .. 257 rows, each one tree node: pivot blocks on the LDS limit (80 | 81), around a wave (63, 64,
    65), off the 8 rows of a workgroup (81, 129, 257), past 256 columns (257), both parities of the ping-pong; nearly every step
    interchanges rows and exact magnitude ties are frequent.  Per block max|x - x_true| / max|x_true| of the device must stay
    within 8 x the larger of the same error of a numpy restatement of the documented Gauss-Jordan and of np.linalg.solve (the
    device differs from the restatement in the order of the final gathered dot only, which moves single roundings; any logic
    error gives O(1))."""
    blocks, csr, x_true, b, ref_err = cliques
    A = _handle(csr, "nd", 500, nd)
    try:
        info = A.coarse_info()
        assert info["form"] == "nested_dissection" and info["rows"] == len(b)
        assert info["nd_max_pivot"] == 257 and info["nd_nodes"] == len(blocks) and info["nd_levels"] == 1
        assert (info["pivot_steps_lds"], info["pivot_steps_chip"]) == _class_rows(cp.CLIQUE_SIZES)
        assert info["row_swaps_lds"] > 0 and info["row_swaps_chip"] > 0
        x = A.op_coarse(b)
        ratios = []
        r0 = 0
        for Bk, ref in zip(blocks, ref_err):
            s = Bk.shape[0]
            xt = x_true[r0:r0 + s]
            ratios.append(np.abs(x[r0:r0 + s] - xt).max() / np.abs(xt).max() / ref)
            r0 += s
        print("row interchanges (LDS, chip):", info["row_swaps_lds"], info["row_swaps_chip"])
        print("device error / reference error per block:", " ".join(f"{s}:{r:.2f}" for s, r in zip(cp.CLIQUE_SIZES, ratios)))
        assert max(ratios) <= 8.0, list(zip(cp.CLIQUE_SIZES, ratios))
        assert np.array_equal(A.op_coarse(b), x)
    finally:
        A.close()


def test_nd_hadamard_blocks_are_inverted_bit_for_bit():
    """Sylvester Hadamard blocks with shuffled rows: every intermediate of the pivoted Gauss-Jordan is a dyadic rational, the inverse
    is (H^T / n)[:, perm] exactly and an integer right-hand side has an exact solution whatever the order of the sums.  A wrong
    column map, a wrong source row or the wrong result buffer cannot hide in a tolerance here."""
    blocks, perms = cp.hadamard_blocks()
    csr = cp.block_diagonal_csr(blocks)
    n = sum(cp.HADAMARD_SIZES)
    A = _handle(csr, "nd", 200)
    try:
        info = A.coarse_info()
        assert info["form"] == "nested_dissection" and info["nd_max_pivot"] == 256 and info["nd_nodes"] == 3
        assert (info["pivot_steps_lds"], info["pivot_steps_chip"]) == _class_rows(cp.HADAMARD_SIZES)
        assert info["row_swaps_lds"] > 0 and info["row_swaps_chip"] > 0
        B = np.stack([cp.integer_vector(n, 21), cp.integer_vector(n, 22) * 3.0, np.ones(n)], axis=1)
        exact = np.empty_like(B)
        r0 = 0
        for Bk, perm in zip(blocks, perms):
            s = Bk.shape[0]
            exact[r0:r0 + s] = cp.hadamard_exact_inverse(Bk, perm) @ B[r0:r0 + s]  # +-1/n times integers: exact in any order
            r0 += s
        assert np.array_equal(sp.csr_matrix((csr[2], csr[1], csr[0]), shape=(n, n)) @ exact, B)
        for c in range(B.shape[1]):
            assert np.array_equal(A.op_coarse(B[:, c]), exact[:, c]), c
        assert np.array_equal(A.op_coarse_multi(B), exact)
    finally:
        A.close()


def _scaled_system(gen, seed):
    rp, ci, v = cp.scale_rows(*gen())
    n = len(rp) - 1
    S = sp.csr_matrix((v, ci, rp), shape=(n, n))
    x_true = cp.integer_vector(n, seed)
    return (rp, ci, v), S, x_true, S @ x_true   # power-of-two scaling, integer x_true: b is exact


def _check_scaled_solve(A, S, x_true, b):
    x = A.op_coarse(b)
    assert np.linalg.norm(x - x_true) <= 1e-11 * np.linalg.norm(x_true)
    assert np.linalg.norm(b - S @ x) <= 1e-11 * np.linalg.norm(b)
    assert np.array_equal(A.op_coarse(b), x)


@pytest.mark.parametrize("name,gen,nd,classes", [
    ("p3d_12_default", lambda: problems.poisson3d(12), (0, -1, -1), ("chip",)),            # interchanges in the large top separator
    ("p3d_14_leaf16_no_merging", lambda: problems.poisson3d(14), (16, 0, 0), ("lds", "chip")),   # a deep tree of small blocks
    ("p2d_80_leaf16", lambda: problems.poisson2d(80), (16, -1, -1), ("lds", "chip")),
])
def test_nd_row_scaled_grids_through_a_whole_tree(name, gen, nd, classes):
    """A seeded third of the rows times 8: the multi-level case, where extend-add, the three products and both passes of the solve
    see pivot blocks whose inversion interchanged rows."""
    csr, S, x_true, b = _scaled_system(gen, 31)
    A = _handle(csr, "nd", 1000, nd)
    try:
        info = A.coarse_info()
        assert info["form"] == "nested_dissection" and info["nd_levels"] >= 2
        assert info["pivot_steps_lds"] + info["pivot_steps_chip"] == len(b)
        for c in classes:
            assert info["pivot_steps_" + c] > 0 and info["row_swaps_" + c] > 0, (name, info)
        print(name, "row interchanges (LDS, chip):", info["row_swaps_lds"], info["row_swaps_chip"])
        _check_scaled_solve(A, S, x_true, b)
    finally:
        A.close()


@pytest.mark.parametrize("interface", [True, False], ids=["interface_form", "plain_chain"])
@pytest.mark.parametrize("name,gen", [
    ("p2d_100_window_128", lambda: problems.poisson2d(100)),
    ("p3d_21_ragged_last_block", lambda: problems.poisson3d(21)),
])
def test_bt_row_scaled_grids(name, gen, interface):
    """The block-tridiagonal form with in-block interchanges in every diagonal block, the ragged last block included."""
    csr, S, x_true, b = _scaled_system(gen, 32)
    A = _handle(csr, "bt", 2000, interface=interface)
    try:
        info = A.coarse_info()
        assert info["form"] == "block_tridiagonal" and info["nblocks"] >= 2
        assert (info["window"] > 0) == (interface and "p2d" in name)
        assert info["pivot_steps_chip"] == len(b) and info["row_swaps_chip"] > 0
        assert info["pivot_steps_lds"] == 0 and info["row_swaps_lds"] == 0
        print(name, "row interchanges:", info["row_swaps_chip"])
        _check_scaled_solve(A, S, x_true, b)
    finally:
        A.close()


def _solve_healthy(blocks, form, dense_limit):
    n = sum(Bk.shape[0] for Bk in blocks)
    x_true = cp.integer_vector(n, 41)
    S = sp.block_diag(blocks).tocsr()
    b = S @ x_true
    A = _handle(cp.block_diagonal_csr(blocks), form, dense_limit)
    try:
        x = A.op_coarse(b)
        assert np.linalg.norm(x - x_true) <= 1e-11 * np.linalg.norm(x_true)
        return x
    finally:
        A.close()


@pytest.mark.parametrize("form,rows", [("nd", 2), ("nd", 96), ("bt", 64)], ids=["nd_lds_2_rows", "nd_chip_96_rows", "bt_64_rows"])
def test_exact_zero_pivot_on_the_device_is_reported_as_singular(form, rows):
    """A clique with two equal rows among healthy cliques: the first pivot is a power of two, so the twin row becomes exactly zero
    and the block's last step meets a pivot of exactly 0 (1 / 0 = inf: nothing is dereferenced).  Setup must fail with
    SPARSH_ENUMERIC, and a healthy handle afterwards must set up and solve as it did before."""
    if form == "nd":
        healthy = cp.clique_blocks((5, rows, 70, 100), seed=13)
        dense_limit = 100
    else:
        healthy = cp.clique_blocks((64, 64), seed=13)   # blocks of 64 rows after RCM: one clique each
        dense_limit = 64
    sick = list(healthy)
    sick[1] = cp.singular_clique(rows)
    x_before = _solve_healthy(healthy, form, dense_limit)
    A = sa.sp_matrix_mg(*cp.block_diagonal_csr(sick)).set_coarse_form(form)
    try:
        with pytest.raises(sa.SparshError) as e:
            A.setup(sa.default_params(**QUIET, **ONE_LEVEL, dense_limit=dense_limit))
        assert e.value.code == sa.SPARSH_ENUMERIC and "singular" in str(e.value), str(e.value)
    finally:
        A.close()
    assert np.array_equal(_solve_healthy(healthy, form, dense_limit), x_before)
