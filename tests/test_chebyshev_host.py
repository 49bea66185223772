"""Spectral bounds of the Chebyshev smoother and the C ABI arguments around it -- host only (sparsh_setup_host), no GPU.

Contract, per smoothed level (every level but the coarsest): gershgorin = max_i sum_j |a_ij| / |a_ii| with a
row's terms added in stored order; lanczos = the largest Ritz value of S = D^-1/2 A D^-1/2 after min(steps, n) steps of plain
Lanczos from the fixed start vector; lmax = min(1.1 * lanczos, gershgorin); lmin = lmax / ratio.  The true largest eigenvalue of S
comes from scipy's eigsh.
"""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems

QUIET = dict(print_setup=0, print_solve=0)


def inputs():
    yield "poisson3d", problems.poisson3d(24)
    yield "poisson2d", problems.poisson2d(120)
    yield "fem_unstructured", problems.fem_unstructured(20000)
    yield "random_spd", problems.random_spd(6000)


INPUTS = dict(inputs())


def host_handle(rp, ci, v, **kw):
    return sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, **kw), host_only=True)


def first_diagonal(rp, ci, v):
    """the first entry with col == row of every row (extract_diagonal), 0 where a row has none"""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    hit = np.flatnonzero(ci[: len(rows)] == rows)
    d = np.zeros(n)
    d[rows[hit][::-1]] = v[hit][::-1]
    return d


def numpy_gershgorin(rp, ci, v):
    """row sums of |a_ij| accumulated column by column over rows padded to one width: every row adds its terms one by one in
    stored order"""
    lens = np.diff(rp)
    W = max(int(lens.max()), 1)
    k = np.arange(W)
    on = k[None, :] < lens[:, None]
    idx = np.minimum(np.where(on, rp[:-1, None] + k[None, :], 0), len(v) - 1)
    pv = np.where(on, np.abs(v[idx]), 0.0)
    s = np.zeros(len(lens))
    for c in range(W):
        s = np.where(on[:, c], s + pv[:, c], s)
    return (s / np.abs(first_diagonal(rp, ci, v))).max()


def true_lambda_max(rp, ci, v):
    n = len(rp) - 1
    A = sp.csr_matrix((v, ci, rp), shape=(n, n))
    i = sp.diags(1.0 / np.sqrt(first_diagonal(rp, ci, v)))
    S = (i @ A @ i).tocsr()
    S = (S + S.T) * 0.5
    if n <= 400:
        return float(np.linalg.eigvalsh(S.toarray())[-1])
    return float(spla.eigsh(S, k=1, which="LA", tol=1e-12, ncv=min(n - 1, 60))[0][0])


@pytest.mark.parametrize("name", list(INPUTS))
def test_bounds_bracket_the_spectrum_on_every_smoothed_level(name):
    A = host_handle(*INPUTS[name], max_levels=6)
    assert A.nlevels >= 2
    for l in range(A.nlevels - 1):
        rp, ci, v, _ = A.level_csr(l)
        c = A.level_chebyshev(l)
        lam = true_lambda_max(rp, ci, v)
        print(f"{name} level {l}: n {len(rp) - 1} true {lam:.6f} lanczos {c['lanczos']:.6f} ({c['lanczos'] / lam:.4f}) "
              f"gershgorin {c['gershgorin']:.4f} lmax {c['lmax']:.6f} (margin {c['lmax'] / lam:.4f})")
        assert c["lanczos"] <= lam * (1 + 1e-10)
        assert c["lanczos"] >= 0.9 * lam
        assert c["lmax"] >= lam
        assert c["gershgorin"] == numpy_gershgorin(rp, ci, v)
        assert c["lmax"] == min(1.1 * c["lanczos"], c["gershgorin"])
        assert c["lmin"] == c["lmax"] / 30.0


def test_ratio_steps_and_forced_bound():
    A = host_handle(*INPUTS["fem_unstructured"])
    c0 = A.level_chebyshev(0)
    A.set_chebyshev(ratio=12.5)
    c1 = A.level_chebyshev(0)
    assert c1["lmax"] == c0["lmax"] and c1["lmin"] == c0["lmax"] / 12.5
    A.set_chebyshev(lanczos_steps=25)  # ratio back to the default, bounds dropped and estimated again
    c2 = A.level_chebyshev(0)
    assert c2["lmin"] == c2["lmax"] / 30.0
    assert c0["lanczos"] < c2["lanczos"] <= c0["gershgorin"]  # more steps: a larger Ritz value (it grows with the Krylov space)
    A.set_chebyshev_lmax(0, 3.25)
    c3 = A.level_chebyshev(0)
    assert c3["lmax"] == 3.25 and c3["lmin"] == 3.25 / 30.0 and c3["lanczos"] == c2["lanczos"] and c3["gershgorin"] == c2["gershgorin"]
    assert A.level_chebyshev(1)["lmax"] != 3.25
    A.set_chebyshev_lmax(0, 0.0)
    assert A.level_chebyshev(0) == c2
    A.set_chebyshev(lanczos_steps=10)
    assert A.level_chebyshev(0) == c0


def test_small_level_takes_n_steps():
    """min(steps, n): 64 steps on a 36-row level end at (or before) the 36th, with the exact largest eigenvalue"""
    rp, ci, v = problems.poisson2d(6)
    A = host_handle(rp, ci, v, limit_upper=20, limit_lower=10)
    assert A.nlevels >= 2
    A.set_chebyshev(lanczos_steps=64)
    c = A.level_chebyshev(0)
    lam = true_lambda_max(rp, ci, v)
    assert abs(c["lanczos"] - lam) <= 1e-10 * lam and c["lmax"] >= lam


@pytest.mark.parametrize("name", ["fem_unstructured", "poisson3d"])
def test_estimate_is_independent_of_the_thread_count(name):
    rp, ci, v = INPUTS[name]
    one = host_handle(rp, ci, v, host_threads=1)
    four = host_handle(rp, ci, v, host_threads=4)
    assert one.nlevels == four.nlevels
    for l in range(one.nlevels - 1):
        assert one.level_chebyshev(l) == four.level_chebyshev(l), l


def test_bounds_selected_before_the_setup_are_the_lazy_ones():
    rp, ci, v = INPUTS["poisson2d"]
    A = sa.sp_matrix_mg(rp, ci, v)
    A.set_smoother("chebyshev", 6)
    A.setup(sa.default_params(**QUIET), host_only=True)
    B = host_handle(rp, ci, v)
    for l in range(A.nlevels - 1):
        assert A.level_chebyshev(l) == B.level_chebyshev(l)


def test_bounds_need_the_host_setup():
    rp, ci, v = problems.poisson2d(16)
    A = sa.sp_matrix_mg(rp, ci, v)
    out = C.c_double()
    assert sa.lib.sparsh_level_chebyshev(A._h, 0, C.byref(out), None, None, None) == sa.SPARSH_ESTATE
    assert sa.lib.sparsh_set_chebyshev_lmax(A._h, 0, 2.0) == sa.SPARSH_ESTATE
    # the selection and its parameters need no setup
    assert sa.lib.sparsh_set_smoother(A._h, sa.SPARSH_SMOOTH_CHEBYSHEV, 0, 0) == sa.SPARSH_OK
    assert sa.lib.sparsh_set_chebyshev(A._h, 20.0, 12) == sa.SPARSH_OK


def test_chebyshev_argument_errors():
    rp, ci, v = problems.poisson2d(80)
    A = host_handle(rp, ci, v)
    h = A._h
    L = A.nlevels
    assert L >= 2
    cheb = sa.SPARSH_SMOOTH_CHEBYSHEV
    for degree in (0, 1, 4, 16):
        assert sa.lib.sparsh_set_smoother(h, cheb, degree, 0) == sa.SPARSH_OK
    assert sa.lib.sparsh_set_smoother(h, cheb, 17, 0) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_set_smoother(h, cheb, -1, 0) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_set_smoother(h, cheb, 4, 1) == sa.SPARSH_EINVAL  # no order
    for kind in (2, 4, -1):  # unknown kinds (2 has never been one and stays none)
        assert sa.lib.sparsh_set_smoother(h, kind, 0, 0) == sa.SPARSH_EINVAL
    for ratio, steps in ((1.0, 0), (0.5, 0), (-3.0, 0), (float("nan"), 0), (float("inf"), 0), (0.0, -1), (0.0, 65)):
        assert sa.lib.sparsh_set_chebyshev(h, ratio, steps) == sa.SPARSH_EINVAL, (ratio, steps)
    for ratio, steps in ((0.0, 0), (1.5, 1), (100.0, 64)):
        assert sa.lib.sparsh_set_chebyshev(h, ratio, steps) == sa.SPARSH_OK, (ratio, steps)
    out = C.c_double()
    for level in (-1, L):
        assert sa.lib.sparsh_level_chebyshev(h, level, C.byref(out), None, None, None) == sa.SPARSH_EINVAL
        assert sa.lib.sparsh_set_chebyshev_lmax(h, level, 2.0) == sa.SPARSH_EINVAL
    for lmax in (-1.0, float("nan"), float("inf")):
        assert sa.lib.sparsh_set_chebyshev_lmax(h, 0, lmax) == sa.SPARSH_EINVAL
    assert sa.lib.sparsh_level_chebyshev(h, 0, None, None, None, None) == sa.SPARSH_OK  # any pointer may be NULL
    # the operator hook and the solvers need the device setup
    n = len(rp) - 1
    b, x, hist, it = np.ones(n), np.zeros(n), np.zeros(8), C.c_int()
    assert sa.lib.sparsh_op_cheby(h, 0, sa._dp(b), sa._dp(x), 4, 0) == sa.SPARSH_ESTATE
    A.set_smoother("chebyshev", 6)
    for method in (sa.SPARSH_AMG, sa.SPARSH_PCG, sa.SPARSH_PBICG, sa.SPARSH_PGMRES):  # accepted as arguments by every solver
        assert sa.lib.sparsh_solve(h, method, sa._dp(b), sa._dp(x), sa._dp(hist), 8, C.byref(it)) == sa.SPARSH_ESTATE
    assert sa.lib.sparsh_krylov_init_dev(h, sa.SPARSH_PCG, None, None) == sa.SPARSH_ESTATE
    A.set_smoother("jacobi")


def test_chebyshev_refuses_the_fp32_preconditioner():
    rp, ci, v = problems.poisson2d(30)
    A = host_handle(rp, ci, v, precond_fp32=1)
    with pytest.raises(sa.SparshError) as e:
        A.set_smoother("chebyshev")
    assert e.value.code == sa.SPARSH_EINVAL and "fp32" in str(e.value)
    A.set_smoother("jacobi")  # Jacobi stays available


def test_non_positive_diagonal_falls_back_to_gershgorin():
    rp, ci, v = problems.poisson2d(80)
    v = v.copy()
    n = len(rp) - 1
    rows = np.repeat(np.arange(n), np.diff(rp))
    k = np.flatnonzero((ci == rows) & (rows == 17))[0]
    v[k] = -v[k]
    A = host_handle(rp, ci, v)
    c = A.level_chebyshev(0)
    assert c["lanczos"] == 0.0 and c["lmax"] == c["gershgorin"] == numpy_gershgorin(rp, ci, v)
    assert c["lmin"] == c["lmax"] / 30.0
