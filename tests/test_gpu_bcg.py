"""Block CG on the device: the small-solve kernel against sparsh_debug_bcg_small bit for bit, the update and
direction kernels against numpy in the stated order bit for bit, whole solves by their true residuals, the loop against its numpy
restatement driven by the handle's own SpMV and block V-cycle, degenerate blocks, the iteration gain over block PCG that is the point
of the method, and the isolation of block PCG.  GPU box only."""
import functools
import math

import numpy as np
import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from bcg_restatement import bcg, degenerate_block, direction, small_cases, update

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
LIMITS = dict(limit_upper=300, limit_lower=100)  # several levels on operators of a few hundred to a few thousand rows
INPUTS = {
    "p3_10_9_8": lambda: problems.poisson3d(10, 9, 8),
    "fem_3000": lambda: problems.fem_unstructured(3000),
}
SIZES = (1, 63, 64, 65, 1000, 4097)  # below, at and above a wave and a pass of a workgroup; several workgroups
KS = (1, 2, 3, 4, 5, 8)              # every width (2, 4, 8), with and without padding columns


@functools.lru_cache(maxsize=None)
def handle(name):
    return sa.sp_matrix_mg(*INPUTS[name]()).setup(sa.default_params(**QUIET, **LIMITS))


@functools.lru_cache(maxsize=None)
def rhs(name, k=8):
    return np.random.default_rng(41).standard_normal((handle(name).nrow, 8))[:, :k]


def solve(A, method, B, X0=None):
    X = np.zeros_like(B) if X0 is None else np.array(X0)
    hists, iters, status, rc = A.solve_multi(method, B, X)
    return X, hists, iters, status, rc


def true_residuals(A, B, X):
    return np.linalg.norm(B - A.level_scipy(0) @ X, axis=0)


# ---------------------------------------------------------------------------- kernels

@pytest.mark.parametrize("W", [2, 4, 8])
def test_small_kernel_is_the_host_function_bit_for_bit(W):
    """every k <= W on the leading blocks of every input: well-conditioned, duplicate, zero, rank 1, at the pivot rule, no direction"""
    A = handle("p3_10_9_8")
    ran = 0
    for name, G, Cm, _ in small_cases():
        for k in range(1, min(len(G), W) + 1):
            Gk, Ck = np.ascontiguousarray(G[:k, :k]), np.ascontiguousarray(Cm[:k, :k])
            for sign in (1.0, -1.0):
                want, wkeep, wrank = sa.bcg_small(Gk, Ck, sign)
                got, keep, rank = A.op_bcg_small(W, Gk, Ck, sign)
                assert rank == wrank and np.array_equal(keep, wkeep), (name, W, k)
                assert np.array_equal(got, want), (name, W, k, sign)
                ran += 1
    assert ran >= 2 * W * 8


def blocks(n, k, seed):
    rng = np.random.default_rng(seed)
    X, R, P, Q = (rng.standard_normal((n, k)) for _ in range(4))
    coef = rng.standard_normal((k, k))
    return X, R, P, Q, coef


@pytest.mark.parametrize("n", SIZES)
def test_update_kernel_is_numpy_in_the_stated_order(n):
    A = handle("p3_10_9_8")
    for k in KS:
        X, R, P, Q, alpha = blocks(n, k, 1000 * n + k)
        for dropped in ((), (0,), (k - 1,), tuple(range(0, k, 2))):
            al = np.array(alpha)
            al[list(dropped), :] = 0.0  # the rows of dropped directions
            wx, wr = update(X, R, P, Q, al)
            for in_place in (False, True):
                gx, gr, norms = A.op_bcg_update(X, R, P, Q, al, in_place=in_place)  # (a padding column that is not zero raises)
                assert np.array_equal(gx, wx) and np.array_equal(gr, wr), (n, k, dropped, in_place)
            # the norms: the bound of the block-dot tests, 1e-13 of the sum of the absolute terms
            for c in range(k):
                exact = math.fsum(float(v) * float(v) for v in wr[:, c])
                assert abs(norms[c] * norms[c] - exact) <= 1e-13 * exact, (n, k, c, norms[c], math.sqrt(exact))


@pytest.mark.parametrize("n", SIZES)
def test_direction_kernel_is_numpy_in_the_stated_order(n):
    A = handle("p3_10_9_8")
    for k in KS:
        Z, _, P, _, beta = blocks(n, k, 2000 * n + k)
        for dropped in ((), (0,), (k - 1,), tuple(range(0, k, 2))):
            be = np.array(beta)
            be[list(dropped), :] = 0.0
            want = direction(Z, P, be)
            for in_place in (False, True):
                assert np.array_equal(A.op_bcg_dir(Z, P, be, in_place=in_place), want), (n, k, dropped, in_place)


def test_hooks_refuse_bad_arguments():
    A = handle("p3_10_9_8")
    with pytest.raises(sa.SparshError) as e:
        A.op_bcg_small(3, np.eye(2), np.eye(2))
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:
        A.op_bcg_small(2, np.eye(3), np.eye(3))
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:
        A.op_bcg_dir(np.ones((5, 9)), np.ones((5, 9)), np.eye(9))
    assert e.value.code == sa.SPARSH_EINVAL


# ---------------------------------------------------------------------------- whole solves

@pytest.mark.parametrize("name", list(INPUTS))
@pytest.mark.parametrize("nrhs", [1, 3, 8])
def test_solves_reach_the_tolerance_in_the_true_residual(name, nrhs):
    A = handle(name)
    B = rhs(name, nrhs)
    X, hists, iters, status, rc = solve(A, "bcg", B)
    tol = A.params.tol
    assert rc == 0 and np.all(status == 0)
    assert len(set(iters)) == 1 and all(len(h) == iters[0] for h in hists)
    assert all(h[-1] <= tol for h in hists) and any(h[-2] > tol for h in hists)
    res = true_residuals(A, B, X)
    info = A.bcg_info()
    print(name, nrhs, "iterations", iters[0], "largest true residual", res.max(), info)
    assert np.all(res <= 10 * tol)
    assert info["iterations"] == iters[0] and info["min_rank"] == nrhs and info["dropped"] == 0 and info["bytes"] > 0
    if nrhs == 1:
        x = np.zeros(A.nrow)
        h, rc1 = A.solve("pcg", B[:, 0], x)
        print(name, "single PCG iterations", len(h))
        assert rc1 == 0 and abs(len(h) - iters[0]) <= 1


def restated(A, B, chunk):
    spmv = lambda V: np.column_stack([A.op_spmv(0, V[:, c]) for c in range(V.shape[1])])  # noqa: E731
    return bcg(spmv, A.op_precond_multi, B, np.zeros_like(B), A.params.tol, 500, chunk)


def spread(h0, h1):
    m = min(len(h0), len(h1))
    return float((np.abs(h0[:m] - h1[:m]) / h0[:m]).max())


@pytest.mark.parametrize("name,nrhs", [("p3_10_9_8", 3), ("fem_3000", 8)])
def test_the_loop_follows_its_restatement(name, nrhs):
    """The restatement runs twice on the CPU with the handle's own SpMV and block V-cycle, its Gram sums ascending and in chunks of
    256 rows: the largest relative spread of the two residual histories is the noise floor of the summation order, and the device,
    whose Gram launch adds in yet another order, may differ from the first by ten times that.  Measured on an MI355X: floor 1.6e-11
    and device 1.2e-11 on p3_10_9_8 with 3 columns (6 iterations all three), floor 1.1e-4 and device 1.2e-4 on fem_3000 with 8
    (18 iterations all three; the last entries before tol are the sensitive ones)."""
    A = handle(name)
    B = rhs(name, nrhs)
    (_, h0, i0), (_, h1, i1) = restated(A, B, 0), restated(A, B, 256)
    floor = spread(h0, h1)
    X, hists, iters, status, rc = solve(A, "bcg", B)
    hd = np.column_stack(hists)
    dev = spread(h0, hd)
    print(name, nrhs, "iterations: restatement", i0["iterations"], i1["iterations"], "device", iters[0], "noise floor", floor, "device", dev)
    assert rc == 0 and i0["status"] == "ok"
    assert abs(iters[0] - i0["iterations"]) <= 1
    assert A.bcg_info()["min_rank"] == i0["min_rank"] == nrhs
    assert dev <= 10 * floor


def test_a_degenerate_block_loses_rank_not_the_solve():
    A = handle("fem_3000")
    B = degenerate_block(rhs("fem_3000"))
    _, h0, i0 = restated(A, B, 0)
    assert i0["status"] == "ok" and i0["min_rank"] == 5
    X, hists, iters, status, rc = solve(A, "bcg", B)
    info = A.bcg_info()
    print("degenerate block: iterations", iters[0], "restatement", i0["iterations"], info, "against", solve(A, "bcg", rhs("fem_3000"))[2][0], "at full rank")
    assert rc == 0 and np.all(status == 0) and not np.isnan(X).any()
    assert info["min_rank"] == i0["min_rank"]
    assert np.all(true_residuals(A, B, X) <= 10 * A.params.tol)
    assert np.array_equal(X[:, 3], np.zeros(A.nrow))  # the zero right-hand side is a dropped direction
    # a column scaled by 1e-6 and a smooth column converge with the rest at full rank
    Bs = np.array(rhs("fem_3000"))
    Bs[:, 2] *= 1e-6
    Bs[:, 4] = A.level_scipy(0) @ np.ones(A.nrow)
    X, hists, iters, status, rc = solve(A, "bcg", Bs)
    assert rc == 0 and A.bcg_info()["min_rank"] == 8 and np.all(true_residuals(A, Bs, X) <= 10 * A.params.tol)


def test_block_cg_needs_at_most_0_6_of_block_pcgs_iterations():
    """the point of the feature: the CPU model gives 18 against 44 - 45 on this problem, a ratio of 0.41"""
    A = handle("fem_3000")
    B = rhs("fem_3000")
    _, _, it_pcg, _, rc0 = solve(A, "pcg", B)
    _, _, it_bcg, _, rc1 = solve(A, "bcg", B)
    print("fem_3000, 8 columns: block PCG", list(it_pcg), "block CG", it_bcg[0], "ratio", it_bcg[0] / it_pcg.max())
    assert rc0 == 0 and rc1 == 0
    assert it_bcg[0] <= 0.6 * it_pcg.max()


# ---------------------------------------------------------------------------- stopping, results, isolation

def test_cap_zero_block_nan_and_check_every():
    rp, ci, v = INPUTS["fem_3000"]()
    B = rhs("fem_3000", 5)
    out = []
    for every in (1, 7):
        A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, **LIMITS, check_every=every))
        out.append(solve(A, "bcg", B))
        if every == 1:
            tol = A.params.tol
            n_it = int(out[0][2][0])
            A.set_stopping(tol, max_iter=4)
            Xc, hc, ic, sc, rcc = solve(A, "bcg", B)
            A.set_stopping(tol, max_iter=sa.default_params().max_iter)
            assert rcc == sa.SPARSH_ENOCONV and np.all(sc == sa.SPARSH_ENOCONV) and np.all(ic == 4) and n_it > 4
            assert all(np.array_equal(hc[c], out[0][1][c][:4]) for c in range(5)) and A.bcg_info()["iterations"] == 4
            # nothing to do: zero right-hand sides, and a block that starts at its solution
            Xz, hz, iz, sz, rcz = solve(A, "bcg", np.zeros((A.nrow, 3)))
            assert rcz == 0 and np.all(iz == 0) and np.array_equal(Xz, np.zeros((A.nrow, 3))) and all(len(h) == 0 for h in hz)
            Xs, hs, is_, ss, rcs = solve(A, "bcg", B, out[0][0])
            assert rcs == 0 and np.all(is_ <= 1)
            # a NaN is a numeric failure of every column
            Bn = np.array(B)
            Bn[11, 2] = np.nan
            _, _, _, sn, rcn = solve(A, "bcg", Bn)
            assert rcn == sa.SPARSH_ENUMERIC and np.all(sn == sa.SPARSH_ENUMERIC)
            # ... and the next solve is clean
            again = solve(A, "bcg", B)
            assert again[4] == 0 and np.array_equal(again[0], out[0][0])
        A.close()
    (X1, h1, i1, s1, _), (X7, h7, i7, s7, _) = out
    # the kernels of the iterations queued past convergence leave at once: the same bits whatever check_every
    assert np.array_equal(X1, X7) and np.array_equal(i1, i7) and np.array_equal(s1, s7)
    assert all(np.array_equal(a, b) for a, b in zip(h1, h7))


def test_block_pcg_keeps_its_bits_and_bytes_around_a_block_cg_solve():
    A = sa.sp_matrix_mg(*INPUTS["p3_10_9_8"]()).setup(sa.default_params(**QUIET, **LIMITS))
    B = rhs("p3_10_9_8", 4)
    zeros = dict(iterations=0, min_rank=0, dropped=0, bytes=0)
    before = solve(A, "pcg", B)
    width_bytes = A.multi_info()
    assert A.bcg_info() == zeros
    first = solve(A, "bcg", B)
    assert first[4] == 0 and A.multi_info() == width_bytes
    info = A.bcg_info()
    W = 4
    assert info["bytes"] >= (5 * W * W + 2 * W * W * 512) * 8 and info["iterations"] == first[2][0]
    after = solve(A, "pcg", B)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[2], after[2])
    assert all(np.array_equal(a, b) for a, b in zip(before[1], after[1]))
    second = solve(A, "bcg", B)
    assert np.array_equal(first[0], second[0]) and all(np.array_equal(a, b) for a, b in zip(first[1], second[1]))
    # another width replaces the block vectors and the solver's arrays with them; a new setup drops both
    solve(A, "bcg", B[:, :2])
    assert A.multi_info()["width"] == 2 and 0 < A.bcg_info()["bytes"] < info["bytes"]
    A.setup(sa.default_params(**QUIET, **LIMITS))
    assert A.multi_info() == dict(width=0, bytes=0) and A.bcg_info()["bytes"] == 0
    # the refusals of the block path hold
    X = np.zeros_like(B)
    for kind, order in (("sor", "symmetric"), ("chebyshev", "forward")):
        A.set_smoother(kind, 0, order)
        with pytest.raises(sa.SparshError) as e:
            A.solve_multi("bcg", B, X)
        assert e.value.code == sa.SPARSH_EINVAL, kind
    A.set_smoother("jacobi")
    A.set_cycle("w")
    with pytest.raises(sa.SparshError) as e:
        A.solve_multi("bcg", B, X)
    assert e.value.code == sa.SPARSH_EINVAL
    A.set_cycle("v")
    assert solve(A, "bcg", B)[4] == 0
    with pytest.raises(sa.SparshError) as e:
        A.solve_multi("bcg", np.ones((A.nrow, 9)), np.zeros((A.nrow, 9)))
    assert e.value.code == sa.SPARSH_EINVAL
    A.close()
