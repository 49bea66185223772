"""The float V-cycle's steps restated in numpy (F32Ref), anchored on the CPU: run in float64, the restatement must equal the oracle's
SpMV, residual, Jacobi sweeps, restriction and prolongation bit for bit on the levels the GPU tests use; run in float32 it is what
tests/test_gpu_fp32_ops.py holds sdia_f32_kernel, csr_f32_kernel, csr_rows_f32_kernel, prolong_agg_f32_kernel,
jacobi_zero_f32_kernel and gemv_f32_kernel to.  Also here, because they need no device: the conditions on the inputs (which slot
counts per 64-row slice, which layouts, which ragged sizes they reach) and the refusals of the float entry points."""
import functools

import numpy as np
import pytest

import oracle
import sparsh_amg_amd as sa
from sparsh_amg_amd import problems

QUIET = dict(print_setup=0, print_solve=0)
SMALL = dict(limit_upper=300, limit_lower=150)  # several levels on operators of a few thousand rows
BANDED_ROWS = 64 * 20 + 29                      # ragged last slice: 29 rows
# (pairs of bands, seed, holes): 2 K + 1 variable diagonals, K = 1 .. 12 -> 3 .. 25 slots in the interior slices and fewer in the
# slices near the two ends, which the far bands do not reach.  The seeds were picked on the CPU until the counts of
# test_inputs_reach_every_path_of_the_float_kernels were all there (8, 16 and 24 among them).
BANDED = [(1, 1, False), (3, 3, True), (4, 4, False), (6, 6, True), (9, 9, False), (12, 12, True), (7, 21, False), (10, 5, True)]


def banded(pairs, seed, holes, n=BANDED_ROWS):
    """The generator of test_sliced_diagonal_paths_fuzz (tests/test_gpu_parity.py) without its constant bands: `pairs` random offsets,
    both signs, every band and the diagonal variable, optionally with 10 % holes in every band."""
    import scipy.sparse as sp

    rng = np.random.default_rng(seed)
    offs = sorted(int(o) for o in rng.choice(np.arange(1, 400), size=pairs, replace=False))
    rows, cols, vals = [], [], []
    for o in offs:
        i = np.arange(n - o)
        keep = rng.random(len(i)) > 0.1 if holes else np.ones(len(i), bool)  # (the pattern stays symmetric: Beck's coarsening needs it)
        for lo, hi in ((i, i + o), (i + o, i)):
            v = -(0.25 + rng.random(len(i)))
            rows.append(lo[keep]); cols.append(hi[keep]); vals.append(v[keep])
    M = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n)).tocsr()
    d = np.asarray(abs(M).sum(axis=1)).ravel() + 1.0 + rng.random(n)
    A = (M + sp.diags(d)).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


GENERATORS = {
    "poisson3d": lambda: problems.poisson3d(19, 11, 23),
    "poisson2d": lambda: problems.poisson2d(45),
    "fem_unstructured": lambda: problems.fem_unstructured(5000, seed=3),
    "random_spd": lambda: problems.random_spd(3000, 9, seed=11),
}
for _k, _s, _h in BANDED:
    GENERATORS[f"banded{2 * _k + 1}{'h' if _h else ''}_s{_s}"] = functools.partial(banded, _k, _s, _h)
COARSENINGS = {"hem": 0, "beck": 1}
CASES = [(name, c) for name in GENERATORS for c in COARSENINGS]
IDS = [f"{name}-{c}" for name, c in CASES]


@functools.lru_cache(maxsize=None)
def matrix(name):
    return GENERATORS[name]()


def case_params(coarsening, **kw):
    return sa.default_params(**QUIET, **SMALL, coarsening=COARSENINGS[coarsening], **kw)


@functools.lru_cache(maxsize=None)
def host_handle(name, coarsening):
    return sa.sp_matrix_mg(*matrix(name)).setup(case_params(coarsening, precond_fp32=1), host_only=True)


# ---------------------------------------------------------------------------------------------------------------- the restatement
class Rows:
    """A CSR matrix as "the k-th stored entry of every row": sum(x) adds a row's products one by one from 0 in stored order, the
    values rounded to the dtype first, product and sum rounded separately (ChebRef.rowsum of tests/test_gpu_chebyshev.py)."""

    def __init__(self, rp, ci, v, dtype):
        self.n = len(rp) - 1
        self.dtype = dtype
        length = np.diff(rp)
        self.order = np.argsort(-length, kind="stable")
        self.count = [int((length > k).sum()) for k in range(int(length.max()) if self.n else 0)]
        self.rp, self.ci = rp.astype(np.int64), ci
        with np.errstate(over="ignore"):
            self.v = v.astype(dtype)

    def sum(self, x):
        assert x.dtype == self.dtype
        s = np.zeros(self.n, dtype=self.dtype)
        for k, c in enumerate(self.count):
            a = self.order[:c]
            j = self.rp[a] + k
            s[a] = s[a] + self.v[j] * x[self.ci[j]]
        return s


class F32Ref:
    """The steps of Engine::vcycle_f32 in numpy, every product, sum and quotient rounded once to `dtype` and taken in the kernels'
    order.  Built from level_csr (A, P, R), coarse_inverse() and params.omega alone."""

    def __init__(self, A, dtype=np.float32):
        self.dtype = np.dtype(dtype).type
        self.nlevels = A.nlevels
        self.w = self.dtype(A.params.omega)
        self.aggregation = A.params.coarsening == 0
        self.n, self.A, self.P, self.R, self.diag, self.agg = [], [], [], [], [], []
        for l in range(A.nlevels):
            rp, ci, v, _ = A.level_csr(l)
            self.n.append(len(rp) - 1)
            if l + 1 == A.nlevels:
                break
            self.A.append(Rows(rp, ci, v, self.dtype))
            rows = np.repeat(np.arange(len(rp) - 1), np.diff(rp))
            d = np.zeros(len(rp) - 1)
            d[rows[ci == rows]] = v[ci == rows]
            assert np.all(d != 0.0)
            self.diag.append(d.astype(self.dtype))
            prp, pci, pv, _ = A.level_csr(l, "P")
            self.P.append(Rows(prp, pci, pv, self.dtype))
            self.agg.append(pci if self.aggregation else None)
            if self.aggregation:
                assert np.all(np.diff(prp) == 1) and np.all(pv == 1.0)
            self.R.append(Rows(*A.level_csr(l, "R")[:3], self.dtype))
        try:
            with np.errstate(over="ignore"):
                self.inv = A.coarse_inverse().astype(self.dtype)
        except sa.SparshError:  # factored coarsest level: no dense inverse
            self.inv = None

    def spmv(self, l, x):
        return self.A[l].sum(x)

    def residual(self, l, b, x):
        return b - self.A[l].sum(x)

    def zero_sweep(self, l, b):
        return (self.w * b) / self.diag[l]

    def jacobi(self, l, b, x, sweeps, x_is_zero=False):
        k = 0
        if x_is_zero:
            x, k = (self.zero_sweep(l, b), 1) if sweeps > 0 else (np.zeros_like(b), 0)
        for _ in range(k, sweeps):
            h = b - self.A[l].sum(x)
            x = x + (self.w * h) / self.diag[l]
        return x

    def restrict(self, l, r):
        return self.R[l].sum(r)

    def prolong(self, l, xc, xf):
        if self.aggregation:
            return xc[self.agg[l]] + xf
        return self.P[l].sum(xc) + xf

    def gemv(self, b):
        """One wavefront per row: lane k adds the products of columns k, k + 64, ... from 0, then the shuffle tree folds the 64 lane
        sums (offsets 32, 16, ... 1; lane 0 holds the result)."""
        n = self.inv.shape[0]
        acc = np.zeros((n, 64), dtype=self.dtype)
        for j0 in range(0, n, 64):
            c = min(64, n - j0)
            acc[:, :c] = acc[:, :c] + self.inv[:, j0:j0 + c] * b[j0:j0 + c]
        o = 32
        while o > 0:
            acc[:, :o] = acc[:, :o] + acc[:, o:2 * o]
            o >>= 1
        return acc[:, 0].copy()

    def cycle(self, r, nu, coarse=None):
        """V(nu, nu) from a zero guess in vcycle_f32's order; r already in the dtype"""
        last = self.nlevels - 1
        bs, xs = [r], []
        for l in range(last):
            xs.append(self.jacobi(l, bs[l], None, nu, x_is_zero=True))
            bs.append(self.restrict(l, self.residual(l, bs[l], xs[l])))
        xc = (coarse or self.gemv)(bs[last])
        for l in range(last, 0, -1):
            xc = self.jacobi(l - 1, bs[l - 1], self.prolong(l - 1, xc, xs[l - 1]), nu)
        return xc


def vectors(n, dtype, seed):
    """(b, x) pairs of a level: standard normal, and the same scaled down until float denormals occur -- by 1e-30 the products
    w h / d and a_ij x_j of a residual near zero, by 1e-39 every operand"""
    rng = np.random.default_rng(seed)
    b, x = rng.standard_normal(n), rng.standard_normal(n)
    return [((b * s).astype(dtype), (x * s).astype(dtype)) for s in (1.0, 1e-30, 1e-39)]


# ---------------------------------------------------------------------------------------------------------------- layout prediction
def slots_per_slice(rp, ci):
    """distinct diagonals (column - row) among the rows of every 64-row slice: the slots of the sliced-diagonal layout"""
    n = len(rp) - 1
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    key = np.unique((rows >> 6) * (2 * n) + (ci - rows + n))
    return np.bincount(key // (2 * n), minlength=(n + 63) // 64)


def predict_layout(A, level):
    """The float operator of a level as the setup decides it (upload_sdia): the sliced-diagonal mirror for a square level of at least
    64 rows with strictly ascending columns whose slots hold at most 1.25 nnz entries, the float CSR values otherwise; none on the
    coarsest level.  Returns (layout, slots per slice or None)."""
    if level + 1 >= A.nlevels:
        return None, None
    rp, ci, _, _ = A.level_csr(level)
    n, nnz = len(rp) - 1, int(rp[-1])
    rows = np.repeat(np.arange(n), np.diff(rp))
    ascending = np.all((np.diff(ci) > 0) | (np.diff(rows) > 0))
    if n < 64 or not ascending:
        return "csr", None
    slots = slots_per_slice(rp, ci)
    if int(slots.sum()) * 64 > nnz + nnz // 4:
        return "csr", None
    return "sdia", slots


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("name,coarsening", CASES, ids=IDS)
def test_restatement_in_float64_is_the_oracle_bit_for_bit(name, coarsening):
    A = host_handle(name, coarsening)
    assert A.nlevels >= 2
    ref = F32Ref(A, np.float64)
    w = A.params.omega
    for l in range(A.nlevels - 1):
        O = oracle.Csr(*A.level_csr(l)[:3])
        prp, pci, pv, pncol = A.level_csr(l, "P")
        P = oracle.Csr(prp, pci, pv, ncol=pncol)
        n, nc = ref.n[l], ref.n[l + 1]
        xc = np.random.default_rng(100 + l).standard_normal(nc)
        for b, x in vectors(n, np.float64, 40 + l)[:2]:
            tag = (name, coarsening, l)
            assert np.array_equal(ref.spmv(l, x), oracle.spmv(O, x)), tag
            assert np.array_equal(ref.residual(l, b, x), oracle.store_residual(O, b, x)), tag
            for sweeps in (1, 2, 3):
                assert np.array_equal(ref.jacobi(l, b, x, sweeps), oracle.jacobi(O, b, x, sweeps - 1, w)), tag
                assert np.array_equal(ref.jacobi(l, b, None, sweeps, x_is_zero=True), oracle.jacobi(O, b, np.zeros(n), sweeps - 1, w)), tag
            assert np.array_equal(ref.restrict(l, x), oracle.transfer_residual(P, x)), tag
            assert np.array_equal(ref.prolong(l, xc, x), oracle.transfer_solution(P, xc, x)), tag
    # the lane sums and the tree add the same products as the plain product, in another order
    b = np.random.default_rng(9).standard_normal(ref.n[-1])
    want = A.coarse_inverse() @ b
    assert np.abs(ref.gemv(b) - want).max() <= 1e-13 * (np.abs(A.coarse_inverse()) @ np.abs(b)).max()


@pytest.mark.parametrize("name,coarsening", CASES, ids=IDS)
def test_restatement_in_float32_rounds_every_step_to_float(name, coarsening):
    """The same class in float32: every result is float32, and it is the float64 result up to float rounding and no closer (a step
    silently carried out in double would agree to 1e-16)."""
    A = host_handle(name, coarsening)
    r32, r64 = F32Ref(A, np.float32), F32Ref(A, np.float64)
    gaps = []
    for l in range(A.nlevels - 1):
        (b, x), = vectors(r32.n[l], np.float32, 60 + l)[:1]
        xc = np.random.default_rng(70 + l).standard_normal(r32.n[l + 1]).astype(np.float32)
        pairs = [(r32.residual(l, b, x), r64.residual(l, b.astype(np.float64), x.astype(np.float64))),
                 (r32.jacobi(l, b, x, 2), r64.jacobi(l, b.astype(np.float64), x.astype(np.float64), 2)),
                 (r32.restrict(l, x), r64.restrict(l, x.astype(np.float64))),
                 (r32.prolong(l, xc, x), r64.prolong(l, xc.astype(np.float64), x.astype(np.float64)))]
        for got, want in pairs:
            assert got.dtype == np.float32
            gap = np.abs(got - want).max() / np.abs(want).max()
            assert gap <= 1e-5
            gaps.append(gap)
    assert max(gaps) > 1e-9
    b = np.random.default_rng(8).standard_normal(r32.n[-1]).astype(np.float32)
    got, want = r32.gemv(b), r64.gemv(b.astype(np.float64))
    assert got.dtype == np.float32 and np.abs(got - want).max() <= 1e-5 * (np.abs(r64.inv) @ np.abs(b)).max()


def test_inputs_reach_every_path_of_the_float_kernels():
    """sdia_f32_kernel walks a slice's slots in chunks of 8 and a switch over the 1 .. 7 left; lanes past the last row are clamped;
    gemv_f32_kernel's lanes run out of columns below 64 and in a ragged last pass.  The inputs must reach all of it."""
    counts, layouts, ragged_levels, coarsest = set(), set(), [], set()
    beck_long_rows = beck_other_values = False
    for name, coarsening in CASES:
        A = host_handle(name, coarsening)
        coarsest.add(A.level_info(A.nlevels - 1)["nrow"])
        assert predict_layout(A, A.nlevels - 1) == (None, None)
        for l in range(A.nlevels - 1):
            layout, slots = predict_layout(A, l)
            layouts.add(layout)
            if layout == "sdia":
                counts |= set(int(c) for c in slots)
                if A.level_info(l)["nrow"] % 64:
                    ragged_levels.append((name, coarsening, l))
            if coarsening == "beck":
                prp, _, pv, _ = A.level_csr(l, "P")
                beck_long_rows |= bool(np.diff(prp).max() > 1)
                beck_other_values |= bool(np.any(pv != 1.0))
    print("slots per slice:", sorted(counts), "coarsest sizes:", sorted(coarsest))
    assert {c % 8 for c in counts} == set(range(8)), sorted(counts)
    assert {8, 16, 24} & counts, sorted(counts)          # a slice made of whole chunks only
    assert max(counts) >= 16, sorted(counts)             # more than one chunk
    assert any(9 <= c <= 15 for c in counts), sorted(counts)  # a chunk and a tail: the dropped ninth diagonal
    assert ragged_levels
    assert layouts == {"sdia", "csr"}
    assert any(n < 64 for n in coarsest) and any(n >= 64 and n % 64 for n in coarsest), sorted(coarsest)
    assert beck_long_rows and beck_other_values  # a general P: csr_rows_f32_kernel with add = 1, 4-6 entries per row of R


def test_restriction_order_is_readable_from_the_handle():
    """level_csr(l, "R") is P^T with every coarse row's entries in ascending fine-row order"""
    import scipy.sparse as sp

    for coarsening in COARSENINGS:
        A = host_handle("poisson2d", coarsening)
        for l in range(A.nlevels - 1):
            rp, ci, v, ncol = A.level_csr(l, "R")
            PT = sp.csr_matrix(A.level_scipy(l, "P").T)
            PT.sort_indices()
            assert ncol == A.level_info(l)["nrow"] and len(rp) - 1 == A.level_info(l)["p_ncol"]
            assert np.array_equal(rp, PT.indptr) and np.array_equal(ci, PT.indices) and np.array_equal(v, PT.data)
    with pytest.raises(sa.SparshError) as e:
        A.level_csr(A.nlevels - 1, "R")
    assert e.value.code == sa.SPARSH_EINVAL


def float_calls(A, level=0):
    """every float entry point with arguments of the right sizes for `level` (host vectors are not touched before the checks)"""
    info = A.level_info(min(max(level, 0), A.nlevels - 1))
    n = info["nrow"]
    f = np.zeros(max(n, info["p_ncol"], 1), dtype=np.float32)
    leveled = {
        "level_f32_layout": lambda: A.level_f32_layout(level),
        "op_jacobi_f32": lambda: A.op_jacobi_f32(level, f[:n], f[:n], 1),
        "op_residual_f32": lambda: A.op_residual_f32(level, f[:n], f[:n]),
        "op_restrict_f32": lambda: sa._check(sa.lib.sparsh_op_restrict_f32(A._h, level, sa._fp(f), sa._fp(f.copy()))),
        "op_prolong_f32": lambda: A.op_prolong_f32(level, f[:max(info["p_ncol"], 1)], f[:n]),
    }
    plain = {
        "op_coarse_f32": lambda: A.op_coarse_f32(f[:A.level_info(A.nlevels - 1)["nrow"]]),
        "op_cvt_f32": lambda: A.op_cvt_f32(np.zeros(5)),
        "op_cvt_f2d_dot": lambda: A.op_cvt_f2d_dot(f[:1], np.zeros(1)),
    }
    return leveled, plain


def refused(call):
    with pytest.raises(sa.SparshError) as e:
        call()
    return e.value.code, str(e.value)


def test_float_entry_points_refuse_what_they_cannot_serve():
    rp, ci, v = matrix("poisson2d")
    # no precond_fp32, and a single level: no float hierarchy, said with op_precond_f32's message
    plain = sa.sp_matrix_mg(rp, ci, v).setup(case_params("hem"), host_only=True)
    single = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET, precond_fp32=1), host_only=True)
    assert plain.nlevels > 1 and single.nlevels == 1
    for A in (plain, single):
        leveled, rest = float_calls(A)
        for name, call in {**leveled, **rest}.items():
            code, msg = refused(call)
            assert code == sa.SPARSH_ESTATE and "fp32 preconditioner hierarchy was not built" in msg, (name, msg)
    # a float hierarchy: a bad level is a bad argument; a good call stops at the missing device setup
    A = host_handle("poisson2d", "hem")
    for level in (-1, A.nlevels, A.nlevels + 7):
        for name, call in float_calls(A, level)[0].items():
            code, msg = refused(call)
            assert code == sa.SPARSH_EINVAL and "level out of range" in msg, (name, level, msg)
    for name, call in float_calls(A, A.nlevels - 1)[0].items():
        if name == "level_f32_layout":  # (answers None there once the device is set up)
            continue
        code, msg = refused(call)
        assert code == sa.SPARSH_EINVAL and "coarsest level has no float operator" in msg, (name, msg)
    for n in (0, -3):
        assert sa.lib.sparsh_op_cvt_f32(A._h, n, None, None) == sa.SPARSH_EINVAL
        assert sa.lib.sparsh_op_cvt_f2d_dot(A._h, n, None, None, None, None) == sa.SPARSH_EINVAL
    leveled, rest = float_calls(A)
    for name, call in {**leveled, **rest}.items():
        code, msg = refused(call)
        assert code == sa.SPARSH_ESTATE and "sparsh_setup has not been called" in msg, (name, msg)
    assert sa.lib.sparsh_op_coarse_f32(None, None, None) == sa.SPARSH_EINVAL
    # float64 arrays are refused by the binding, not rounded on the way in
    with pytest.raises(TypeError):
        A.op_residual_f32(0, np.zeros(4), np.zeros(4))
