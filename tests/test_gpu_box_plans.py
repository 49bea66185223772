"""The box-grid kernels (sdia_box2_kernel, sdia_box1_kernel) under the launch plans the benchmark runs and under forced ones.

The planners give every box grid of the other parity tests one plane per chunk (CZ = 1), so a workgroup there takes three steps of
the plane loop.  Here sparsh_set_box_plan forces (points per thread Q, lines per tile TY, planes per chunk CZ) -- several planes per
chunk, a short last chunk, TY from one line to the largest region the workgroup holds -- and every stored vector is compared with the
CPU oracle on the device's own level operators (level_csr) bit for bit, every fused dot with a long-double sum to 1e-12 of the sum of
the terms' magnitudes.  Then whole solves under forced plans, the 216^3 hierarchy of the benchmark under its own plans, and the
argument checks of the override.  GPU box only.
"""
import numpy as np
import pytest

import oracle
import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import hist_tolerance

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
BLOCK = 1024  # threads per workgroup of both kernels (kBoxBlock)


def _stencil7(nx, ny, nz, c):
    """7-point operator on an nx x ny x nz box with a distinct constant per offset: c = (down, south, west, centre, east, north, up)."""
    import scipy.sparse as sp

    def shift(n, k):
        return sp.diags([np.ones(n - 1)], [k], shape=(n, n))

    Ix, Iy, Iz = sp.identity(nx), sp.identity(ny), sp.identity(nz)
    A = (c[3] * sp.kron(Iz, sp.kron(Iy, Ix)) + c[2] * sp.kron(Iz, sp.kron(Iy, shift(nx, -1))) + c[4] * sp.kron(Iz, sp.kron(Iy, shift(nx, 1)))
         + c[1] * sp.kron(Iz, sp.kron(shift(ny, -1), Ix)) + c[5] * sp.kron(Iz, sp.kron(shift(ny, 1), Ix))
         + c[0] * sp.kron(shift(nz, -1), sp.kron(Iy, Ix)) + c[6] * sp.kron(shift(nz, 1), sp.kron(Iy, Ix))).tocsr()
    A.sort_indices()
    return A.indptr.astype(np.int32), A.indices.astype(np.int32), A.data.astype(np.float64)


def _lds_bytes(kernel, nx, ty):
    """Dynamic LDS of a launch: two region planes (x0, x1) for the double sweep, one for the marching kernel (pad cell per line + 1)."""
    return (2 if kernel == 2 else 1) * ((ty + (4 if kernel == 2 else 2)) * (nx + 1) + 1) * 8


def _max_ty(kernel, q, nx, ny):
    """Largest lines per tile the kernel runs with q points per thread (0: none): region rows <= q * 1024 threads, LDS <= 64 KiB."""
    ty = min(ny, q * BLOCK // nx - (4 if kernel == 2 else 2))
    while ty >= 1 and _lds_bytes(kernel, nx, ty) > 65536:
        ty -= 1
    return max(ty, 0)


def _planner(kernel, nx, ny, nz, shared_cu=False):
    """box_planner restated: the plan with the lowest modelled cost (first one on ties)."""
    best, plan = None, None
    for q in (2, 3, 4):
        ty = _max_ty(kernel, q, nx, ny)
        if ty < 1:
            continue
        ytiles = -(-ny // ty)
        for zch in range(1, nz + 1):
            cz = -(-nz // zch)
            w = ytiles * -(-nz // cz)
            steps = cz + (2 if kernel == 2 else 1)
            two_per_cu = (q == 2) if kernel == 2 else (shared_cu and q <= 3)
            cost = ((w + 511) // 512) * steps * q * 16 if two_per_cu and w > 256 else ((w + 255) // 256) * steps * q * 10
            if best is None or cost < best:
                best, plan = cost, (q, ty, cz)
    return plan


def _workgroups(ny, nz, ty, cz):
    return -(-ny // ty) * -(-nz // cz)


def _plan_of(A, l, kernel):
    d = A.level_double_sweep(l) if kernel == 2 else A.level_marching_ops(l)
    return d["on"], (d["points_per_thread"], d["lines_per_tile"], d["planes_per_chunk"])


def _csr(A, l, which="A"):
    rp, ci, v, ncol = A.level_csr(l, which)
    return oracle.Csr(rp, ci, v, ncol=ncol)


def _dot_ok(got, x, y):
    """A fused dot against the long-double sum of its terms, to 1e-12 of the sum of their magnitudes (as test_blas1)."""
    t = np.asarray(x, dtype=np.longdouble) * np.asarray(y, dtype=np.longdouble)
    return abs(np.longdouble(got) - t.sum()) <= 1e-12 * np.abs(t).sum()


class _LevelRef:
    """What the oracle says level l's operators give on fixed inputs; independent of the launch plan, so computed once."""

    def __init__(self, A, l, grid, rng):
        self.l, self.grid = l, grid
        self.n = A.level_info(l)["nrow"]
        Ol = _csr(A, l)
        n = self.n
        self.x, self.b = rng.standard_normal(n), rng.standard_normal(n)
        self.bz = self.b.copy()
        self.bz[::7] = 0.0  # zeros in the right-hand side take the plain-division branch of div_const
        zero = np.zeros(n)
        self.jac = {s: oracle.jacobi(Ol, self.b, self.x, s - 1) for s in (1, 2, 3, 4, 7)}
        self.jz = {s: oracle.jacobi(Ol, self.b, zero, s - 1) for s in (3, 4, 5, 7)}
        self.jzz = oracle.jacobi(Ol, self.bz, zero, 2)
        self.ax = oracle.spmv(Ol, self.x)
        self.paired = A.level_paired(l) == 1 and grid[0] % 2 == 0  # row pairs on an even line: the marching kernel's RESID_PAIRX epilogue
        if self.paired:
            r = oracle.store_residual(Ol, self.b, self.x)
            bc = oracle.transfer_residual(_csr(A, l, "P"), r)
            self.restrict = (bc, oracle.jacobi(_csr(A, l + 1), bc, np.zeros(len(bc)), 0))
        self.prolong = bool(A.level_prolong_fused(l))
        if self.prolong:
            self.xf = rng.standard_normal(A.level_info(l - 1)["nrow"])
            self.prolonged = oracle.transfer_solution(_csr(A, l - 1, "P"), self.jac[1], self.xf)


def _check_double(A, ref, tag, zero_sweeps=(3, 4, 5, 7)):
    """op_jacobi with 2, 4, 7 sweeps and from a zero guess (3 = the ZERO launch alone, 4, 5, 7 with what follows it)."""
    l = ref.l
    for s in (2, 4, 7):
        assert np.array_equal(A.op_jacobi(l, ref.b, ref.x, s), ref.jac[s]), (tag, "jacobi", s)
    for s in zero_sweeps:
        assert np.array_equal(A.op_jacobi(l, ref.b, np.zeros(ref.n), s, x_is_zero=True), ref.jz[s]), (tag, "jacobi from zero", s)
    assert np.array_equal(A.op_jacobi(l, ref.bz, np.zeros(ref.n), 3, x_is_zero=True), ref.jzz), (tag, "jacobi from zero, zeros in b")


def _check_marching(A, ref, tag):
    """The marching kernel's epilogues: plain sweep (1 and 3 sweeps), SpMV + dot, sweep + dot, pair restriction, prolongation."""
    l = ref.l
    for s in (1, 3):
        assert np.array_equal(A.op_jacobi(l, ref.b, ref.x, s), ref.jac[s]), (tag, "jacobi", s)
    y, d = A.op_spmv_dot(l, ref.x)
    assert np.array_equal(y, ref.ax) and _dot_ok(d, ref.x, ref.ax), (tag, "spmv_dot")
    y, d = A.op_jacobi_dot(l, ref.b, ref.x)
    assert np.array_equal(y, ref.jac[1]) and _dot_ok(d, ref.jac[1], ref.b), (tag, "jacobi_dot")
    if ref.paired:
        bc, xc = A.op_residual_restrict(l, ref.b, ref.x)
        assert np.array_equal(bc, ref.restrict[0]) and np.array_equal(xc, ref.restrict[1]), (tag, "residual_restrict")
    if ref.prolong:
        assert np.array_equal(A.op_jacobi_prolong(l, ref.b, ref.x, ref.xf), ref.prolonged), (tag, "jacobi_prolong")


def _plans(kernel, grid, full):
    """(Q, TY, CZ) to force: every Q the grid admits; TY = 1, two thirds of the largest, the largest the region allows; CZ = 1, 2, 3, 7,
    nz - 1 (last chunk of one plane), nz.  Coarser levels (full = False): TY = 1 and the largest, CZ = 2, nz - 1, nz."""
    nx, ny, nz = grid
    out = []
    for q in (2, 3, 4):
        top = _max_ty(kernel, q, nx, ny)
        if top < 1:
            continue
        tys = sorted({1, max(1, 2 * top // 3), top} if full else {1, top})  # (2/3 of the largest: a ragged last tile where ny allows)
        czs = sorted({c for c in ((1, 2, 3, 7, nz - 1, nz) if full else (2, nz - 1, nz)) if 1 <= c <= nz})
        out += [(q, ty, cz) for ty in tys for cz in czs]
    return out


GRIDS = {
    "even_nx_odd_nz_40x36x45": lambda: problems.poisson3d(40, 36, 45),
    "odd_nx_27x50x33": lambda: problems.poisson3d(27, 50, 33),
    "line216_216x30x29": lambda: problems.poisson3d(216, 30, 29),  # TY 12 / 14 with Q 3 / 4 as at 216^3
    "stencil7_36x28x31": lambda: _stencil7(36, 28, 31, (-2.5, -2.0, -1.5, 10.0, -0.5, -1.0, -0.7)),
}


@pytest.mark.parametrize("name", list(GRIDS))
def test_forced_plans_bitwise(name):
    """Every box level of the hierarchy under a sweep of forced plans of each kernel in turn (the other one on its planner's plan):
    the level-0 sweep is the full set of _plans, coarser box levels a smaller one.  (No plan here launches more than ny * nz <= 4096
    marching workgroups: all of them fit the reduction buffers.)"""
    rp, ci, v = GRIDS[name]()
    A = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET))
    nz0 = A.level_double_sweep(0)["grid"][2]
    rng = np.random.default_rng(91)
    boxes = [l for l in range(A.nlevels - 1) if A.level_double_sweep(l)["on"]]
    assert boxes and boxes[0] == 0, [A.level_double_sweep(l) for l in range(A.nlevels)]
    ran = {1: [], 2: []}
    for l in boxes:
        grid = tuple(A.level_double_sweep(l)["grid"])
        ref = _LevelRef(A, l, grid, rng)
        assert A.level_marching_ops(l)["on"], (name, l)
        for kernel in (2, 1):
            planned = _plan_of(A, l, kernel)[1]
            for plan in _plans(kernel, grid, full=l == 0):
                A.set_box_plan(l, kernel, *plan)
                assert _plan_of(A, l, kernel) == (True, plan), (name, l, kernel, plan)
                tag = (name, l, grid, kernel, plan)
                if kernel == 2:
                    _check_double(A, ref, tag)
                else:
                    _check_marching(A, ref, tag)
                ran[kernel].append((l, plan))
            A.set_box_plan(l, kernel)  # back to the planner's plan
            assert _plan_of(A, l, kernel)[1] == planned
    for kernel in (2, 1):
        level0 = [p for l, p in ran[kernel] if l == 0]
        assert any(p[2] > 1 and nz0 % p[2] != 0 for p in level0), (name, kernel)  # chunks of several planes and a shorter last one ran
        assert {p[0] for p in level0} == {2, 3, 4}, (name, kernel, level0)
        print(f"{name} kernel {kernel}: {len(level0)} plans on level 0, {len(ran[kernel]) - len(level0)} on coarser levels; "
              f"level 0 ran {sorted(level0)}")
    A.close()


def _force_plans(A, boxes, double_cz, marching_cz):
    """Every box level on plans of several planes per chunk: double sweep Q2 / half the largest TY, marching kernel Q3 / largest TY."""
    for l in boxes:
        nx, ny, nz = A.level_double_sweep(l)["grid"]
        A.set_box_plan(l, 2, 2, max(1, _max_ty(2, 2, nx, ny) // 2), min(double_cz, nz))
        A.set_box_plan(l, 1, 3, _max_ty(1, 3, nx, ny), min(marching_cz, nz))


def test_solves_under_forced_plans():
    """AMG and PCG with both kernels on forced plans of several planes per chunk (short last chunks): AMG history and x bitwise those of
    the same handle with the box kernels off, PCG within hist_tolerance of the oracle; the captured PCG iteration gives the eager
    run's bits, also after the plans change (the graph is dropped and captured again)."""
    rp, ci, v = problems.poisson3d(40, 36, 45)
    n = len(rp) - 1
    b = np.random.default_rng(93).standard_normal(n)
    A = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET))
    G = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET, use_graph=1))
    boxes = [l for l in range(A.nlevels - 1) if A.level_double_sweep(l)["on"]]
    assert len(boxes) >= 2
    _force_plans(A, boxes, 4, 7)
    assert all(A.level_double_sweep(l)["planes_per_chunk"] > 1 and A.level_marching_ops(l)["planes_per_chunk"] > 1 for l in boxes)

    def run(H, method):
        x = np.zeros(n)
        h, rc = H.solve(method, b, x)
        assert rc == 0 and len(h) > 1
        return np.array(h), x

    h_amg, x_amg = run(A, "amg")
    h_pcg, x_pcg = run(A, "pcg")
    A.set_double_sweep(0).set_marching_ops(0)
    assert not A.level_double_sweep(0)["on"] and not A.level_marching_ops(0)["on"]
    h0, x0 = run(A, "amg")
    assert np.array_equal(h_amg, h0) and np.array_equal(x_amg, x0)
    A.set_double_sweep(2).set_marching_ops(2)
    O = oracle.Csr(rp, ci, v)
    xo, ho = oracle.solve("pcg", O, b)
    assert len(h_pcg) == len(ho), (len(h_pcg), len(ho))
    assert np.all(np.abs(h_pcg - ho) / ho <= hist_tolerance(ho))
    assert np.linalg.norm(x_pcg - xo) <= 1e-8 * np.linalg.norm(xo)
    _force_plans(G, boxes, 4, 7)
    for _ in range(2):
        hg, xg = run(G, "pcg")
        assert np.array_equal(hg, h_pcg) and np.array_equal(xg, x_pcg)
    for H in (A, G):  # other plans: the captured graph of the old ones must not be replayed
        _force_plans(H, boxes, 3, 2)
    h2, x2 = run(A, "pcg")
    hg, xg = run(G, "pcg")
    assert np.array_equal(hg, h2) and np.array_equal(xg, x2)
    assert np.all(np.abs(h2 - ho) / ho <= hist_tolerance(ho))
    A.close()
    G.close()


def test_benchmark_levels_216():
    """The 216^3 hierarchy of the benchmark, set up with defaults: the plans in force on every level that runs a box kernel (printed),
    level 0's double sweep on Q4 / TY14 / CZ14, and the box kernels' operators against the oracle on each of those levels -- then once
    more with the marching kernel on its shared-CU plan on levels 0 - 2."""
    rp, ci, v = problems.poisson3d(216)
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET))
    del rp, ci, v
    rng = np.random.default_rng(95)
    on = []
    for l in range(A.nlevels - 1):
        d2, d1 = A.level_double_sweep(l), A.level_marching_ops(l)
        if d2["on"] or d1["on"]:
            on.append(l)
            print(f"216^3 level {l} grid {d2['grid']}: double sweep {'on' if d2['on'] else 'off'} plan {_plan_of(A, l, 2)[1]}, "
                  f"marching kernel {'on' if d1['on'] else 'off'} plan {_plan_of(A, l, 1)[1]}")
    assert 0 in on and _plan_of(A, 0, 2) == (True, (4, 14, 14))
    for l in on:
        grid = tuple(A.level_double_sweep(l)["grid"])
        ref = _LevelRef(A, l, grid, rng)
        tag = ("216^3", l, grid)
        if A.level_double_sweep(l)["on"]:
            _check_double(A, ref, tag, zero_sweeps=(3, 4))
        _check_marching(A, ref, tag)
        if l <= 2 and A.level_marching_ops(l)["on"]:
            A.set_box_plan(l, "marching", shared_cu=True)
            plan = _plan_of(A, l, 1)[1]
            assert plan == _planner(1, *grid, shared_cu=True), (l, plan)
            print(f"216^3 level {l}: marching kernel on the shared-CU plan {plan}")
            _check_marching(A, ref, tag + ("shared-CU", plan))
        del ref
    A.close()


def test_box_plan_argument_checks():
    """sparsh_set_box_plan refuses (SPARSH_EINVAL) every plan the kernels cannot run and leaves the plan in force alone; (0, 0, 0)
    restores the planner's plan, shared_cu its shared-CU plan; a level that is not a box grid and a handle without setup are refused."""
    nx, ny, nz = 63, 64, 5  # 63-point lines: Q4 / TY60 holds the double sweep's region in its threads but not in 64 KiB of LDS
    rp, ci, v = problems.poisson3d(nx, ny, nz)
    B = sa.sp_matrix_mg(rp, ci, v)
    with pytest.raises(sa.SparshError) as e:
        B.set_box_plan(0, 2, 2, 1, 1)
    assert e.value.code == sa.SPARSH_ESTATE
    B.close()
    A = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET))
    assert A.level_double_sweep(0)["grid"] == [nx, ny, nz]
    planned = {k: _plan_of(A, 0, k)[1] for k in (1, 2)}
    assert planned == {k: _planner(k, nx, ny, nz) for k in (1, 2)}

    def refused(kernel, q, ty, cz, what):
        before = {k: _plan_of(A, 0, k) for k in (1, 2)}
        with pytest.raises(sa.SparshError) as e:
            A.set_box_plan(0, kernel, q, ty, cz)
        assert e.value.code == sa.SPARSH_EINVAL and what in str(e.value), (kernel, q, ty, cz, str(e.value))
        assert {k: _plan_of(A, 0, k) for k in (1, 2)} == before

    for kernel in (2, 1):
        refused(kernel, 1, 1, 1, "points per thread")
        refused(kernel, 5, 1, 1, "points per thread")
        refused(kernel, 2, 0, 1, "lines per tile")
        refused(kernel, 2, ny + 1, 1, "lines per tile")
        refused(kernel, 2, 1, 0, "planes per chunk")
        refused(kernel, 2, 1, nz + 1, "planes per chunk")
    assert _max_ty(2, 2, nx, ny) == 28 and _max_ty(1, 2, nx, ny) == 30
    refused(2, 2, 29, 1, "threads")  # (29 + 4) * 63 = 2079 > 2048 points
    refused(1, 2, 31, 1, "threads")  # (31 + 2) * 63 = 2079
    A.set_box_plan(0, 1, 2, 29, 1)  # the marching kernel's region is two lines smaller
    assert _plan_of(A, 0, 1)[1] == (2, 29, 1)
    assert _lds_bytes(2, nx, 60) > 65536 and (60 + 4) * nx <= 4 * BLOCK
    refused(2, 4, 60, 1, "LDS")
    A.set_box_plan(0, 2, 4, 59, 1)
    assert _plan_of(A, 0, 2)[1] == (4, 59, 1)
    with pytest.raises(sa.SparshError) as e:
        A.set_box_plan(0, 4, 2, 1, 1)
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:
        A.set_box_plan(A.nlevels, 2, 2, 1, 1)
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(sa.SparshError) as e:  # the shared-CU plan comes from the planner alone
        A.set_box_plan(0, "marching", 2, 1, 1, shared_cu=True)
    assert e.value.code == sa.SPARSH_EINVAL
    with pytest.raises(ValueError):
        A.set_box_plan(0, "double", shared_cu=True)
    for k in (2, 1):
        A.set_box_plan(0, k)
        assert _plan_of(A, 0, k) == (True, planned[k])
    A.set_box_plan(0, "marching", shared_cu=True)
    assert _plan_of(A, 0, 1)[1] == _planner(1, nx, ny, nz, shared_cu=True)
    A.set_box_plan(0, "marching")
    assert _plan_of(A, 0, 1)[1] == planned[1]
    rng = np.random.default_rng(97)
    x, b = rng.standard_normal(A.level_info(0)["nrow"]), rng.standard_normal(A.level_info(0)["nrow"])
    Ol = oracle.Csr(rp, ci, v)
    assert np.array_equal(A.op_jacobi(0, b, x, 3), oracle.jacobi(Ol, b, x, 2))  # the restored plans run
    A.close()
    # one partial per marching workgroup: 4 x 80 x 60 on one line and one plane per workgroup is 4800 of them, more than the
    # buffers hold (4096 + 8 here: nothing else of this hierarchy reduces over more blocks)
    nx, ny, nz = 4, 80, 60
    rp, ci, v = problems.poisson3d(nx, ny, nz)
    D = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET))
    with pytest.raises(sa.SparshError) as e:
        D.set_box_plan(0, 1, 2, 1, 1)
    assert e.value.code == sa.SPARSH_EINVAL and "partial" in str(e.value) and _plan_of(D, 0, 1)[1] == _planner(1, nx, ny, nz)
    D.set_box_plan(0, 2, 2, 1, 1)  # the double sweep writes no partials
    D.set_box_plan(0, 1, 2, 1, 2)  # 2400 workgroups
    assert _plan_of(D, 0, 1)[1] == (2, 1, 2) and _workgroups(ny, nz, 1, 2) == 2400
    x, b = rng.standard_normal(len(rp) - 1), rng.standard_normal(len(rp) - 1)
    y, d = D.op_spmv_dot(0, x)
    Ol = oracle.Csr(rp, ci, v)
    ax = oracle.spmv(Ol, x)
    assert np.array_equal(y, ax) and _dot_ok(d, x, ax)
    assert np.array_equal(D.op_jacobi(0, b, x, 3), oracle.jacobi(Ol, b, x, 2))
    D.close()
    rp, ci, v = problems.poisson2d(80)
    C = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET))
    assert C.level_double_sweep(0)["grid"] == [0, 0, 0]
    for kernel in (2, 1):
        with pytest.raises(sa.SparshError) as e:
            C.set_box_plan(0, kernel, 2, 1, 1)
        assert e.value.code == sa.SPARSH_EINVAL and "not a box grid" in str(e.value)
        with pytest.raises(sa.SparshError) as e:
            C.set_box_plan(0, kernel)
        assert e.value.code == sa.SPARSH_EINVAL
    C.close()
