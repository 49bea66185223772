"""The box-grid kernels (sdia_box2_kernel, sdia_box1_kernel) on workgroups of 256 and 512 threads.

The workgroup size is a dimension of the launch plan: (threads, points per thread Q, lines per tile TY, planes per chunk CZ).  Forced
plans on small grids -- idle lanes past the region, one-line tiles, a short last chunk, odd nx, reductions over 4 and 8 waves -- are
compared with the CPU oracle on the device's own level operators bit for bit (fused dots to 1e-12 of the sum of magnitudes); then the
argument checks of sparsh_set_box_plan_ex, whole solves under 256- and 512-thread plans, and the plans the setup's timing picks at 96^3.
The helpers are those of test_gpu_box_plans.py with the thread count added.  GPU box only.
"""
import ctypes as C

import numpy as np
import pytest

import oracle
import sparsh_amg_amd as sa
from sparsh_amg_amd import problems
from conftest import hist_tolerance

pytestmark = pytest.mark.gpu

QUIET = dict(print_setup=0, print_solve=0)
THREADS = (256, 512, 1024)


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


def _halo(kernel):
    return 4 if kernel == 2 else 2


def _lds_bytes(kernel, nx, ty):
    """Dynamic LDS of a launch: two region planes (x0, x1) for the double sweep, one for the marching kernel (pad cell per line + 1)."""
    return (2 if kernel == 2 else 1) * ((ty + _halo(kernel)) * (nx + 1) + 1) * 8


def _max_ty(kernel, threads, q, nx, ny):
    """Largest lines per tile the kernel runs with q points per thread (0: none): region rows <= q * threads, LDS <= 64 KiB."""
    ty = min(ny, q * threads // nx - _halo(kernel))
    while ty >= 1 and _lds_bytes(kernel, nx, ty) > 65536:
        ty -= 1
    return max(ty, 0)


def _runs(kernel, grid, threads, plan):
    """box_plan_refusal restated: the kernel can run (threads, Q, TY, CZ) on the grid."""
    nx, ny, nz = grid
    q, ty, cz = plan
    return (threads in THREADS and 2 <= q <= 4 and 1 <= ty <= ny and 1 <= cz <= nz and (ty + _halo(kernel)) * nx <= q * threads
            and _lds_bytes(kernel, nx, ty) <= 65536)


def _plan_of(A, l, kernel):
    d = A.level_double_sweep(l) if kernel == 2 else A.level_marching_ops(l)
    return d["on"], (d["points_per_thread"], d["lines_per_tile"], d["planes_per_chunk"])


def _threads_of(A, l, kernel):
    return A.level_box_threads(l)[0 if kernel == 2 else 1]


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


def _check_marching(A, ref, tag, ran=None):
    """The marching kernel's epilogues: plain sweep (1 and 3 sweeps), SpMV + dot, sweep + dot, pair restriction, prolongation; `ran`
    counts the launches of the two epilogues that only some levels have."""
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
    if ran is not None:
        ran["residual_restrict"] += bool(ref.paired)
        ran["jacobi_prolong"] += bool(ref.prolong)


def _plans(kernel, grid, threads):
    """(Q, TY, CZ) to force: every Q the thread count admits on the grid; TY = 1 and the largest that fits; CZ = 1, 2, nz - 1 (a last
    chunk of one plane), nz."""
    nx, ny, nz = grid
    out = []
    for q in (2, 3, 4):
        top = _max_ty(kernel, threads, q, nx, ny)
        if top < 1:
            continue
        czs = sorted({c for c in (1, 2, nz - 1, nz) if 1 <= c <= nz})
        out += [(q, ty, cz) for ty in sorted({1, top}) for cz in czs]
    return out


GRIDS = {
    "even_nx_odd_nz_40x36x45": lambda: problems.poisson3d(40, 36, 45),
    "odd_nx_27x50x33": lambda: problems.poisson3d(27, 50, 33),
    "stencil7_36x28x31": lambda: _stencil7(36, 28, 31, (-2.5, -2.0, -1.5, 10.0, -0.5, -1.0, -0.7)),
    "line108_108x20x9": lambda: problems.poisson3d(108, 20, 9),  # the line length of the benchmark's levels 1 - 4 in a small box
}


@pytest.mark.parametrize("threads", [256, 512])
@pytest.mark.parametrize("name", list(GRIDS))
def test_forced_plans_bitwise(name, threads):
    """Every box level of the hierarchy under forced plans of `threads` threads, each kernel in turn (the other one on its planner's
    plan): all of _plans on every level.  (No plan here launches more than ny * nz <= 4096 marching workgroups: all fit the
    reduction buffers.)"""
    rp, ci, v = GRIDS[name]()
    A = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET))
    rng = np.random.default_rng(191)
    boxes = [l for l in range(A.nlevels - 1) if A.level_double_sweep(l)["on"]]
    assert boxes and boxes[0] == 0, [A.level_double_sweep(l) for l in range(A.nlevels)]
    ran = {1: [], 2: []}
    epilogues = {"residual_restrict": 0, "jacobi_prolong": 0}
    for l in boxes:
        grid = tuple(A.level_double_sweep(l)["grid"])
        ref = _LevelRef(A, l, grid, rng)
        assert A.level_marching_ops(l)["on"], (name, l)
        assert A.level_box_threads(l) == (1024, 1024)
        for kernel in (2, 1):
            planned = _plan_of(A, l, kernel)[1]
            for plan in _plans(kernel, grid, threads):
                assert _runs(kernel, grid, threads, plan)
                A.set_box_plan(l, kernel, *plan, threads=threads)
                assert _plan_of(A, l, kernel) == (True, plan) and _threads_of(A, l, kernel) == threads, (name, l, kernel, plan)
                tag = (name, l, grid, kernel, threads, plan)
                if kernel == 2:
                    _check_double(A, ref, tag)
                else:
                    _check_marching(A, ref, tag, epilogues)
                ran[kernel].append((l, plan))
            A.set_box_plan(l, kernel)  # back to the planner's plan, on 1024 threads
            assert _plan_of(A, l, kernel)[1] == planned and _threads_of(A, l, kernel) == 1024
    print(f"{name} on {threads} threads: marching launches with the pair restriction {epilogues['residual_restrict']}, with the prolongation "
          f"{epilogues['jacobi_prolong']}")
    if len(boxes) > 1:  # every box level but the finest prolongates in its last post-sweep
        assert epilogues["jacobi_prolong"] > 0, (name, threads)
    if name in ("even_nx_odd_nz_40x36x45", "line108_108x20x9"):  # Poisson on an even line: level 0's aggregates are row pairs
        assert epilogues["residual_restrict"] > 0, (name, threads)
    nx0, ny0 = A.level_double_sweep(0)["grid"][:2]
    for kernel in (2, 1):
        level0 = [p for l, p in ran[kernel] if l == 0]
        assert level0 and (len(boxes) == 1 or len(ran[kernel]) > len(level0)), (name, kernel, ran[kernel])  # level 0 and coarser box levels ran
        fits = {q for q in (2, 3, 4) if _max_ty(kernel, threads, q, nx0, ny0) >= 1}  # (108-point lines: 256 threads at Q = 2 hold no region)
        assert len(fits) >= 2 and {p[0] for p in level0} == fits, (name, kernel, level0)
        print(f"{name} kernel {kernel} on {threads} threads: {len(level0)} plans on level 0, {len(ran[kernel]) - len(level0)} on coarser levels")
    A.close()


def test_box_threads_argument_checks():
    """sparsh_set_box_plan_ex refuses a region larger than Q * threads points and every thread count but 256, 512 and 1024, and leaves
    the plan in force alone; sparsh_set_box_plan still means 1024 threads."""
    nx, ny, nz = 40, 36, 45
    rp, ci, v = problems.poisson3d(nx, ny, nz)
    A = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET))
    assert A.level_double_sweep(0)["grid"] == [nx, ny, nz] and A.level_box_threads(0) == (1024, 1024)

    def state():
        return [(_plan_of(A, 0, k), _threads_of(A, 0, k)) for k in (1, 2)]

    def refused(kernel, threads, q, ty, cz, what):
        before = state()
        with pytest.raises(sa.SparshError) as e:
            A.set_box_plan(0, kernel, q, ty, cz, threads=threads)
        assert e.value.code == sa.SPARSH_EINVAL and what in str(e.value), (kernel, threads, q, ty, cz, str(e.value))
        assert state() == before

    A.set_box_plan(0, 2, 3, 5, 4, threads=512)  # a plan of its own in force, so that "unchanged" is not "the default"
    A.set_box_plan(0, 1, 2, 3, 7, threads=256)
    assert state() == [((True, (2, 3, 7)), 256), ((True, (3, 5, 4)), 512)]
    for kernel in (2, 1):
        for threads in (0, 64, 128, 255, 384, 768, 2048, -256):
            refused(kernel, threads, 2, 1, 1, "threads per workgroup")
        for threads in (256, 512):
            for q in (2, 3, 4):
                top = _max_ty(kernel, threads, q, nx, ny)
                if top >= ny:  # (512 threads at Q = 4 hold every line of a plane)
                    continue
                assert top >= 1
                refused(kernel, threads, q, top + 1, 1, "threads")  # one line more than q * threads points hold
                assert (top + 1 + _halo(kernel)) * nx > q * threads >= (top + _halo(kernel)) * nx
        refused(kernel, 256, 5, 1, 1, "points per thread")
        refused(kernel, 512, 2, 0, 1, "lines per tile")
        refused(kernel, 512, 2, 1, nz + 1, "planes per chunk")
    # the largest region 1024 threads hold at Q = 2 does not fit 512: the old entry point takes it, so it means 1024
    top = _max_ty(2, 1024, 2, nx, ny)
    assert top > _max_ty(2, 512, 2, nx, ny)
    refused(2, 512, 2, top, 3, "threads")
    sa._check(sa.lib.sparsh_set_box_plan(A._h, 0, 2, 2, top, 3))
    assert state()[1] == ((True, (2, top, 3)), 1024)
    sa._check(sa.lib.sparsh_set_box_plan_ex(A._h, 0, 1, 512, 3, 2, 5))
    assert state()[0] == ((True, (3, 2, 5)), 512)
    sa._check(sa.lib.sparsh_set_box_plan(A._h, 0, 1, 3, 2, 5))
    assert state()[0] == ((True, (3, 2, 5)), 1024)
    a, b = C.c_int(-1), C.c_int(-1)
    sa._check(sa.lib.sparsh_level_box_threads(A._h, 0, C.byref(a), C.byref(b)))
    assert (a.value, b.value) == (1024, 1024)
    with pytest.raises(sa.SparshError) as e:
        A.level_box_threads(A.nlevels)
    assert e.value.code == sa.SPARSH_EINVAL
    rng = np.random.default_rng(197)
    x, b = rng.standard_normal(nx * ny * nz), rng.standard_normal(nx * ny * nz)
    A.set_box_plan(0, 2, 4, 2, 44, threads=256).set_box_plan(0, 1, 4, 3, 44, threads=256)
    assert np.array_equal(A.op_jacobi(0, b, x, 3), oracle.jacobi(oracle.Csr(rp, ci, v), b, x, 2))
    A.close()


def _force_threads(A, boxes, threads, double_cz, marching_cz):
    """Every box level on `threads`-thread plans of several planes per chunk: double sweep Q3 / largest TY, marching kernel Q4 / half the
    largest TY."""
    for l in boxes:
        nx, ny, nz = A.level_double_sweep(l)["grid"]
        A.set_box_plan(l, 2, 3, _max_ty(2, threads, 3, nx, ny), min(double_cz, nz), threads=threads)
        A.set_box_plan(l, 1, 4, max(1, _max_ty(1, threads, 4, nx, ny) // 2), min(marching_cz, nz), threads=threads)
        assert A.level_box_threads(l) == (threads, threads)


def test_solves_under_small_workgroups():
    """AMG and PCG with every box level on 256-thread and then 512-thread plans: AMG history and x bitwise those of the same handle with
    the box kernels off, PCG within hist_tolerance of the oracle; the captured PCG iteration gives the eager run's bits, also after the
    thread count changes (the graph is dropped and captured again)."""
    rp, ci, v = problems.poisson3d(40, 36, 45)
    n = len(rp) - 1
    b = np.random.default_rng(193).standard_normal(n)
    A = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET))
    G = sa.sp_matrix_mg(rp, ci, v).set_double_sweep(2).set_marching_ops(2).setup(sa.default_params(**QUIET, use_graph=1))
    boxes = [l for l in range(A.nlevels - 1) if A.level_double_sweep(l)["on"]]
    assert len(boxes) >= 2

    def run(H, method):
        x = np.zeros(n)
        h, rc = H.solve(method, b, x)
        assert rc == 0 and len(h) > 1
        return np.array(h), x

    A.set_double_sweep(0).set_marching_ops(0)
    assert not A.level_double_sweep(0)["on"] and not A.level_marching_ops(0)["on"]
    h0, x0 = run(A, "amg")
    A.set_double_sweep(2).set_marching_ops(2)
    O = oracle.Csr(rp, ci, v)
    xo, ho = oracle.solve("pcg", O, b)
    for threads in (256, 512):
        _force_threads(A, boxes, threads, 4, 7)
        _force_threads(G, boxes, threads, 4, 7)
        h_amg, x_amg = run(A, "amg")
        assert np.array_equal(h_amg, h0) and np.array_equal(x_amg, x0), threads
        h_pcg, x_pcg = run(A, "pcg")
        assert len(h_pcg) == len(ho), (threads, len(h_pcg), len(ho))
        assert np.all(np.abs(h_pcg - ho) / ho <= hist_tolerance(ho)), threads
        assert np.linalg.norm(x_pcg - xo) <= 1e-8 * np.linalg.norm(xo)
        for _ in range(2):  # captured, then replayed: after 256 -> 512 the graph of the old plans must not be replayed
            hg, xg = run(G, "pcg")
            assert np.array_equal(hg, h_pcg) and np.array_equal(xg, x_pcg), threads
    A.close()
    G.close()


def test_timed_plans_96():
    """Default setup at 96^3 (885 k rows: the setup times the candidate plans on every box level of >= 60 000 rows): whatever it chose
    on a level that runs a box kernel is a plan the kernel can run, level_box_threads reports its thread count, and the operators
    under it are bitwise the oracle's."""
    rp, ci, v = problems.poisson3d(96)
    A = sa.sp_matrix_mg(rp, ci, v).setup(sa.default_params(**QUIET))
    del rp, ci, v
    rng = np.random.default_rng(195)
    on, timed = [], []
    for l in range(A.nlevels - 1):
        d2, d1 = A.level_double_sweep(l), A.level_marching_ops(l)
        if d2["double_sweep_us"] > 0 or d1["marching_kernel_us"] > 0:
            timed.append(l)
        if d2["on"] or d1["on"]:
            on.append(l)
        if d2["grid"][0] > 0:
            print(f"96^3 level {l} grid {d2['grid']}: double sweep {'on' if d2['on'] else 'off'} threads {_threads_of(A, l, 2)} plan "
                  f"{_plan_of(A, l, 2)[1]} ({d2['two_single_sweeps_us']} / {d2['double_sweep_us']} us), marching kernel "
                  f"{'on' if d1['on'] else 'off'} threads {_threads_of(A, l, 1)} plan {_plan_of(A, l, 1)[1]} "
                  f"({d1['table_kernel_us']} / {d1['marching_kernel_us']} us)")
    assert 0 in timed and on
    assert all(A.level_info(l)["nrow"] >= 60000 for l in timed)
    for l in on:
        grid = tuple(A.level_double_sweep(l)["grid"])
        for kernel in (2, 1):
            if _plan_of(A, l, kernel)[0]:
                assert _runs(kernel, grid, _threads_of(A, l, kernel), _plan_of(A, l, kernel)[1]), (l, kernel)
        ref = _LevelRef(A, l, grid, rng)
        tag = ("96^3", l, grid, A.level_box_threads(l))
        if A.level_double_sweep(l)["on"]:
            _check_double(A, ref, tag, zero_sweeps=(3, 4))
        if A.level_marching_ops(l)["on"]:
            _check_marching(A, ref, tag)
        del ref
    A.close()
