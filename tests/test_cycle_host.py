"""W- and K-cycles at chosen levels: the C ABI arguments, the WK levels and visit counts, the visit cap and the refusals that need
no device -- host only (sparsh_setup_host), no GPU.

Contract: level l is a WK level when 1 <= l < last and l % stride == 0; a level is visited
2^(number of WK levels <= l) times per cycle; more than 1024 visits per cycle, all levels together, are SPARSH_EINVAL at the solve.
"""
import numpy as np
import pytest

import sparsh_amg_amd as sa
from sparsh_amg_amd import problems

QUIET = dict(print_setup=0, print_solve=0)
GRID = problems.poisson2d(120)  # 14 400 rows: pairwise aggregation halves it per level


def host_handle(levels, **kw):
    """a hierarchy of exactly `levels` levels: coarsening goes on down to a handful of rows, max_levels ends it"""
    A = sa.sp_matrix_mg(*GRID).setup(sa.default_params(**QUIET, max_levels=levels, limit_upper=4, limit_lower=2, **kw), host_only=True)
    assert A.nlevels == levels
    return A


def expected(levels, stride):
    last = levels - 1
    wk = [1 <= l < last and l % stride == 0 for l in range(levels)]
    visits = [2 ** sum(wk[: l + 1]) for l in range(levels)]
    return wk, visits


def refused(call):
    with pytest.raises(sa.SparshError) as e:
        call()
    assert e.value.code == sa.SPARSH_EINVAL, e.value
    return str(e.value)


def test_set_cycle_arguments():
    A = sa.sp_matrix_mg(*GRID)
    assert A.cycle_info() == dict(kind="v", stride=3, nlevels_wk=0, level_visits=0, bytes=0)  # before any setup
    A.set_cycle("k", 2)
    assert A.cycle_info()["kind"] == "k" and A.cycle_info()["stride"] == 2
    for kind, stride in ((3, 1), (-1, 1), (sa.SPARSH_CYCLE_W, 9), (sa.SPARSH_CYCLE_W, -1), (7, 12)):
        refused(lambda: A.set_cycle(kind, stride))
        info = A.cycle_info()
        assert (info["kind"], info["stride"]) == ("k", 2), (kind, stride, info)  # a refused call changes nothing
    A.set_cycle("w")  # stride 0: the default of 3
    assert (A.cycle_info()["kind"], A.cycle_info()["stride"]) == ("w", 3)
    for s in range(1, 9):
        A.set_cycle("w", s)
        assert A.cycle_info()["stride"] == s
    A.set_cycle("v")
    assert (A.cycle_info()["kind"], A.cycle_info()["stride"]) == ("v", 3)
    assert sa.lib.sparsh_set_cycle(None, 1, 1) == sa.SPARSH_EINVAL  # null handle
    with pytest.raises(sa.SparshError):  # level queries want the host setup
        A.level_cycle(0)


@pytest.mark.parametrize("kind", ["w", "k"])
def test_wk_levels_and_visits_of_a_six_level_hierarchy(kind):
    A = host_handle(6)
    for stride in (1, 2, 3):
        A.set_cycle(kind, stride)
        wk, visits = expected(6, stride)
        got = [A.level_cycle(l) for l in range(6)]
        assert [g[0] for g in got] == wk, (stride, got)
        assert [g[1] for g in got] == visits, (stride, got)
        info = A.cycle_info()
        assert info["nlevels_wk"] == sum(wk) and info["level_visits"] == sum(visits) and info["bytes"] == 0
    # written out once, so that the test does not rest on expected() alone
    A.set_cycle(kind, 1)
    assert [A.level_cycle(l) for l in range(6)] == [(False, 1), (True, 2), (True, 4), (True, 8), (True, 16), (False, 16)]
    A.set_cycle(kind, 2)
    assert [A.level_cycle(l) for l in range(6)] == [(False, 1), (False, 1), (True, 2), (False, 2), (True, 4), (False, 4)]
    A.set_cycle(kind, 3)
    assert [A.level_cycle(l) for l in range(6)] == [(False, 1), (False, 1), (False, 1), (True, 2), (False, 2), (False, 2)]
    A.set_cycle("v", 1)  # the V-cycle has no WK level whatever the stride
    assert [A.level_cycle(l) for l in range(6)] == [(False, 1)] * 6
    assert A.cycle_info()["nlevels_wk"] == 0 and A.cycle_info()["level_visits"] == 6
    refused(lambda: A.level_cycle(6))
    refused(lambda: A.level_cycle(-1))


def test_visit_cap():
    """12 levels: stride 1 makes levels 1..10 recurse, 1 + 2 + ... + 1024 + 1024 = 3071 visits; stride 2 makes 126"""
    A = host_handle(12)
    n = A.nrow
    b, x = np.ones(n), np.zeros(n)
    A.set_cycle("k", 1)
    assert A.cycle_info()["level_visits"] == 3071
    for call in (lambda: A.solve("fcg", b, x), lambda: A.solve("amg", b, x), lambda: A.op_precond(b), lambda: A.vcycle(b, x, iterations=1)):
        msg = refused(call)
        assert "1024" in msg and "largest stride that fits is 8" in msg and "smallest 2" in msg, msg
    A.set_cycle("w", 1)
    assert "largest stride that fits is 8" in refused(lambda: A.solve("pcg", b, x))
    A.solve("cg", b, x, allow=(sa.SPARSH_ESTATE,))  # no preconditioner, no cycle: only the missing device setup is in the way
    A.set_cycle("w", 2)
    assert A.cycle_info()["level_visits"] == 126
    with pytest.raises(sa.SparshError) as e:  # fits: what is left is the missing device setup
        A.solve("pcg", b, x)
    assert e.value.code == sa.SPARSH_ESTATE


def test_k_cycle_is_refused_by_the_methods_that_need_a_fixed_operator():
    A = host_handle(6)
    n = A.nrow
    b, x = np.ones(n), np.zeros(n)
    A.set_cycle("k", 2)
    for method in ("pcg", "pbicg", "pgmres"):
        assert "SPARSH_FCG" in refused(lambda: A.solve(method, b, x)), method
        assert "SPARSH_FCG" in refused(lambda: A.solve_dev(method, None, None)), method
    assert "SPARSH_FCG" in refused(lambda: A.krylov_init_dev("pcg", None, None))
    for method in ("fcg", "amg", "cg", "bicg", "gmres"):  # accepted: only the device setup is missing
        with pytest.raises(sa.SparshError) as e:
            A.solve(method, b, x)
        assert e.value.code == sa.SPARSH_ESTATE, method
    A.set_cycle("w", 2)  # a fixed operator: every method takes it
    for method in ("pcg", "pbicg", "pgmres", "fcg"):
        with pytest.raises(sa.SparshError) as e:
            A.solve(method, b, x)
        assert e.value.code == sa.SPARSH_ESTATE, method
    # before any setup the K refusal stands too
    B = sa.sp_matrix_mg(*GRID).set_cycle("k")
    assert "SPARSH_FCG" in refused(lambda: B.solve("pcg", b, x))


@pytest.mark.parametrize("kind", ["w", "k"])
def test_fp32_preconditioner_and_block_solves_are_refused(kind):
    A = host_handle(6, precond_fp32=1)
    n = A.nrow
    b, x = np.ones(n), np.zeros(n)
    A.set_cycle(kind, 2)
    assert "precond_fp32" in refused(lambda: A.solve("fcg", b, x))
    assert "precond_fp32" in refused(lambda: A.op_precond(b))
    A.set_cycle("v")
    with pytest.raises(sa.SparshError) as e:
        A.solve("fcg", b, x)
    assert e.value.code == sa.SPARSH_ESTATE
    B = host_handle(6).set_cycle(kind, 2)
    msg = refused(lambda: B.solve_multi("pcg", np.ones((n, 2)), np.zeros((n, 2))))
    assert "SPARSH_CYCLE_V" in msg, msg
