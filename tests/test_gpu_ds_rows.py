"""Directed search with constraint rows on the device (run with -m gpu): mrbf_ds_direction_rows on the seeded QPs of
tests/ds_rows_util.py against the stored results of the host mirror (tests/golden/ds_rows_host.npz, written by
tests/golden/make_ds_rows_host.py), with the certificate of every solution; bit identity across runs, batch positions, pointer kinds
and -- without constraint rows -- with mrbf_ds_direction; the statuses; the refusals; mrbf_ds_criticality_rows against mrbf_eval +
mrbf_ds_direction_rows; and one whole constrained step through the routing.

The bound on z = G d: |z_dev - z_host|_i <= MARGIN (d + K) 2^-52 (sum_j |G_ij| + |r_i|) with MARGIN = 8 x the stored "worst_ratio", the
largest ratio of the host mirror against itself with the columns of W permuted on these same QPs."""
import numpy as np
import pytest

from tests import ds_rows_util as ru
from tests import ds_util
from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import torch

    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib, descent
    from morbit.jl_amd import surrogates as sg


@pytest.fixture(scope="module")
def golden():
    return ru.load_golden()


@pytest.mark.parametrize("d,k,m_eq,m_in", ru.GPU_SHAPES)
def test_direction_rows_shapes(d, k, m_eq, m_in, golden):
    K = k + m_eq + m_in
    margin = 8.0 * float(golden["worst_ratio"])
    G, r, X, lb, ub, Ae, be, Ai, bi = ru.make_batch(d, k, m_eq, m_in)
    rc, D, C, om, mu, status, iters = descent.ds_directions_rows_many(G, r, X, lb, ub, Ae, be, Ai, bi)
    assert rc == 0
    key = ru.key(d, k, m_eq, m_in)
    assert np.array_equal(status, golden[key + "_status"]) and np.all(status == _lib.DS_OK), status
    assert np.all(iters[:, 0] <= 8 * (d + K) + 16) and np.all(iters[:, 1] <= iters[:, 0])
    worst = kkt = 0.0
    for p in range(ru.N_QP):
        lo, hi = descent._sd_box(X[p], lb, ub)
        kkt = max(kkt, ru.check_solution(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p], D[p], C[p], om[p], mu[p], (d, k, m_eq, m_in, p)))
        bound = ru.z_bound(G[p], r[p], K, margin)
        diff = np.abs(C[p, :k] - golden[key + "_z"][p])
        worst = max(worst, float(np.max(diff / bound)) * margin)
        print("%s QP %d: ratio %.3g" % (key, p, float(np.max(diff / bound)) * margin))
        assert np.all(diff <= bound), (key, p, diff, bound)
        assert abs(om[p] - golden[key + "_omega"][p]) <= float(np.max(bound)), (key, p, om[p])
    print("%s: |z - z_host| <= %.3g (d + K) eps scale (margin %.3g), certificate <= %.1e, iterations <= %.2f (d + K)"
          % (key, worst, margin, kkt, iters[:, 0].max() / (d + K)))


def _call(ctx, G, r, X, lb, ub, Ae, be, Ai, bi, device=False, want_mult=True, want_iters=True):
    """mrbf_ds_direction_rows with host arrays or with device tensors for every array; returns host copies of all six outputs"""
    nq, k, n = G.shape
    m_eq, m_in = be.shape[1], bi.shape[1]
    K = k + m_eq + m_in
    host = [np.ascontiguousarray(np.transpose(G, (0, 2, 1))), np.ascontiguousarray(r), np.ascontiguousarray(X),
            np.ascontiguousarray(np.broadcast_to(lb, (nq, n))), np.ascontiguousarray(np.broadcast_to(ub, (nq, n))),
            np.ascontiguousarray(Ae), np.ascontiguousarray(be), np.ascontiguousarray(Ai), np.ascontiguousarray(bi)]
    outs = [np.empty((nq, n)), np.empty((nq, K)), np.empty(nq), np.empty((nq, K)), np.empty(nq, dtype=np.int32), np.empty((nq, 2), dtype=np.int32)]
    if device:
        ins = [torch.from_numpy(a).cuda() for a in host]
        bufs = [torch.from_numpy(a).cuda() for a in outs]
    else:
        ins, bufs = host, outs
    p = _lib.as_ptr
    ptrs = [p(a) for a in ins]
    for i, m in ((5, m_eq), (6, m_eq), (7, m_in), (8, m_in)):      # NULL where the count is 0
        if m == 0:
            ptrs[i] = None
    rc = ctx.lib.mrbf_ds_direction_rows(ctx.h, nq, n, k, m_eq, m_in, *ptrs, p(bufs[0]), p(bufs[1]), p(bufs[2]), p(bufs[3]) if want_mult else None,
                                        p(bufs[4]), p(bufs[5]) if want_iters else None)
    assert rc == 0
    if device:
        torch.cuda.synchronize()
        return [b.cpu().numpy() for b in bufs]
    return bufs


def _same(a, b, rows_a=slice(None), rows_b=slice(None), which=range(6)):
    return all(np.array_equal(a[i][rows_a], b[i][rows_b], equal_nan=True) for i in which)


@pytest.mark.parametrize("d,k,m_eq,m_in", [(65, 2, 2, 3), (7, 5, 3, 8), (300, 2, 1, 1)])
def test_bits(d, k, m_eq, m_in):
    ctx = _lib.default_context()
    b = ru.make_batch(d, k, m_eq, m_in)
    first = _call(ctx, *b)
    assert _same(first, _call(ctx, *b))                                    # the same call twice
    assert _same(first, _call(ctx, *b, device=True))                       # host and device pointers
    rev = slice(None, None, -1)
    per_qp = lambda s: [a if i in (3, 4) else a[s] for i, a in enumerate(b)]
    assert _same(first, _call(ctx, *per_qp(rev)), rows_b=rev)              # QP p at position 36 - p, among other neighbours
    for p in (0, 17, 36):                                                  # ... and alone
        assert _same(_call(ctx, *per_qp(slice(p, p + 1))), first, rows_b=slice(p, p + 1)), p
    # mult_out and iters_out may be NULL: the other outputs keep their bits
    assert _same(first, _call(ctx, *b, want_mult=False, want_iters=False), which=(0, 1, 2, 4))


@pytest.mark.parametrize("d,k", [(65, 3), (7, 16), (300, 5)])
def test_without_rows_the_bits_are_mrbf_ds_direction(d, k):
    ctx = _lib.default_context()
    G, r, X, lb, ub = ds_util.make_batch(d, k)
    nq = G.shape[0]
    rows = _call(ctx, G, r, X, lb, ub, np.zeros((nq, 0, d)), np.zeros((nq, 0)), np.zeros((nq, 0, d)), np.zeros((nq, 0)))
    rc, D, Z, om, mu, status, iters = descent.ds_directions_many(G, r, X, lb, ub, ctx=ctx)
    assert rc == 0
    assert _same(rows, [D, Z, om, mu, status, iters])


def test_statuses_on_the_device():
    rng = np.random.default_rng(4)
    d, k, m_eq, m_in, nq = 9, 3, 1, 2, 8
    G = rng.standard_normal((nq, k, d))
    r = -rng.uniform(0.1, 1.0, (nq, k))
    X = np.full((nq, d), 0.5)
    lb, ub = np.zeros(d), np.ones(d)
    Ae, Ai = rng.standard_normal((nq, m_eq, d)), rng.standard_normal((nq, m_in, d))
    be, bi = np.zeros((nq, m_eq)), np.tile([0.0, 0.3], (nq, 1))
    r[1, 0] = 0.0          # CRITICAL: a zero
    r[2, 2] = 0.7          # CRITICAL: a positive entry
    r[3, 1] = np.nan       # CRITICAL: a NaN
    X[4, 5] = 2.5          # INFEASIBLE: l_5 > u_5
    be[5, 0] = 0.3         # NO_START: d = 0 misses the equality
    bi[6, 1] = -0.2        # NO_START: d = 0 violates an inequality
    be[7, 0] = 1e-12 * np.abs(Ae[7, 0]).sum()      # within START_TOL = 1e-10 of the row's scale: clamped, solved
    bi[7, 0] = -1e-13 * np.abs(Ai[7, 0]).sum()
    rc, D, C, om, mu, status, iters = descent.ds_directions_rows_many(G, r, X, lb, ub, Ae, be, Ai, bi)
    assert rc == 0
    assert list(status) == [_lib.DS_OK] + [_lib.DS_CRITICAL] * 3 + [_lib.DS_INFEASIBLE, _lib.DS_NO_START, _lib.DS_NO_START, _lib.DS_OK]
    for p in (1, 2, 3):
        assert not D[p].any() and not C[p].any() and om[p] == 0.0 and not mu[p].any()
    assert not D[4].any() and om[4] == -np.inf
    for p in (5, 6):
        assert np.all(np.isnan(D[p])) and np.isnan(om[p]) and np.all(np.isnan(C[p])) and np.all(np.isnan(mu[p]))
    for p in (0, 7):
        lo, hi = descent._sd_box(X[p], lb, ub)
        h = np.concatenate([np.zeros(k), be[p], bi[p]]) if p == 0 else np.concatenate([np.zeros(k), [0.0], [0.0, 0.3]])    # clamped
        ru.check_solution(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p], D[p], C[p], om[p], mu[p], p, h=h)
    for p in range(nq):      # every status is the host mirror's
        lo, hi = descent._sd_box(X[p], lb, ub)
        assert descent._ds_active_set_rows(G[p], r[p], lo, hi, Ae[p], be[p], Ai[p], bi[p])[4] == status[p], p


def test_refusals_write_nothing():
    ctx = _lib.default_context()
    d, k, nq = 5, 2, 3
    rng = np.random.default_rng(1)
    Gl, r, X = rng.standard_normal((nq, d, k)), -np.ones((nq, k)), np.full((nq, d), 0.5)
    LB, UB = np.zeros((nq, d)), np.ones((nq, d))
    A1, b1 = rng.standard_normal((nq, 1, d)), np.zeros((nq, 1))
    p = _lib.as_ptr

    def call(h=ctx.h, n_qp=nq, dd=d, kk=k, me=1, mi=1, G=Gl, Ae=A1, bi=b1, d_out=True, c_out=True):
        outs = [np.full((nq, d), 7.0), np.full((nq, 17), 7.0), np.full(nq, 7.0), np.full((nq, 17), 7.0), np.full(nq, 7, dtype=np.int32),
                np.full((nq, 2), 7, dtype=np.int32)]
        rc = ctx.lib.mrbf_ds_direction_rows(h, n_qp, dd, kk, me, mi, p(G), p(r), p(X), p(LB), p(UB), p(Ae), p(b1), p(A1), p(bi),
                                            p(outs[0]) if d_out else None, p(outs[1]) if c_out else None, p(outs[2]), p(outs[3]),
                                            p(outs[4]), p(outs[5]))
        assert all(np.all(o == 7) for o in outs), rc
        return rc

    assert call(h=None) == -1
    assert call(n_qp=0) == -3 and call(dd=0) == -4 and call(dd=4097) == -4 and call(kk=0) == -5 and call(kk=17) == -5
    assert call(me=-1) == -6 and call(mi=-1) == -7 and call(kk=8, me=4, mi=5) == -8
    assert call(G=None) == -9 and call(Ae=None) == -14 and call(bi=None) == -17 and call(d_out=False) == -18 and call(c_out=False) == -19
    for rc in (-3, -4, -5, -6, -7, -8, -9, -14, -17, -18, -19):
        assert ctx.lib.mrbf_dispatch_after(_lib.ENTRY_DS_ROWS, rc) == 0      # errors, not "take the host method"


def two_parabolas(X):
    X = np.atleast_2d(X)
    return np.stack([np.sum((X - 1.0) ** 2, axis=1), np.sum((X + 1.0) ** 2, axis=1)], axis=1)


def ball(X):
    """a modelled inequality: inside the ball of radius sqrt(4 d) around the origin (slack at every site of the box [-2, 2]^d but its corners)"""
    X = np.atleast_2d(X)
    return (np.sum(X ** 2, axis=1) / X.shape[1] - 4.0)[:, None]


def _fit(f, C):
    return pkg.update_model(pkg.RbfConfig(kernel="cubic", polynomial_degree=1), C, f(C))


def _containers():
    rng = np.random.default_rng(21)
    d = 7
    C = rng.uniform(-2.0, 2.0, (40, d))
    both = _fit(two_parabolas, C)                                             # a fitted two-output cubic model (d = 7, n = 40)
    con = _fit(ball, rng.uniform(-2.0, 2.0, (45, d)))
    linear = (sg.SurrogateContainer(objectives=[sg.RefSurrogate(both, [0, 1])]),
              (np.ones((1, d)), np.zeros(1), np.linspace(1.0, -1.0, d)[None, :], np.array([0.4])))      # one equality, one inequality
    modelled = (sg.SurrogateContainer(objectives=[sg.RefSurrogate(both, [0, 1])], nl_ineq_constraints=[sg.RefSurrogate(con, [0])]), None)
    return d, linear, modelled


def test_criticality_rows_equals_eval_plus_direction_rows(golden):
    """The device call assembles its rows with sd_assemble_kernel; the rows it is compared with here are `_sd_host_rows`' (NumPy sums of
    mrbf_eval's values and Jacobians), whose right-hand sides differ in the last bits: the z bound applies, not bit identity."""
    margin = 8.0 * float(golden["worst_ratio"])
    d, linear, modelled = _containers()
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    rng = np.random.default_rng(5)
    for sc, lin in (linear, modelled):
        plan = sg.container_plan(sc)
        for trial in range(3):
            x_n = np.linspace(-1.5, 1.5, d) * (1.0, 0.5, 0.9)[trial]            # on the linear equality (sum = 0), inside the ball
            r = -rng.uniform(0.1, 1.0, 2) * (1.0 if trial % 2 else 30.0)
            rc, om, dd, info, mu = descent.ds_criticality_rows_device(plan, x_n, x_n, lb, ub, r, lin, want_mult=True)
            assert rc == 0 and info["status"] == _lib.DS_OK and info["ms_total"] > 0, (rc, info)
            G, A_eq, b_eq, A_in, b_in = descent._sd_host_rows(sc, None, x_n, x_n, lin)
            K = 2 + b_eq.size + b_in.size
            assert mu.shape == (K,)
            rc2, D, C, om2, mu2, status, iters = descent.ds_directions_rows_many(G[None], r[None], x_n[None], lb, ub, A_eq[None], b_eq[None],
                                                                                 A_in[None], b_in[None], ctx=plan["models"][0].ctx)
            assert rc2 == 0 and status[0] == _lib.DS_OK
            bound = ru.z_bound(G, r, K, margin)
            print("trial %d: |z - z'| / bound = %.3g" % (trial, float(np.max(np.abs(G @ dd - C[0, :2]) / bound))))
            assert np.all(np.abs(G @ dd - C[0, :2]) <= bound) and abs(om - om2[0]) <= float(np.max(bound))
            assert info["omega"] == om
            lo, hi = descent._sd_box(x_n, lb, ub)
            W = np.vstack([G, A_eq, A_in])
            h = np.concatenate([np.zeros(2), np.where(np.abs(b_eq) <= 1e-10 * np.abs(A_eq).sum(axis=1), 0.0, b_eq), b_in])     # clamped
            ru.check_solution(G, r, lo, hi, A_eq, b_eq, A_in, b_in, dd, W @ dd, max(0.0, -float(np.max((W @ dd)[:2]))), mu, trial, h=h)
    # a start off the equality: -2 with NO_START, "take the host method"
    sc, lin = linear
    plan = sg.container_plan(sc)
    rc, om, dd, info = descent.ds_criticality_rows_device(plan, np.full(d, 0.3), np.full(d, 0.3), lb, ub, -np.ones(2), lin)
    assert rc == -2 and info["status"] == _lib.DS_NO_START and _lib.load().mrbf_dispatch_after(_lib.ENTRY_DS_ROWS, rc) == 1


def test_whole_constrained_step_through_the_routing():
    d, linear, _ = _containers()
    sc, lin = linear
    lb, ub = np.full(d, -2.0), np.full(d, 2.0)
    x = np.linspace(-1.5, 1.5, d)
    fx = two_parabolas(x)[0]
    cfg = descent.DirectedSearchConfig(reference_point=[-1.0, -1.0], constraint_rows="device")
    s1, s2 = {}, {}
    om, dn = descent.get_criticality_ds(cfg, sc, None, x, x, fx, 0.5, lb, ub, lin=lin, stats=s1)
    assert s1["path"] == "device" and s1["status"] == _lib.DS_OK and om > 0, s1
    om2, xp, mxp, step = descent.compute_descent_step_ds(cfg, sc, None, x, x, 0.5, lb, ub, om, dn, lin=lin, stats=s2)
    assert step > 0 and abs(float(np.sum(xp))) <= 1e-12                           # the linear equality is kept by x_plus
    assert float(lin[2][0] @ xp) <= 0.4 + 1e-12
    # the default configuration keeps the host route
    s3 = {}
    descent.get_criticality_ds(descent.DirectedSearchConfig(reference_point=[-1.0, -1.0]), sc, None, x, x, fx, 0.5, lb, ub, lin=lin, stats=s3)
    assert s3["path"] == "reference" and s3["method"] == "slsqp"
