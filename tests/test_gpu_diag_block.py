"""The 128 x 128 diagonal-block core (csrc/chol_diag_core.hpp, run with -m gpu): one core, the same bits whoever calls it -- the
stand-alone launch (mrbf_debug_potrf impl 2), the persistent factorisation (impl 3) and the one-launch small fit, whose Cholesky-QR of
the centred coordinates (the Gx block) takes the full core for 64 < d <= 128 and block64 up to d = 64."""
import ctypes

import numpy as np
import pytest

from tests.conftest import has_gpu

pytestmark = pytest.mark.gpu

if has_gpu():
    import morbit.jl_amd as pkg
    from morbit.jl_amd import _lib
    from tests.test_gpu_fit_batch import _free, _spec, assert_same_model, batch, single
from oracle import rbf_oracle as orc


@pytest.fixture(scope="module")
def ctx():
    c = pkg.Context()
    yield c
    c.close()


def _spd(n):
    """as tests/test_gpu_parity.py::test_builtin_cholesky_matches_lapack builds it"""
    rng = np.random.Generator(np.random.PCG64(n))
    G = rng.standard_normal((n, n + 20))
    return G @ G.T / n + np.eye(n)


def _potrf(ctx, A, impl):
    F = np.asfortranarray(A.copy())
    info = ctypes.c_int32(-7)
    ctx.check(ctx.lib.mrbf_debug_potrf(ctx.h, A.shape[0], _lib.as_ptr(F), impl, ctypes.byref(info), None))
    return info.value, np.tril(F)


def test_one_core_same_bits_for_every_caller(ctx):
    A = _spd(128)
    Lref = np.linalg.cholesky(A)
    bound = 1e-12 * np.abs(Lref).max()
    i2, L2 = _potrf(ctx, A, 2)  # the stand-alone launch
    i3, L3 = _potrf(ctx, A, 3)  # the persistent launch
    A256 = _spd(256)
    A256[:128, :128] = A
    i256, L256 = _potrf(ctx, A256, 3)
    assert (i2, i3, i256) == (0, 0, 0)
    for name, L in (("impl 2", L2), ("impl 3", L3), ("impl 3, leading block of order 256", L256[:128, :128])):
        err = np.abs(L - Lref).max()
        print("%s: max |L - L_lapack| %.3e (bound %.3e)" % (name, err, bound))
        assert err < bound, (name, err)
    assert np.array_equal(L2, L3)
    assert np.array_equal(L256[:128, :128], L3)


@pytest.mark.parametrize("p", [0, 15, 16, 127])  # first leaf, end of a leaf, start of the next, last column
def test_bad_pivot_keeps_its_index(ctx, p):
    B = _spd(128)
    B[p, p] = -1.0
    for impl in (2, 3):
        info, _ = _potrf(ctx, B, impl)
        assert info == p + 1, (impl, info)


@pytest.mark.parametrize("d", [64, 65, 128])  # the largest that takes block64; the smallest and the largest that take the full core
def test_gx_block_of_the_one_launch_fit(ctx, d):
    n, k = 2 * d + 1, 2
    specs = [_spec("cubic", 1, n, d, k, seed=1000 * n + 10 * d + p) for p in range(8)]
    refs = [single(ctx, s) for s in specs]
    assert all(rc == 0 for rc, _ in refs)
    for p, (s, (_, m)) in enumerate(zip(specs, refs)):
        assert m.info["fallbacks"] == 0, (p, m.info)
        ref = orc.fit(s["C"], s["Y"], s["kid"], s["a"], s["b"], s["deg"])
        ew = np.abs(m.weights - ref.w).max() / np.abs(ref.w).max()
        print("d %d start %d: rel_residual %.3e  weights against the oracle %.3e" % (d, p, m.info["rel_residual"], ew))
        # the bounds of tests/test_gpu_parity.py::test_medium_sizes_against_oracle
        assert m.info["rel_residual"] < 1e-10, (p, m.info)
        assert ew < 1e-10, (p, ew)
    got = batch(ctx, specs)
    for p, (g, r) in enumerate(zip(got, refs)):
        assert_same_model(g, r, (n, d, "cubic", k, len(got), p), well_conditioned=True)
    _free(got), _free(refs)
