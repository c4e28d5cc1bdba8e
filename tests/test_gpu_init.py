"""GPU: the engine's device-RNG initialisation, element by element.

A session created with d0 = z0 = NULL draws its codes from the counter stream of
``seed`` and its filters from the stream of ``seed ^ 0xd0d0d0d0`` (csrc/util.hip, k_randn).
``Session.results()`` before any step returns that initial z and crop(embed(d0)), so every
element of both draws is compared with the NumPy restatement tests/rng_ref.py: a wrong
offset, the wrong half of a Box-Muller pair or a layout mix-up moves values by O(1), the
bound is 1e-13.  (The sharded draws are in tests/test_gpu_multirank.py.)

The bound: |x| <= sqrt(2 * 53 * ln 2) = 8.57; the device's log, sqrt and sincospi and
NumPy's log, sqrt, sin, cos differ by a few ulp each, and the restatement's rounding of
the argument 2 pi u2 adds at most 2 pi 2^-53 * 8.57 = 6e-15.

Not covered: launch_randn's chunk boundary at 2^30 elements.  Observing it needs more
than 8.6 GB of draws copied to the host; by reading, `out + c0` and `offset + c0` advance
together.
"""
import numpy as np
import pytest

from rng_ref import FILTER_SEED_XOR, randn_ref

pytestmark = pytest.mark.gpu

ATOL = 1e-13
BIG_SEED = 0x123456789ABCDEF1   # all 64 bits of the seed reach the kernel


def _step0(ctx, p, b, smooth_init=None):
    from ccsc_code_iccv2017_amd import learners as E
    s = E.Session(ctx, p, b, d0=None, z0=None, smooth_init=smooth_init)
    try:
        d, z, _, _ = s.results(want_DZ=False)
    finally:
        s.close()
    return d, z


def _check(what, got, want):
    assert got.shape == want.shape
    dev = float(np.abs(got - want).max())
    print(f"{what}: max |engine - randn_ref| = {dev:.3e} over {got.size} draws")
    np.testing.assert_allclose(got, want, rtol=0, atol=ATOL)


def _draw(shape, seed, offset=0):
    return randn_ref(int(np.prod(shape)), seed, offset).reshape(shape, order="F")


@pytest.mark.parametrize("variant,sb,psf,K,n,ni,seed", [
    ("dp", (12, 11), 5, 3, 6, 2, 20171),
    ("dz", (12, 11), 5, 3, 6, 2, BIG_SEED),
    # the 110 x 110 grid, whose z-step keeps a state layout: results() must still hand
    # back the draw in output order
    ("dz", (100, 100), 11, 2, 4, 2, 20173),
])
def test_step0_2d_draws_equal_reference_stream(gpu_ctx, variant, sb, psf, K, n, ni, seed):
    """dP: z [X,Y,K,n] is the stream from element 0; dZ: the first block's ni K P draws,
    repeated for every block (dZ:44-47).  d_res [psf,psf,K] is the filters' stream.
    Measured on the MI355X: max |engine - randn_ref| 2.0e-15 (dP z), 2.1e-15 (dZ z),
    2.2e-15 (dZ z on the 110 grid, 96800 draws), 1.1e-15 (d)."""
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import learners as E
    r = psf // 2
    X, Y = sb[0] + 2 * r, sb[1] + 2 * r
    b = np.random.default_rng(1).standard_normal(sb + (n,))
    v = L.CCSC_DZPAR if variant == "dz" else L.CCSC_DPAR
    p = E.make_problem(v, b.shape, [psf, psf, K], 1.0, 1.0, 1, 0.0, "none", ni=ni, seed=seed)
    d, z = _step0(gpu_ctx, p, b)
    if variant == "dz":
        want = np.tile(_draw((X, Y, K, ni), seed), (1, 1, 1, n // ni))
    else:
        want = _draw((X, Y, K, n), seed)
    _check(f"{variant} z", z, want)
    _check(f"{variant} d", d, _draw((psf, psf, K), seed ^ FILTER_SEED_XOR))


def test_step0_3d_draws_equal_reference_stream(gpu_ctx):
    """3D learner on the 10 x 11 x 9 grid: z [X,Y,T,K,n], d_res [psf,psf,psf,K].
    Measured on the MI355X: max |engine - randn_ref| 2.0e-15 (z), 1.3e-15 (d)."""
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import learners as E
    sb, psf, K, n, seed = (8, 9, 7), 3, 3, 4, 20175
    g = tuple(s + 2 * (psf // 2) for s in sb)
    b = np.random.default_rng(2).standard_normal(sb + (n,))
    p = E.make_problem(L.CCSC_L3D, b.shape, [psf] * 3 + [K], 1.0, 0.1, 1, 0.0, "none", seed=seed)
    d, z = _step0(gpu_ctx, p, b)
    _check("L3 z", z, _draw(g + (K, n), seed))
    _check("L3 d", d, _draw((psf, psf, psf, K), seed ^ FILTER_SEED_XOR))


def test_step0_4d_draws_equal_reference_stream(gpu_ctx):
    """4D learner, 2 x 2 views: z [X,Y,1,1,K,n], d_res [psf,psf,U,V,K] (views inside K).
    Measured on the MI355X: max |engine - randn_ref| 1.7e-15 (z), 1.4e-15 (d)."""
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import learners as E
    sb, UV, psf, K, n, seed = (10, 9), 2, 5, 3, 4, 20177
    r = psf // 2
    b = np.random.default_rng(3).standard_normal(sb + (UV, UV, n))
    p = E.make_problem(L.CCSC_L4D, b.shape, [psf, psf, UV, UV, K], 1.0, 1.0, 1, 0.0, "none",
                       seed=seed)
    d, z = _step0(gpu_ctx, p, b)
    _check("L4 z", z, _draw((sb[0] + 2 * r, sb[1] + 2 * r, 1, 1, K, n), seed))
    _check("L4 d", d, _draw((psf, psf, UV, UV, K), seed ^ FILTER_SEED_XOR))


def test_step0_hs23_draws_equal_reference_stream(gpu_ctx):
    """2-3D learner, W = 3: z [X,Y,K,n]; the filters are ONE [psf,psf,K] draw replicated
    over the wavelengths (L23:54-56), d_res [psf,psf,W,K].
    Measured on the MI355X: max |engine - randn_ref| 1.7e-15 (z), 1.4e-15 (d)."""
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import learners as E
    sb, W, psf, K, n, seed = (12, 11), 3, 5, 4, 5, 20179
    r = psf // 2
    rng = np.random.default_rng(4)
    b = rng.random(sb + (W, n))
    sm = 0.5 * rng.random(sb + (W, n))
    p = E.make_problem(L.CCSC_HS23, b.shape, [psf, psf, W, K], 1.0, 0.2, 1, 0.0, "none", seed=seed)
    d, z = _step0(gpu_ctx, p, b, smooth_init=sm)
    _check("HS23 z", z, _draw((sb[0] + 2 * r, sb[1] + 2 * r, K, n), seed))
    d1 = _draw((psf, psf, K), seed ^ FILTER_SEED_XOR)
    assert d.shape == (psf, psf, W, K)
    for w in range(1, W):
        assert np.array_equal(d[:, :, w, :], d[:, :, 0, :])   # replicated, bit for bit
    _check("HS23 d", d, np.repeat(d1[:, :, None, :], W, axis=2))
