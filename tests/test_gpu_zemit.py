"""The D-precompute's code spectra formed in the last z-iteration (Route::zemit):
with the register-line z-step, tol = 0 and the MFMA factor, the last z-launch of a phase
stores the spectra it forms into the idle `yz` buffer and k_gram_chol_mf reads them, adding
the term of w as it stages its rows, instead of a k_zhat_line pass into Zh.

Every case runs the route on against the route off (CCSC_ZEMIT=0) in one process: fresh
sessions, the same inputs.  Both paths run the same arithmetic on the same values, so the
results are expected to be equal or to differ in the last bits; the bound ONOFF is 100 times
the largest relative difference measured over the cases of this file, or 1e-12
where that was 0.  The basic case is also held against the float64 oracle with the
project's tolerances (objectives 1e-9, d / z / DZ 1e-7), the route-on error being no more
than twice the route-off error.

All shapes are 100 x 100 patches with psf 11: the 110 x 110 grid is the only one the
register-line route serves.  Sessions run with verbose "none" and no objective trace unless
a case says otherwise: an objective evaluation materialises the state, which takes the
fallback.
"""
import os

import numpy as np
import pytest

from oracle import ccsc_oracle as O

gpu = pytest.mark.gpu

# measured: the largest on/off difference over the cases below was 0 (every output equal
# bit for bit on MI355X), so the bound is the 1e-12 floor
ONOFF = 1e-12


def _maxrel(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


def _rel(a, b):
    a = np.asarray(a)
    b = np.asarray(b)
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300)


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _inputs(variant, K, n, ni, seed):
    rng = np.random.default_rng(seed)
    b = rng.standard_normal((100, 100, n))
    d0 = rng.standard_normal((11, 11, K))
    z0 = rng.standard_normal((110, 110, K, ni if variant == "dz" else n))
    return b, d0, z0


def _run(ctx, variant, inputs, K, ni, steps, zemit, *, tol=0.0, trace=False, poke=False,
         zsplit2=None, **kw):
    """`steps` outer iterations on a fresh session with the route on or off; poke: the
    codes are read out between the steps (results() materialises the state)."""
    from ccsc_code_iccv2017_amd import learners as E
    b, d0, z0 = inputs
    env = {"CCSC_ZEMIT": "1" if zemit else "0"}
    if zsplit2 is not None:
        env["CCSC_ZSPLIT2"] = zsplit2
    with _env(**env):
        p = E.make_problem(E.L.CCSC_DPAR if variant == "dp" else E.L.CCSC_DZPAR, b.shape,
                           [11, 11, K], 1.0, 1.0, steps, tol, "none", ni=ni,
                           trace_objective=trace, **kw)
        s = E.Session(ctx, p, b, d0, z0)
        try:
            for i in range(steps):
                done = s.step(1)
                if done:
                    break
                if poke and i + 1 < steps:
                    s.results(want_z=True, want_DZ=False)
            d, z, DZ, obj = s.results(want_z=True, want_DZ=True, want_obj=True)
            it = s.iterlog()
            plan = E.plan_bytes(s.p)
        finally:
            s.close()
    return {"d": d, "z": z, "DZ": DZ, "obj": obj, "it": it, "plan": plan}


def _onoff(on, off, what):
    worst = 0.0
    for k in ("d", "z", "DZ"):
        r = _maxrel(on[k], off[k])
        print(f"zemit on/off {what} {k}: max rel diff {r:.3e}")
        worst = max(worst, r)
    return worst


def _assert_same_bits(a, b):
    for k in ("d", "z", "DZ"):
        assert np.array_equal(a[k], b[k]), k
    assert a["obj"] == b["obj"]


_basic_cache = {}


def _basic(ctx, variant):
    """Case 1, shared by the tests that use it: K = 5, n = 6, ni = 3 (2 blocks), runs of 1, 2
    and 3 outer iterations with the route on and off (the final objective of the run of m
    iterations is the trace's entry m), and the oracle's run of 3."""
    if variant not in _basic_cache:
        K, n, ni = 5, 6, 3
        inp = _inputs(variant, K, n, ni, seed=31)
        runs = {(m, on): _run(ctx, variant, inp, K, ni, m, on) for m in (1, 2, 3) for on in (True, False)}
        learn = O.learn_2d_dparallel if variant == "dp" else O.learn_2d_dzparallel
        b, d0, z0 = inp
        orc = learn(b, [11, 11, K], 1.0, 1.0, 3, 0.0, "brief", {"d": d0, "z": z0}, ni=ni)
        _basic_cache[variant] = (inp, runs, orc)
    return _basic_cache[variant]


@gpu
@pytest.mark.parametrize("variant", ["dz", "dp"])
def test_basic_on_off_and_oracle(gpu_ctx, variant):
    _, runs, orc = _basic(gpu_ctx, variant)
    on, off = runs[(3, True)], runs[(3, False)]
    assert on["plan"] > off["plan"]   # the route is on: `yz` holds F complex per slice
    assert _onoff(on, off, f"basic {variant}") <= ONOFF
    tr_on = np.array([runs[(m, True)]["obj"] for m in (1, 2, 3)])
    tr_off = np.array([runs[(m, False)]["obj"] for m in (1, 2, 3)])
    print(f"zemit on/off basic {variant} objective trace: {np.abs(tr_on / tr_off - 1).max():.3e}")
    np.testing.assert_allclose(tr_on, tr_off, rtol=ONOFF)
    d_o, z_o, DZ_o, it_o = orc[:4]
    tr_o = np.asarray(it_o["obj_vals_z"])[1:4]
    np.testing.assert_allclose(tr_on, tr_o, rtol=1e-9)
    np.testing.assert_allclose(tr_off, tr_o, rtol=1e-9)
    for k, ref in (("d", d_o), ("z", z_o), ("DZ", DZ_o)):
        e_on, e_off = _rel(on[k], ref), _rel(off[k], ref)
        print(f"zemit oracle {variant} {k}: on {e_on:.3e} off {e_off:.3e}")
        assert e_on < 1e-7 and e_off < 1e-7
        assert e_on <= 2 * e_off
    e_on = np.abs(tr_on / tr_o - 1).max()
    e_off = np.abs(tr_off / tr_o - 1).max()
    assert e_on <= 2 * e_off or e_on == 0


@gpu
@pytest.mark.parametrize("K,n,ni,what", [
    (72, 8, 4, "tile d-solve shape: Tn = 5, padded rows of the last tile, K < 16 Tn staging"),
    (17, 4, 2, "odd K: one full tile plus one column"),
])
def test_filter_counts(gpu_ctx, K, n, ni, what):
    """(Blocks of so few patches resolve to the Woodbury factor, which keeps k_zhat_line:
    the K x K Cholesky factor is asked for, as C1/C2 run it.)"""
    inp = _inputs("dz", K, n, ni, seed=K)
    on = _run(gpu_ctx, "dz", inp, K, ni, 2, True, dfactor="cholesky")
    off = _run(gpu_ctx, "dz", inp, K, ni, 2, False, dfactor="cholesky")
    assert on["plan"] > off["plan"]
    assert _onoff(on, off, f"K={K}") <= ONOFF
    assert abs(on["obj"] / off["obj"] - 1) <= ONOFF


@gpu
def test_two_stream_phase_emits_both_halves(gpu_ctx):
    """n = 512 patches: every z-launch of a phase runs as two halves on two streams, each
    emitting at its own offset; the result equals the one-stream run bit for bit (as
    test_zline_two_stream_phase_is_exact) and the route-off run within ONOFF."""
    K, n, ni = 2, 512, 64
    inp = _inputs("dz", K, n, ni, seed=512)
    kw = dict(max_it_d=2, max_it_z=3)
    on = _run(gpu_ctx, "dz", inp, K, ni, 2, True, **kw)
    off = _run(gpu_ctx, "dz", inp, K, ni, 2, False, **kw)
    one = _run(gpu_ctx, "dz", inp, K, ni, 2, True, zsplit2="0", **kw)
    assert on["plan"] > off["plan"]
    assert _onoff(on, off, "two-stream") <= ONOFF
    _assert_same_bits(on, one)


@gpu
def test_invalidation_by_objective_trace(gpu_ctx):
    """trace_objective evaluates the objective after every z-iteration, which materialises
    the state over `yz`: the planner leaves the route off for such a run, nothing is emitted
    and every precompute takes the fallback."""
    inp, _, _ = _basic(gpu_ctx, "dz")
    on = _run(gpu_ctx, "dz", inp, 5, 3, 3, True, trace=True)
    off = _run(gpu_ctx, "dz", inp, 5, 3, 3, False, trace=True)
    assert on["plan"] == off["plan"]   # such a run never reads the spectra: `yz` stays as it was
    _assert_same_bits(on, off)
    assert np.array_equal(on["it"]["trace"]["obj_z"], off["it"]["trace"]["obj_z"])


@gpu
def test_invalidation_by_results_between_steps(gpu_ctx):
    """results(want_z=True) between two step(1) calls materialises the state after the last
    z-launch emitted: the next precompute must take the fallback, not read `yz`."""
    inp, _, _ = _basic(gpu_ctx, "dz")
    on = _run(gpu_ctx, "dz", inp, 5, 3, 3, True, poke=True)
    off = _run(gpu_ctx, "dz", inp, 5, 3, 3, False, poke=True)
    _assert_same_bits(on, off)


@gpu
def test_tol_run_is_the_unchanged_path(gpu_ctx):
    inp, _, _ = _basic(gpu_ctx, "dz")
    on = _run(gpu_ctx, "dz", inp, 5, 3, 3, True, tol=1e-3)
    off = _run(gpu_ctx, "dz", inp, 5, 3, 3, False, tol=1e-3)
    assert on["plan"] == off["plan"]
    _assert_same_bits(on, off)


def test_plan_grows_by_the_half_spectra_only():
    """C2 (2D dzParallel, K = 100, n = 10,000, 110 x 110 grid, tol = 0): with the route on
    `yz` holds np K F complex instead of np K P reals, nothing else changes, and the plan
    stays under the full-size test's 0.95 x 288 GB."""
    from ccsc_code_iccv2017_amd import _lib
    if not _lib.LIB_PATH.exists():
        from ccsc_code_iccv2017_amd import build
        build.build()
    from ccsc_code_iccv2017_amd import learners as E
    n, K, F, P = 10000, 100, 6160, 12100
    p = E.resolve(E.make_problem(E.L.CCSC_DZPAR, (100, 100, n), [11, 11, K], 1.0, 1.0, 20, 0.0,
                                 "none"))
    with _env(CCSC_ZEMIT="1"):
        on = E.plan_bytes(p)
    with _env(CCSC_ZEMIT="0"):
        off = E.plan_bytes(p)
    assert on - off == n * K * (F * 16 - P * 8)
    assert on < 0.95 * 288e9
    p.tol = 1e-3   # the route needs tol = 0
    with _env(CCSC_ZEMIT="1"):
        assert E.plan_bytes(p) == off
    # ... and a run that never evaluates the objective after a z-iteration (which would
    # materialise the state over the spectra before any precompute could read them)
    for kw in ({"verbose": "brief"}, {"trace_objective": True}):
        q = E.resolve(E.make_problem(E.L.CCSC_DZPAR, (100, 100, n), [11, 11, K], 1.0, 1.0, 20, 0.0,
                                     kw.get("verbose", "none"),
                                     trace_objective=kw.get("trace_objective", False)))
        with _env(CCSC_ZEMIT="1"):
            assert E.plan_bytes(q) == off
