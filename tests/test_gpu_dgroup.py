"""The D-precompute as one launch over a rank's blocks, the diagonal tiles inverted in it
(Route::dgroup and Route::dinv): with the emitted code spectra (Route::zemit) every
local block's spectra lie in `yz` before the precompute starts, so k_gram_chol_mf runs once
over all of them (blockIdx.y the block), and where the tile d-solve reads the factor the
kernel leaves L_jj^-1 in the diagonal tiles' slots itself, through the device helper that
k_invert_diag runs (diag_tile_invert, kernels.hpp), instead of a second kernel.

Every case runs the route on against CCSC_DGROUP=0 (one launch per block, k_invert_diag on
its side stream: the path before the route) in one process: fresh sessions, the same seeded
inputs, verbose "none", tol 0.  Both paths run the same arithmetic on the same values, so bit
equality is expected; the bound ONOFF is 100 times the largest relative difference measured
over the cases of this file, or 1e-12 where that was 0.  One case is also held
against the float64 oracle with the project's tolerances (objectives 1e-9, d / z / DZ 1e-7).

All shapes are 100 x 100 patches with psf 11 (the 110 x 110 grid of the register-line route),
the K x K Cholesky factor asked for as C1/C2 run it (blocks of so few patches would resolve to
the Woodbury factor).  The shapes are the smallest at which each piece can go wrong:
  K = 5                no tile d-solve, so grouping alone: the blockIdx.y offsets
  K = 65               Tn = 5, the last tile with one real row and 15 padding rows; 3 blocks
  K = 80, ni = 17      whole tiles only; a second staging chunk that holds one patch
  K = 100, ni = 16     the headline tile count (the panel on waves 0 and 1, then on wave 0
                       alone); an exact staging chunk
  K = 112              the largest tile d-solve shape; grid.y = 1
"""
import os

import numpy as np
import pytest

from oracle import ccsc_oracle as O

gpu = pytest.mark.gpu

# measured: the largest on/off difference over the cases below was 0 (every output equal bit
# for bit on MI355X), so the bound is the 1e-12 floor
ONOFF = 1e-12
# (two ranks against one rank, both with the route on, measured 0 as well: with shards of 2 + 1
# blocks the consensus sums run in the one-rank order, so that pair has the same bound)


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


def _problem(variant, b, K, ni, steps, trace=False, **kw):
    from ccsc_code_iccv2017_amd import learners as E
    return E.make_problem(E.L.CCSC_DPAR if variant == "dp" else E.L.CCSC_DZPAR, b.shape,
                          [11, 11, K], 1.0, 1.0, steps, 0.0, "none", ni=ni,
                          trace_objective=trace, dfactor="cholesky", **kw)


def _run(ctx, variant, inputs, K, ni, steps, on, *, trace=False, poke=False, **kw):
    """`steps` outer iterations on a fresh session with the route on or off; poke: the codes
    are read out between the steps (results() materialises the state, so the next precompute
    takes the per-block loop)."""
    from ccsc_code_iccv2017_amd import learners as E
    b, d0, z0 = inputs
    with _env(CCSC_DGROUP="1" if on else "0"):
        p = _problem(variant, b, K, ni, steps, trace, **kw)
        s = E.Session(ctx, p, b, d0, z0)
        try:
            for i in range(steps):
                if s.step(1):
                    break
                if poke and i + 1 < steps:
                    s.results(want_z=True, want_DZ=False)
            d, z, DZ, obj = s.results(want_z=True, want_DZ=True, want_obj=True)
            it = s.iterlog()
            plan = E.plan_bytes(s.p)
        finally:
            s.close()
    return {"d": d, "z": z, "DZ": DZ, "obj": obj, "it": it, "plan": plan}


def _worst(a, b, what):
    worst = 0.0
    for k in ("d", "z", "DZ"):
        r = _maxrel(a[k], b[k])
        print(f"dgroup {what} {k}: max rel diff {r:.3e}")
        worst = max(worst, r)
    r = abs(a["obj"] / b["obj"] - 1)
    print(f"dgroup {what} objective: rel diff {r:.3e}")
    return max(worst, r)


_k5 = {}


def _case5(ctx):
    """K = 5, ni = 3, 2 blocks, 3 steps, route on and off: shared with the oracle test."""
    if not _k5:
        inp = _inputs("dz", 5, 6, 3, seed=31)
        _k5["inp"] = inp
        _k5[True] = _run(ctx, "dz", inp, 5, 3, 3, True)
        _k5[False] = _run(ctx, "dz", inp, 5, 3, 3, False)
    return _k5


@gpu
def test_grouping_alone(gpu_ctx):
    """K = 5: the sweep d-solve reads the factor as it is, so only the grouped launch differs."""
    c = _case5(gpu_ctx)
    assert c[True]["plan"] == c[False]["plan"]
    assert _worst(c[True], c[False], "on/off K=5") <= ONOFF


@gpu
def test_against_the_oracle(gpu_ctx):
    """The K = 5 case against the float64 oracle.  (The oracle factors every bin by pinv: at
    the tile shapes, K > 64, its run takes half a minute and more, so those are held against
    the path before the route, which the parity tests hold against the oracle.)"""
    c = _case5(gpu_ctx)
    b, d0, z0 = c["inp"]
    d_o, z_o, DZ_o, it_o = O.learn_2d_dzparallel(b, [11, 11, 5], 1.0, 1.0, 3, 0.0, "brief",
                                                 {"d": d0, "z": z0}, ni=3)[:4]
    obj_o = np.asarray(it_o["obj_vals_z"])[3]
    for on in (True, False):
        r = c[on]
        for k, ref in (("d", d_o), ("z", z_o), ("DZ", DZ_o)):
            e = _rel(r[k], ref)
            print(f"dgroup oracle route {'on' if on else 'off'} {k}: {e:.3e}")
            assert e < 1e-7
        e = abs(r["obj"] / obj_o - 1)
        print(f"dgroup oracle route {'on' if on else 'off'} objective: {e:.3e}")
        assert e < 1e-9


@gpu
def test_padded_last_tile_three_blocks(gpu_ctx):
    inp = _inputs("dz", 65, 9, 3, seed=65)
    on = _run(gpu_ctx, "dz", inp, 65, 3, 3, True)
    off = _run(gpu_ctx, "dz", inp, 65, 3, 3, False)
    assert on["plan"] == off["plan"]
    assert _worst(on, off, "on/off K=65") <= ONOFF


@gpu
@pytest.mark.parametrize("variant,K,n,ni,steps,what", [
    ("dz", 80, 34, 17, 3, "whole tiles, second chunk of one patch"),
    ("dz", 100, 32, 16, 3, "headline tile count, exact chunk"),
    ("dp", 100, 32, 16, 3, "headline tile count, exact chunk"),
    ("dz", 112, 3, 3, 2, "largest tile d-solve shape, grid.y = 1"),
])
def test_tile_shapes(gpu_ctx, variant, K, n, ni, steps, what):
    inp = _inputs(variant, K, n, ni, seed=K + ni)
    on = _run(gpu_ctx, variant, inp, K, ni, steps, True)
    off = _run(gpu_ctx, variant, inp, K, ni, steps, False)
    assert on["plan"] == off["plan"]
    assert _worst(on, off, f"on/off {variant} K={K} ni={ni}") <= ONOFF


@gpu
def test_two_ranks_group_their_own_shards(gpu_ctx):
    """K = 100, ni = 3, 3 blocks: two ranks on one device (host transport, shards of 2 and 1
    blocks) launch over their own block counts."""
    from ccsc_code_iccv2017_amd import learners as E
    K, ni, n = 100, 3, 9
    b, d0, z0 = _inputs("dz", K, n, ni, seed=100)
    p = _problem("dz", b, K, ni, 3)

    def learn(ctx, on):
        with _env(CCSC_DGROUP="1" if on else "0"):
            d, z, DZ, it = E.learn_once(ctx, p, b, d0, z0, want_obj=True)
        return {"d": d, "z": z, "DZ": DZ, "obj": it["obj_val"]}

    one = learn(gpu_ctx, True)
    mctx = E.Context.multi([0, 0])
    try:
        two_on = learn(mctx, True)
        two_off = learn(mctx, False)
    finally:
        mctx.close()
    assert _worst(two_on, two_off, "on/off two ranks") <= ONOFF
    assert _worst(two_on, one, "two ranks / one rank") <= ONOFF


@gpu
def test_block_past_the_fused_lds_keeps_the_separate_inversion(gpu_ctx):
    """K = 65, ni = 545, 2 blocks, 2 steps: the block's w beside the three inversion tiles
    would pass 80 KB of LDS, so the kernel stays unfused (Route::dinv off) while the launch is
    still grouped, followed by one k_invert_diag over both blocks' bins.  Filters and codes start
    from the device RNG and the codes stay on the device (7 GB): d, DZ and the objective are
    compared."""
    from ccsc_code_iccv2017_amd import learners as E
    K, ni, n = 65, 545, 1090
    b = np.random.default_rng(545).standard_normal((100, 100, n))
    got = {}
    for on in (True, False):
        with _env(CCSC_DGROUP="1" if on else "0"):
            s = E.Session(gpu_ctx, _problem("dz", b, K, ni, 2, max_it_d=2, max_it_z=2, seed=7),
                          b)
            try:
                s.step(1)
                s.step(1)
                d, _, DZ, obj = s.results(want_z=False, want_DZ=True, want_obj=True)
            finally:
                s.close()
        got[on] = {"d": d, "DZ": DZ, "obj": obj}
    worst = max(_maxrel(got[True][k], got[False][k]) for k in ("d", "DZ"))
    worst = max(worst, abs(got[True]["obj"] / got[False]["obj"] - 1))
    print(f"dgroup on/off ni=545: max rel diff {worst:.3e}")
    assert np.isfinite(got[True]["obj"])
    assert worst <= ONOFF


@gpu
def test_results_between_steps_alternate_the_paths(gpu_ctx):
    """results() between the steps materialises the state: the next precompute takes the
    per-block loop (with the fused inversion), the others the grouped launch."""
    K, ni, n = 100, 3, 6
    inp = _inputs("dz", K, n, ni, seed=7)
    on = _run(gpu_ctx, "dz", inp, K, ni, 3, True, poke=True)
    off = _run(gpu_ctx, "dz", inp, K, ni, 3, False, poke=True)
    assert _worst(on, off, "on/off poked") <= ONOFF


@gpu
def test_objective_trace_keeps_the_block_loop(gpu_ctx):
    """trace_objective leaves the emitted-spectra route off, and the grouped launch with it:
    plan bytes and results equal with and without the switch."""
    K, ni, n = 100, 3, 6
    inp = _inputs("dz", K, n, ni, seed=7)
    on = _run(gpu_ctx, "dz", inp, K, ni, 2, True, trace=True)
    off = _run(gpu_ctx, "dz", inp, K, ni, 2, False, trace=True)
    assert on["plan"] == off["plan"]
    assert _worst(on, off, "on/off traced") <= ONOFF
    np.testing.assert_allclose(on["it"]["trace"]["obj_z"], off["it"]["trace"]["obj_z"],
                               rtol=ONOFF)


def test_plan_and_support_do_not_depend_on_the_switch():
    """ccsc_plan_bytes and ccsc_supported say the same with CCSC_DGROUP on and off: C2 and
    the shapes of this file, one and two ranks."""
    from ccsc_code_iccv2017_amd import _lib
    if not _lib.LIB_PATH.exists():
        from ccsc_code_iccv2017_amd import build
        build.build()
    from ccsc_code_iccv2017_amd import learners as E
    L = E.L
    shapes = [(100, 10000, 100), (5, 6, 3), (65, 9, 3), (80, 34, 17), (100, 32, 16), (112, 3, 3),
              (100, 4000, 2000)]
    for K, n, ni in shapes:
        for trace in (False, True):
            p = E.resolve(E.make_problem(L.CCSC_DZPAR, (100, 100, n), [11, 11, K], 1.0, 1.0, 3,
                                         0.0, "none", ni=ni, trace_objective=trace,
                                         dfactor="cholesky"))
            got = {}
            for v in ("1", "0"):
                with _env(CCSC_DGROUP=v):
                    eb = L.errbuf()
                    sup = L.lib().ccsc_supported(p, eb, len(eb))
                    nr = (1, 2) if n // ni >= 2 else (1,)
                    got[v] = (sup, eb.value, [E.plan_bytes(p, r, k) for k in nr for r in range(k)])
            assert got["1"] == got["0"], (K, n, ni, trace)
