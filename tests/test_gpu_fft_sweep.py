"""GPU: every FFT plan of the four transform families against numpy.fft in float64.

Input: seeded standard normal, 3 slices per call (so the slice stride is exercised).
Reference: numpy.fft over the same axes; test_fft_plans.py bounds its own error against an
extended-precision direct DFT by 1e-14.  Metric and bars are the suite's own
(test_fft2d_r2c_c2r): max|hs - ref| / max|ref| < 1e-13 for the spectra, max|rt - a| < 1e-12
for the round trip.  A plan whose largest generic radix R exceeds 128 gets both bars times
R / 128: a direct R-term sum has a worst-case error linear in R.

The grids are fft_cases.py's; test_fft_plans.py audits that they reach every pass signature
the planners produce.  Each test prints the worst ratio of a measured error to its bar.

Worst measured ratio to the bar per family (MI355X; spectrum, round trip):
  slice family      0.009 at 103 x 103        0.003 at 103 x 103
  line family, 2D   0.008 at 6 x 1000         0.003 at 6 x 1152
  line family, 3D   0.008 at 6 x 5 x 89       0.003 at 6 x 5 x 1664
  t-tile family     0.007 at Tn 113, Xh 33    0.003 at Tn 113, Xh 33
No length was over a bar.  The plans with a generic radix above 128 (up to 2039 in one
pass) stayed under 0.01 of their scaled bar as well.
"""
import numpy as np
import pytest

import fft_cases as FC
from ccsc_code_iccv2017_amd import _lib as L

pytestmark = pytest.mark.gpu

COUNT = 3
SPEC_BAR = 1e-13
RT_BAR = 1e-12


def _plan(family, *dims):
    from ccsc_code_iccv2017_amd.learners import fft_plan
    try:
        return fft_plan(family, *dims)
    except L.CCSCError as e:
        assert e.code == L.CCSC_E_UNSUPPORTED, e
        return None


def _bar_scale(plan):
    R = max([r for k in "xyt" if k in plan for r in plan[k]["rad"] if r not in FC.NATIVE],
            default=0)
    return max(1.0, R / 128.0)


class Worst:
    """Collects error / bar ratios of one sweep; fails with every grid over its bar."""

    def __init__(self, name):
        self.name, self.spec, self.rt, self.over = name, (0.0, None), (0.0, None), []

    def add(self, grid, spec_err, rt_err, scale):
        rs, rr = spec_err / (SPEC_BAR * scale), rt_err / (RT_BAR * scale)
        if self.spec[1] is None or rs > self.spec[0]:
            self.spec = (rs, grid)
        if self.rt[1] is None or rr > self.rt[0]:
            self.rt = (rr, grid)
        if not (rs < 1.0 and rr < 1.0):     # (a NaN fails too)
            self.over.append((grid, spec_err, rt_err, scale))

    def finish(self):
        print(f"\n{self.name}: worst spectrum error / bar {self.spec[0]:.3f} at {self.spec[1]}, "
              f"worst round-trip error / bar {self.rt[0]:.3f} at {self.rt[1]}")
        assert not self.over, f"{self.name}: (grid, spectrum error, round-trip error, bar scale) {self.over}"


def _rng(*dims):
    seed = 0
    for d in dims:
        seed = seed * 4099 + d
    return np.random.default_rng(seed)


def _run_real(ctx, hook, family, dims, w):
    """One grid of a real-input family (slices / lines): spectra and round trip."""
    p = _plan(family, *dims)
    assert p is not None, dims
    a = _rng(*dims).standard_normal(dims + (COUNT,))
    hs, rt = hook(ctx, a)
    axes = tuple(range(len(dims)))
    ref = np.fft.fftn(a, axes=axes)[: dims[0] // 2 + 1]
    assert hs.shape == ref.shape and rt.shape == a.shape
    w.add(dims, np.abs(hs - ref).max() / np.abs(ref).max(), np.abs(rt - a).max(), _bar_scale(p))


SLICE_CHUNKS = {
    "square": [(n, n) for n in FC.SLICE_N],
    "n_by_110": [(n, 110) for n in FC.SLICE_N],
    "110_by_n": [(110, n) for n in FC.SLICE_N],
    "n_by_5": [(n, 5) for n in FC.SLICE_N],
    "5_by_n": [(5, n) for n in FC.SLICE_N],
    "audit": list(FC.SLICE_AUDIT),
}


def test_slice_chunks_are_the_sweep():
    assert sorted(set(g for c in SLICE_CHUNKS.values() for g in c)) == sorted(set(FC.slice_grids()))


@pytest.mark.parametrize("chunk", list(SLICE_CHUNKS))
def test_slice_family(gpu_ctx, chunk):
    """LDS slice R2C / C2R (ccsc_test_fft2d).  The planner's rejections are exactly the
    grids with an extent pinned in fft_cases.SLICE_REJECTED, and the hook launches nothing
    on them."""
    from ccsc_code_iccv2017_amd.learners import fft2d_test
    w = Worst(f"slice family, {chunk}")
    for X, Y in SLICE_CHUNKS[chunk]:
        if X in FC.SLICE_REJECTED or Y in FC.SLICE_REJECTED:
            assert _plan(L.FFT_SLICE2D, X, Y) is None, (X, Y)
            with pytest.raises(L.CCSCError) as e:
                fft2d_test(gpu_ctx, np.zeros((X, Y, 1)))
            assert e.value.code == L.CCSC_E_UNSUPPORTED
            continue
        _run_real(gpu_ctx, fft2d_test, L.FFT_SLICE2D, (X, Y), w)
    w.finish()


def _line2d_chunks():
    g = FC.line2d_grids()
    rows = [d for d in g if d[1] == 5]
    cols = [d for d in g if d[0] == 6 and d[1] != 5]
    rest = [d for d in g if d not in rows and d not in cols]
    return {"rows_n_by_5": rows, "cols_6_by_n": cols, "tiles_and_audit": rest}


LINE2D_CHUNKS = _line2d_chunks()


@pytest.mark.parametrize("chunk", list(LINE2D_CHUNKS))
def test_line_family_2d(gpu_ctx, chunk):
    """Global row and column line passes planned by plan_lines (ccsc_test_gfft, T = 1)."""
    from ccsc_code_iccv2017_amd.learners import gfft_test
    w = Worst(f"line family 2D, {chunk}")
    for dims in LINE2D_CHUNKS[chunk]:
        _run_real(gpu_ctx, gfft_test, L.FFT_LINE2D, dims, w)
    w.finish()


LINE3D_CHUNKS = {"t_lines": [d for d in FC.line3d_grids() if d[:2] == (6, 5)],
                 "volumes_and_audit": [d for d in FC.line3d_grids() if d[:2] != (6, 5)]}


@pytest.mark.parametrize("chunk", list(LINE3D_CHUNKS))
def test_line_family_3d(gpu_ctx, chunk):
    """The same kernels planned with t-lines: rows over the Y T rows of a slice, y lines per
    plane, t lines over the Y rows."""
    from ccsc_code_iccv2017_amd.learners import gfft_test
    w = Worst(f"line family 3D, {chunk}")
    for dims in LINE3D_CHUNKS[chunk]:
        _run_real(gpu_ctx, gfft_test, L.FFT_LINE3D, dims, w)
    w.finish()


@pytest.mark.parametrize("Xh", FC.TTILE_XH)
def test_ttile_family(gpu_ctx, Xh):
    """The 3D learner's t-tile transform (ccsc_test_tfft): forward against numpy along t,
    then its unnormalised inverse (round trip / Tn against the input)."""
    from ccsc_code_iccv2017_amd.learners import tfft_test
    w = Worst(f"t-tile family, Xh = {Xh}")
    insts = {}
    for Tn, xh in FC.ttile_tiles():
        if xh != Xh:
            continue
        p = _plan(L.FFT_TTILE, Xh, 1, Tn)
        if p is None:   # (pinned by test_fft_plans.py: 54, 81, 108, 126)
            assert Tn in FC.SLICE_REJECTED or Tn == 126, Tn
            with pytest.raises(L.CCSCError) as e:
                tfft_test(gpu_ctx, np.zeros((Xh, 1, Tn, 1), dtype=complex))
            assert e.value.code == L.CCSC_E_UNSUPPORTED
            continue
        insts[Tn] = p["inst"]
        rng = _rng(Tn, Xh)
        shape = (Xh, FC.TTILE_YN, Tn, COUNT)
        a = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
        out, rt = tfft_test(gpu_ctx, a)
        ref = np.fft.fft(a, axis=2)
        w.add((Tn, Xh), np.abs(out - ref).max() / np.abs(ref).max(), np.abs(rt / Tn - a).max(),
              _bar_scale(p))
    if Xh == 38:
        assert insts[42] == "fixed38"
    if Xh == 33:
        assert [insts[t] for t in (6, 9, 14, 18, 21, 42, 63)] == ["rm42"] * 7
    assert "all" in insts.values()
    w.finish()


def test_hooks_validate_before_launch(gpu_ctx):
    from ccsc_code_iccv2017_amd.learners import gfft_test, tfft_test
    lib, eb = L.lib(), L.errbuf()
    a = np.zeros(8)
    for call in (lambda: lib.ccsc_test_gfft(gpu_ctx.ptr, 0, 4, 1, 1, L.dptr(a), None, None, eb, len(eb)),
                 lambda: lib.ccsc_test_gfft(gpu_ctx.ptr, 4, 2, 1, 0, L.dptr(a), None, None, eb, len(eb)),
                 lambda: lib.ccsc_test_gfft(None, 4, 2, 1, 1, L.dptr(a), None, None, eb, len(eb)),
                 lambda: lib.ccsc_test_tfft(gpu_ctx.ptr, 2, 2, 0, 1, L.dptr(a), None, None, eb, len(eb)),
                 lambda: lib.ccsc_test_tfft(gpu_ctx.ptr, 2, 2, 1, 1, None, None, None, eb, len(eb))):
        assert call() == L.CCSC_E_INVALID
    # outputs are optional
    hs, rt = gfft_test(gpu_ctx, np.ones((4, 2, 1)))
    assert abs(hs[0, 0, 0] - 8.0) < 1e-12 and np.abs(rt - 1.0).max() < 1e-12
    out, rt = tfft_test(gpu_ctx, np.ones((2, 1, 2, 1), dtype=complex))
    assert np.abs(out[:, 0, 0, 0] - 2.0).max() < 1e-12 and np.abs(rt - 2.0).max() < 1e-12
