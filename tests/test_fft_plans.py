"""CPU: every FFT plan the four transform families can run, through ccsc_test_fft_plan (host
only: the planners the sessions call, no GPU).

Per plan: the radices multiply to n, the pass count fits the kernels' slots, generic radices
are what each planner may feed the generic pass, every pass's work fits the capacity the
launched instantiation holds, the LDS budget holds, the twiddle tables tile their buffer and
the ragged last workgroups cover the grid.  The rejected lengths are pinned, and the grids
the GPU sweeps run (fft_cases.py) must reach every pass signature the planners produce
anywhere in the range swept here.  The last test validates the sweeps' reference (numpy.fft
in float64) against a direct DFT in extended precision.
"""
import math

import numpy as np
import pytest

import fft_cases as FC
from ccsc_code_iccv2017_amd import _lib as L

NMAX = 2048
KIB = 1024



def _plan(family, *dims):
    """The plan, or None when the planner rejects the geometry (any other error raises)."""
    from ccsc_code_iccv2017_amd.learners import fft_plan
    try:
        return fft_plan(family, *dims)
    except L.CCSCError as e:
        assert e.code == L.CCSC_E_UNSUPPORTED, e
        assert "plan" in str(e) or "LDS" in str(e) or "half spectrum" in str(e), e
        return None


@pytest.fixture(scope="module")
def lib():
    if not L.LIB_PATH.exists():
        from ccsc_code_iccv2017_amd import build
        build.build()
    return L.lib()


def _twiddle_sizes(d):
    sizes, Ns = [], 1
    for R in d["rad"]:
        sizes.append((R - 1) * Ns + (0 if R in FC.NATIVE else R))
        Ns *= R
    return sizes


def check_dir(family, d, what):
    """The per-direction assertions of one plan."""
    lds_family = family in FC.LDS_FAMILIES
    n, rad = d["n"], d["rad"]
    assert math.prod(rad) == n, what
    assert d["npass"] == len(rad) <= (3 if lds_family else 4), what
    assert d["threads"] == (1024 if lds_family else 256), what
    Ns = 1
    for s, R in enumerate(rad):
        nb, lines = n // R, d["lines"]
        if d["pfa"] and s == 1:
            # the prime-factor pass: (output group, k1, line) task slots padded to whole waves
            work = -(-((R - 1) // 2) // FC.QP) * 2 * (-(-lines // 64) * 64)
        elif R in FC.NATIVE:
            work = nb * lines
        else:
            assert R % 2 == 1 and R >= 3, what
            if lds_family:
                assert R >= 13 and FC.is_prime(R), what
            work = lines * nb * -(-((R - 1) // 2) // FC.QP)
        assert work <= d["cap"][s], (what, s, R, work, d["cap"][s])
        Ns *= R
    if d["pfa"]:
        assert n == 74 and rad == [2, 37] and lds_family, what
    assert d["lds_bytes"] <= (160 if lds_family else 40) * KIB, what
    assert not (lds_family and d["tw_global"]), what


def check_twiddles(dirs, what):
    """The passes' tables follow one another from 0 and fill the buffer (the two directions
    of a slice share one buffer; every line direction has its own)."""
    off = 0
    for d in dirs:
        for o, size in zip(d["twoff"], _twiddle_sizes(d)):
            assert o == off, what
            off += size
    for d in dirs:
        assert d["ntw"] == max(off, 1), what


def check_plan(family, dims, p):
    what = (FC.FAMILY_NAME[family], dims)
    for name in "xyt":
        if name in p:
            check_dir(family, p[name], what + (name,))
    if family == L.FFT_SLICE2D:
        X, Y = dims
        assert p["x"]["n"] == X and p["y"]["n"] == Y, what
        assert p["x"]["lines"] == (Y + 1) // 2 and p["y"]["lines"] == X // 2 + 1, what
        check_twiddles([p["x"], p["y"]], what)
    elif family == L.FFT_TTILE:
        Xh, _, Tn = dims
        assert p["t"]["n"] == Tn and p["t"]["lines"] == Xh, what
        check_twiddles([p["t"]], what)
    else:
        X, Y, T = dims if family == L.FFT_LINE3D else dims + (1,)
        Xh, rows = X // 2 + 1, Y * T
        x = p["x"]
        assert x["n"] == X and 1 <= x["lines"], what
        assert x["groups"] * 2 * x["lines"] >= rows > (x["groups"] - 1) * 2 * x["lines"], what
        check_twiddles([x], what)
        for name, n in (("y", Y), ("t", T))[: 2 if family == L.FFT_LINE3D else 1]:
            c = p[name]
            assert c["n"] == n and 1 <= c["lines"] <= min(32, Xh), what
            assert c["groups"] * c["lines"] >= Xh > (c["groups"] - 1) * c["lines"], what
            check_twiddles([c], what)
    if family in FC.LDS_FAMILIES:
        # the instantiation the launcher picks compiles every pass kind the plan needs
        for name in "xyt":
            if name in p:
                assert p[name]["mask"] & ~p["inst_mask"] == 0, what
    else:
        assert p["inst"] == "all", what


def _range_grids():
    """(family, dims) of every geometry the range sweeps plan."""
    g = []
    for n in range(1, NMAX + 1):
        g += [(L.FFT_SLICE2D, (n, 6)), (L.FFT_SLICE2D, (6, n))]
        g += [(L.FFT_LINE2D, (n, 6)), (L.FFT_LINE2D, (6, n))]
        g += [(L.FFT_LINE3D, (n, 6, 5)), (L.FFT_LINE3D, (6, n, 5)), (L.FFT_LINE3D, (6, 5, n))]
    for n in range(1, 113):
        g += [(L.FFT_SLICE2D, (n, n)), (L.FFT_SLICE2D, (n, 110)), (L.FFT_SLICE2D, (110, n))]
    for xh in FC.TTILE_XH:
        g += [(L.FFT_TTILE, (xh, 1, tn)) for tn in range(2, 257)]
    return g


def _gpu_grids():
    g = [(L.FFT_SLICE2D, d) for d in FC.slice_grids()]
    g += [(L.FFT_LINE2D, d) for d in FC.line2d_grids()]
    g += [(L.FFT_LINE3D, d) for d in FC.line3d_grids()]
    g += [(L.FFT_TTILE, (xh, 1, tn)) for tn, xh in FC.ttile_tiles()]
    return g


@pytest.fixture(scope="module")
def range_plans(lib):
    return {(f, d): _plan(f, *d) for f, d in _range_grids()}


@pytest.fixture(scope="module")
def gpu_plans(lib):
    return {(f, d): _plan(f, *d) for f, d in _gpu_grids()}


def test_every_plan_in_range_is_consistent(range_plans):
    planned = 0
    for (family, dims), p in range_plans.items():
        if p is not None:
            check_plan(family, dims, p)
            planned += 1
    assert planned > 0.5 * len(range_plans)


def test_every_gpu_sweep_plan_is_consistent(gpu_plans):
    for (family, dims), p in gpu_plans.items():
        if p is not None:
            check_plan(family, dims, p)


def test_line_families_reject_no_length(range_plans):
    """The global line passes are the fallback of every learner and the solvers' only
    transform: every length 2..2048 plans, in every direction."""
    rejected = [(FC.FAMILY_NAME[f], d) for (f, d), p in range_plans.items()
                if f in (L.FFT_LINE2D, L.FFT_LINE3D) and p is None]
    assert rejected == []


def test_long_lines_keep_their_twiddles_in_global_memory(range_plans):
    """A line too long for its rows / columns and its twiddle table in one 40 KiB workgroup
    (the 2047-entry table of 2048 = 8 8 8 4, the roots of a one-pass generic plan past about 850)
    reads the table from global memory; every shorter line stages it into LDS as before."""
    for X, want in ((840, False), (847, False), (1024, False), (857, True), (1021, True),
                    (2042, True), (2048, True)):
        assert range_plans[(L.FFT_LINE2D, (X, 6))]["x"]["tw_global"] is want, X
        assert range_plans[(L.FFT_LINE2D, (6, X))]["y"]["tw_global"] is want, X
    for (f, d), p in range_plans.items():
        if f in (L.FFT_LINE2D, L.FFT_LINE3D) and max(d) <= 848:
            assert not any(p[k]["tw_global"] for k in "xyt" if k in p), d


def test_slice_rejections_are_pinned(range_plans, lib):
    rejected = tuple(n for n in range(1, 113) if range_plans[(L.FFT_SLICE2D, (n, n))] is None)
    assert rejected == FC.SLICE_REJECTED == (54, 81, 108)
    # the other extent only sets the line count: the same lengths fall out next to 110 lines
    for n in range(1, 113):
        for dims in ((n, 110), (110, n)):
            assert (range_plans[(L.FFT_SLICE2D, dims)] is None) == (n in rejected), dims
    # the fallback: a dParallel problem on each rejected grid is still supported
    import ctypes as C
    from ccsc_code_iccv2017_amd.learners import make_problem
    eb = L.errbuf()
    for n in rejected:
        p = make_problem(L.CCSC_DPAR, (n - 2, n - 2, 4), [3, 3, 3], 1.0, 1.0, 2, 0.0, "none", ni=2)
        assert lib.ccsc_supported(C.byref(p), eb, len(eb)) == 0, (n, eb.value)


def test_ttile_rejections_start_where_the_slices_do(range_plans):
    """The t tile shares plan1d with the slices: its first rejected length is 54 at every
    line count (the 3D end-to-end fallback case of test_gpu_parity.py uses it)."""
    for xh in FC.TTILE_XH:
        rej = [tn for tn in range(2, 129) if range_plans[(L.FFT_TTILE, (xh, 1, tn))] is None]
        assert rej == [54, 81, 108, 126][: len(rej)] and rej[0] == 54, (xh, rej)


def test_pinned_instantiations(gpu_plans):
    assert gpu_plans[(L.FFT_TTILE, (38, 1, 42))]["inst"] == "fixed38"
    for tn in (6, 9, 14, 18, 21, 42, 63):
        assert gpu_plans[(L.FFT_TTILE, (33, 1, tn))]["inst"] == "rm42", tn
    assert gpu_plans[(L.FFT_SLICE2D, (74, 74))]["inst"] == "rm74"
    assert gpu_plans[(L.FFT_SLICE2D, (74, 74))]["x"]["pfa"]
    assert gpu_plans[(L.FFT_SLICE2D, (110, 110))]["x"]["rad"] == [11, 10]


def test_gpu_sweep_reaches_every_signature(range_plans, gpu_plans):
    """The audit: every (family, direction, slot, radix kind, Ns > 1) pass signature, every
    prime-factor pass, four-slot plan and kernel instantiation that ANY geometry of the range
    produces is run by at least one grid of the GPU sweeps."""
    def sigs(plans):
        out = {}
        for (f, d), p in plans.items():
            if p is not None:
                for s in FC.signatures(f, p):
                    out.setdefault(s, d)
        return out
    everything, swept = sigs(range_plans), sigs(gpu_plans)
    missing = {s: d for s, d in everything.items() if s not in swept}
    assert not missing, f"signatures no GPU sweep grid reaches (and a grid that has each): {missing}"
    # what the sweeps are there for, by name
    for s in [("slice2d", "x", "pfa"), ("slice2d", "y", "pfa"), ("ttile", "t", "pfa"),
              ("slice2d", "inst", "rm74"), ("ttile", "inst", "rm42"), ("ttile", "inst", "fixed38"),
              ("ttile", "inst", "all"), ("line2d", "x", "four slots"), ("line2d", "y", "four slots"),
              ("line3d", "t", "four slots"), ("slice2d", "x", 1, 4, True),
              ("slice2d", "y", 2, "generic prime", True), ("line2d", "x", 0, "generic composite", False),
              ("line2d", "y", 1, "generic composite", True)]:
        assert s in swept, s


@pytest.mark.parametrize("family,dims", [
    (L.FFT_SLICE2D, (0, 4)), (L.FFT_TTILE, (4, 1, 0)), (L.FFT_LINE2D, (4, -1)),
    (L.FFT_LINE3D, (4, 4, 0)), (7, (4, 4, 4))])
def test_plan_hook_validates(lib, family, dims):
    from ccsc_code_iccv2017_amd.learners import fft_plan
    with pytest.raises(L.CCSCError) as e:
        fft_plan(family, *dims)
    assert e.value.code == L.CCSC_E_INVALID


def test_numpy_reference_against_extended_precision_dft():
    """The GPU sweeps compare with numpy.fft in float64.  Its own error against a direct DFT
    in np.longdouble (roots exp(-2 pi i (j k mod n) / n) from an n-entry table, so no argument
    grows with j k) stays under 1e-14 relative max-abs at every length, a tenth of the
    sweeps' bar of 1e-13."""
    ld = np.longdouble
    two_pi = 8 * np.arctan(ld(1))
    rng = np.random.default_rng(7)
    worst = 0.0
    for n in list(range(2, 257)) + [509, 512, 1021, 1024]:
        x = rng.standard_normal((2, n)) + 1j * rng.standard_normal((2, n))
        ang = two_pi * np.arange(n, dtype=ld) / ld(n)
        wr, wi = np.cos(ang), -np.sin(ang)
        jk = np.outer(np.arange(n), np.arange(n)) % n
        xr, xi = x.real.astype(ld), x.imag.astype(ld)
        Wr, Wi = wr[jk], wi[jk]
        dr = xr @ Wr - xi @ Wi
        di = xr @ Wi + xi @ Wr
        got = np.fft.fft(x, axis=1)
        err = max(np.abs(got.real - dr).max(), np.abs(got.imag - di).max())
        rel = float(err / np.sqrt(dr * dr + di * di).max())
        worst = max(worst, rel)
        assert rel < 1e-14, (n, rel)
    print(f"numpy.fft worst relative max-abs error vs the extended-precision DFT: {worst:.2e}")
