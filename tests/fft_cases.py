"""Shared by test_fft_plans.py (CPU) and test_gpu_fft_sweep.py (GPU): the grids the GPU
sweeps run per transform family, and the pass signatures of a plan.  The CPU module audits
that these grids reach every signature the planners produce anywhere in their tested range,
so a planner change cannot silently shrink what the GPU sweeps cover."""
from ccsc_code_iccv2017_amd import _lib as L

NATIVE = (11, 10, 8, 7, 5, 4, 3, 2)
QP = 3                      # conjugate output pairs per generic-pass task
LDS_FAMILIES = (L.FFT_SLICE2D, L.FFT_TTILE)
FAMILY_NAME = {L.FFT_SLICE2D: "slice2d", L.FFT_TTILE: "ttile", L.FFT_LINE2D: "line2d",
               L.FFT_LINE3D: "line3d"}

# lengths n <= 112 the slice planner rejects (no native plan of <= 3 passes: 54 = 2 3^3,
# 81 = 3^4, 108 = 2^2 3^3, and a generic pass takes primes >= 13 only); the learners run such
# grids on the global line passes.  Pinned by test_fft_plans.py.
SLICE_REJECTED = (54, 81, 108)

# ---- grids of the GPU sweeps --------------------------------------------------------------
SLICE_N = range(2, 113)


# The *_AUDIT grids are not in the issue's ranges: each is the smallest grid found for a pass
# signature that only longer lines produce (test_fft_plans.py's coverage audit names the
# signature when one goes missing): radix 11 in slot 1 (121), 4, 5, 7, 8, 10, 11 in slot 2
# (484 = 11 11 4, 125, 343, 512, 1000, 1331).
SLICE_AUDIT = ((125, 6), (343, 6), (484, 6), (512, 6), (1000, 6), (1331, 6),
               (6, 125), (6, 343), (6, 484), (6, 512))


def slice_grids():
    """(X, Y): squares, the 110-line neighbours (the other extent sets the line count and
    hence the plan), and odd Y = 5 (Yp padding) / odd X = 5."""
    g = []
    for n in SLICE_N:
        g += [(n, n), (n, 110), (110, n), (n, 5), (5, n)]
    return sorted(set(g)) + list(SLICE_AUDIT)


LINE2D_EXTRA = (509, 512, 1000, 1021, 1024, 2042, 2048)
# radix 7 in slot 2 (448 = 8 8 7), 3 and a generic composite in slot 3 (768 = 8 8 4 3,
# 1152 = 8 4 4 9), a generic prime in slot 3 (1664 = 8 4 4 13)
LINE2D_AUDIT = ((448, 6), (768, 6), (1152, 6), (1664, 6), (6, 448), (6, 768), (6, 1152), (6, 1664))


def line2d_grids():
    """(X, Y): Y = 5 leaves an unpaired last row and ragged row groups; the long lengths give
    four-slot plans, large primes and L = 1; the last two full column tiles with a ragged
    xtiles."""
    g = []
    for n in list(range(2, 301)) + list(LINE2D_EXTRA):
        g += [(n, 5), (6, n)]
    return g + [(266, 266), (70, 67)] + list(LINE2D_AUDIT)


# the same kernels planned with t-lines (rows over Y T rows, the t lines): one grid per
# signature of the x, y and t directions that (6, 5, n) with n <= 130 does not produce
LINE3D_AUDIT = (
    (5, 6, 5), (7, 6, 5), (13, 6, 5), (18, 6, 5), (26, 6, 5), (50, 6, 5), (112, 6, 5), (144, 6, 5),
    (160, 6, 5), (208, 6, 5), (384, 6, 5), (768, 6, 5), (800, 6, 5), (1152, 6, 5), (1664, 6, 5),
    (1792, 6, 5),
    (6, 9, 5), (6, 13, 5), (6, 18, 5), (6, 26, 5), (6, 48, 5), (6, 50, 5), (6, 144, 5), (6, 224, 5),
    (6, 384, 5), (6, 768, 5), (6, 800, 5), (6, 1152, 5), (6, 1264, 5), (6, 1664, 5), (6, 1792, 5),
    (6, 5, 144), (6, 5, 208), (6, 5, 384), (6, 5, 512), (6, 5, 768), (6, 5, 1152), (6, 5, 1664), (6, 5, 1792))


def line3d_grids():
    """(X, Y, T)"""
    return ([(6, 5, n) for n in range(2, 131)] + [(12, 11, 10), (22, 20, 10), (9, 7, 5)] +
            list(LINE3D_AUDIT))


TTILE_XH = (4, 33, 38)
TTILE_YN = 3


def ttile_tiles():
    """(Tn, Xh)"""
    return [(tn, xh) for xh in TTILE_XH for tn in range(2, 129)] + [(196, 4)]   # 7 7 4: 4 in slot 2


# ---- pass signatures ------------------------------------------------------------------------
def is_prime(p):
    return p >= 2 and all(p % d for d in range(2, int(p ** 0.5) + 1))


def pass_kind(R):
    if R in NATIVE:
        return R
    return "generic prime" if is_prime(R) else "generic composite"


def signatures(family, plan):
    """Pass signatures of one plan (learners.fft_plan): (family, direction, slot, radix or
    generic kind, Ns > 1) per pass, the prime-factor pass, four-slot plans and the
    instantiation."""
    fam = FAMILY_NAME[family]
    sig = set()
    for dname in "xyt":
        d = plan.get(dname)
        if d is None:
            continue
        Ns = 1
        for s, R in enumerate(d["rad"]):
            if d["pfa"] and s == 1:
                sig.add((fam, dname, "pfa"))
            else:
                sig.add((fam, dname, s, pass_kind(R), Ns > 1))
            Ns *= R
        if d["npass"] == 4:
            sig.add((fam, dname, "four slots"))
    if family in LDS_FAMILIES:
        sig.add((fam, "inst", plan["inst"]))
    return sig
