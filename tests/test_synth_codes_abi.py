"""CPU: ccsc_synthesize* / ccsc_densify* validate every argument before they touch a device
(a NULL context shows the reasons without a GPU), and the one place the synthesis kernel's
indices are computed (csrc/synth_codes.hpp, through ccsc_test_synth_index) agrees with Python
integers on grids whose row count reaches 2^31 - 2, on tiles that straddle the wrap of each
axis, and with ks = g."""
import ctypes as C
import itertools

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from ccsc_code_iccv2017_amd import _lib
    if not _lib.LIB_PATH.exists():
        from ccsc_code_iccv2017_amd import build
        build.build()
    return _lib


def _i3(v):
    return None if v is None else (C.c_int32 * 3)(*v)


GOOD = dict(d=True, ks=(3, 3, 1), C=1, K=2, g=(6, 5, 1), jc=True, ir=True, pr=True, n=2, nnz=4,
            out=True)


def _synth(L, entry, **kw):
    a = dict(GOOD, **kw)
    d = np.zeros(3 * 3 * 2)
    jc = np.array([0, 2, 4], dtype=np.int64)
    ir = np.zeros(4, dtype=np.int64)
    pr = np.zeros(4)
    out = np.zeros(6 * 5 * 2)
    eb = L.errbuf()
    fn = getattr(L.lib(), entry)
    if entry.endswith("_dev"):
        p = [x.ctypes.data if a[k] else None
             for k, x in (("d", d), ("jc", jc), ("ir", ir), ("pr", pr), ("out", out))]
    else:
        p = [L.dptr(d if a["d"] else None), L.lptr(jc if a["jc"] else None),
             L.lptr(ir if a["ir"] else None), L.dptr(pr if a["pr"] else None),
             L.dptr(out if a["out"] else None)]
    rc = fn(None, p[0], _i3(a["ks"]), a["C"], a["K"], _i3(a["g"]), p[1], p[2], p[3], a["n"],
            a["nnz"], p[4], eb, len(eb))
    return rc, eb.value.decode()


def _dens(L, entry, jc=True, ir=True, pr=True, M=8, n=2, nnz=4, out=True):
    a = dict(jc=jc, ir=ir, pr=pr, out=out)
    arr = dict(jc=np.array([0, 2, 4], dtype=np.int64), ir=np.zeros(4, dtype=np.int64),
               pr=np.zeros(4), out=np.zeros(16))
    eb = L.errbuf()
    fn = getattr(L.lib(), entry)
    if entry.endswith("_dev"):
        p = {k: (arr[k].ctypes.data if a[k] else None) for k in arr}
    else:
        p = {k: (L.dptr if k in ("pr", "out") else L.lptr)(arr[k] if a[k] else None) for k in arr}
    rc = fn(None, p["jc"], p["ir"], p["pr"], M, n, nnz, p["out"], eb, len(eb))
    return rc, eb.value.decode()


SYNTH = ["ccsc_synthesize", "ccsc_synthesize_dev"]
DENS = ["ccsc_densify", "ccsc_densify_dev"]


@pytest.mark.parametrize("entry", SYNTH)
@pytest.mark.parametrize("kw,word", [
    (dict(d=False), "d"), (dict(ks=None), "ks"), (dict(g=None), "g"), (dict(jc=False), "jc"),
    (dict(ir=False), "ir"), (dict(pr=False), "pr"), (dict(out=False), "out"),
    (dict(ks=(2, 3, 1)), "ks[0]"), (dict(ks=(3, 4, 1)), "ks[1]"), (dict(ks=(3, 3, 2)), "ks[2]"),
    (dict(ks=(0, 3, 1)), "ks[0]"), (dict(ks=(3, -1, 1)), "ks[1]"), (dict(ks=(3, 3, 0)), "ks[2]"),
    (dict(ks=(7, 3, 1)), "ks[0]"), (dict(ks=(3, 7, 1)), "ks[1]"), (dict(ks=(3, 3, 3)), "ks[2]"),
    (dict(g=(0, 5, 1)), "g[0]"), (dict(C=0), "C"), (dict(K=0), "K"), (dict(n=-1), "n"),
    (dict(nnz=-1), "nnz")])
def test_synthesize_rejections_are_invalid_and_name_the_argument(L, entry, kw, word):
    rc, msg = _synth(L, entry, **kw)
    assert rc == L.CCSC_E_INVALID and word in msg, (rc, msg)


@pytest.mark.parametrize("entry", SYNTH)
def test_synthesize_limits_are_unsupported_with_a_reason(L, entry):
    rc, msg = _synth(L, entry, g=(32768, 32768, 1), K=2)           # M = 2^31
    assert rc == L.CCSC_E_UNSUPPORTED and "2^31" in msg and "M" in msg, (rc, msg)
    rc, msg = _synth(L, entry, g=(1 << 30, 1 << 30, 1 << 30), K=1 << 30)
    assert rc == L.CCSC_E_UNSUPPORTED and "2^31" in msg, (rc, msg)
    # filters of more than 2^31 values: 1025 * 1025 taps, C = 2^11, K = 1
    rc, msg = _synth(L, entry, g=(1025, 1025, 1), ks=(1025, 1025, 1), C=1 << 11, K=1)
    assert rc == L.CCSC_E_UNSUPPORTED and "filters" in msg and " d " in msg, (rc, msg)


@pytest.mark.parametrize("entry", SYNTH)
def test_synthesize_valid_arguments_reach_the_context_check(L, entry):
    for kw in (dict(), dict(n=0, out=False), dict(nnz=0, ir=False, pr=False),
               dict(g=(32768, 32767, 1), K=2), dict(ks=(5, 5, 1), g=(5, 5, 1)),
               dict(ks=(1, 1, 1))):
        rc, msg = _synth(L, entry, **kw)
        assert rc == L.CCSC_E_INVALID and "ctx" in msg, (kw, rc, msg)


@pytest.mark.parametrize("entry", DENS)
@pytest.mark.parametrize("kw,word", [
    (dict(jc=False), "jc"), (dict(ir=False), "ir"), (dict(pr=False), "pr"),
    (dict(out=False), "out"), (dict(M=-1), "M"), (dict(n=-1), "n"), (dict(nnz=-1), "nnz")])
def test_densify_rejections_are_invalid_and_name_the_argument(L, entry, kw, word):
    rc, msg = _dens(L, entry, **kw)
    assert rc == L.CCSC_E_INVALID and word in msg, (rc, msg)


@pytest.mark.parametrize("entry", DENS)
def test_densify_limits_and_valid_arguments(L, entry):
    rc, msg = _dens(L, entry, M=1 << 31)
    assert rc == L.CCSC_E_UNSUPPORTED and "2^31" in msg, (rc, msg)
    for kw in (dict(), dict(n=0, out=False), dict(nnz=0, ir=False, pr=False),
               dict(M=(1 << 31) - 1)):
        rc, msg = _dens(L, entry, **kw)
        assert rc == L.CCSC_E_INVALID and "ctx" in msg, (kw, rc, msg)


# ---- the index arithmetic ----------------------------------------------------------------

def _index(L, g, ks, Cn, K, row, lo, ln, p, c, col):
    out = np.zeros(8, dtype=np.int64)
    eb = L.errbuf()
    L.check(L.lib().ccsc_test_synth_index(_i3(g), _i3(ks), Cn, K, row, _i3(lo), _i3(ln), _i3(p),
                                          c, col, L.lptr(out), eb, len(eb)), eb)
    return [int(v) for v in out]


def _want(g, ks, Cn, K, row, lo, ln, p, c, col):
    """The same eight numbers from Python integers and the definition."""
    X, Y, T = g
    e = (row % X, row // X % Y, row // (X * Y) % T, row // (X * Y * T))
    r = [s // 2 for s in ks]
    # in the window iff some output point of the tile has the entry inside its footprint
    hit = all(any((q - e[a] + r[a]) % g[a] < ks[a] for q in _axis_points(lo[a], ln[a], e[a],
                                                                       r[a], g[a]))
              for a in range(3))
    i = [(p[a] - e[a] + r[a]) % g[a] for a in range(3)]
    tap = -1
    if all(i[a] < ks[a] for a in range(3)):
        tap = i[0] + ks[0] * (i[1] + ks[1] * (i[2] + ks[2] * (c + Cn * e[3])))
    o = p[0] + X * (p[1] + Y * (p[2] + T * (c + Cn * col)))
    return [e[0], e[1], e[2], e[3], int(hit), tap, o, X * Y * T * K]


def _axis_points(lo, ln, e, r, g):
    """The tile's points along an axis; for a long tile only those that can matter (the ends
    and the points within r of the entry, circularly), so huge axes stay cheap."""
    if ln <= 64:
        return range(lo, lo + ln)
    near = {(e + s) % g for s in range(-r, r + 1)}
    return [q for q in near | {lo, lo + ln - 1} if lo <= q < lo + ln]


BIG = [
    # (g, ks, C, K): M = 2^31 - 65536 and 2^31 - 794648 (rows up to M - 1 < 2^31)
    ((32768, 32767, 1), (11, 11, 1), 3, 2),
    ((1290, 1290, 129), (5, 5, 5), 1, 10),
    ((32768, 32767, 1), (32767, 32767, 1), 1, 2),
]


@pytest.mark.parametrize("g,ks,Cn,K", BIG)
def test_index_arithmetic_is_exact_up_to_2_pow_31(L, g, ks, Cn, K):
    M = g[0] * g[1] * g[2] * K
    assert (1 << 31) - (1 << 24) < M < 1 << 31
    rows = [0, 1, g[0] - 1, g[0], g[0] * g[1] - 1, g[0] * g[1], M // 2 - 1, M // 2, M - g[0],
            M - 2, M - 1, (1 << 31) - 2 if (1 << 31) - 2 < M else M - 3]
    lo, ln = (g[0] - 16, 16, 0), (16, 16, 1)
    lo = (lo[0], lo[1], min(lo[2], g[2] - 1))
    for row in rows:
        for p in [(0, 0, 0), (g[0] - 1, g[1] - 1, g[2] - 1), (g[0] - 3, 17, g[2] // 2)]:
            a = (g, ks, Cn, K, row, lo, ln, p, Cn - 1, 999_999)
            assert _index(L, *a) == _want(*a), a
    # an output index far past 2^32
    a = (g, ks, Cn, K, M - 1, lo, ln, (g[0] - 1, g[1] - 1, g[2] - 1), Cn - 1, 3_000_000)
    got = _index(L, *a)
    assert got == _want(*a) and got[6] > 1 << 40


def test_rows_reach_2_pow_31_minus_2(L):
    g, ks, K = (65536, 16384, 1), (3, 3, 1), 2          # M = 2^31 is refused ...
    out = np.zeros(8, dtype=np.int64)
    eb = L.errbuf()
    rc = L.lib().ccsc_test_synth_index(_i3(g), _i3(ks), 1, K, 0, _i3((0, 0, 0)), _i3((1, 1, 1)),
                                       _i3((0, 0, 0)), 0, 0, L.lptr(out), eb, len(eb))
    assert rc == L.CCSC_E_UNSUPPORTED
    g, K = (2, (1 << 30) - 1, 1), 1                      # ... M = 2^31 - 2 is not
    for row in ((1 << 31) - 3, (1 << 31) - 4):
        a = (g, (1, 3, 1), 1, K, row, (0, (1 << 30) - 9, 0), (2, 8, 1), (1, 0, 0), 0, 5)
        assert _index(L, *a) == _want(*a)
    g = ((1 << 31) - 1, 1, 1)                            # M = 2^31 - 1: row 2^31 - 2, and sums
    for row, p in (((1 << 31) - 2, 1), ((1 << 31) - 2, (1 << 31) - 4), (0, (1 << 31) - 2)):
        a = (g, (1001, 1, 1), 1, 1, row, ((1 << 31) - 9, 0, 0), (8, 1, 1), (p, 0, 0), 0, 2)
        assert _index(L, *a) == _want(*a)                # of coordinates that leave int32
    g, K = ((1 << 30) - 1, 1, 1), 2                      # the last row of the last filter
    a = (g, (5, 1, 1), 2, K, (1 << 31) - 3, ((1 << 30) - 17, 0, 0), (16, 1, 1), (1, 0, 0), 1, 7)
    assert _index(L, *a)[:4] == [(1 << 30) - 2, 0, 0, 1]
    assert _index(L, *a) == _want(*a)


SMALL = [((7, 5, 1), (3, 5, 1)), ((3, 3, 1), (3, 3, 1)), ((17, 17, 1), (11, 11, 1)),
         ((6, 5, 4), (3, 3, 3)), ((5, 5, 5), (5, 5, 5)), ((9, 8, 1), (1, 1, 1))]


@pytest.mark.parametrize("g,ks", SMALL)
def test_window_and_taps_on_every_tile_that_straddles_the_wrap(L, g, ks):
    """Small grids, exhaustively: every entry position against tiles at the start, across the
    end (a tile next to the wrap has its window on both sides) and over the whole axis, and
    every output point; ks = g included."""
    K, Cn = 2, 2
    tiles = []
    for a in range(3):
        t = {(0, g[a]), (g[a] - 1, 1), (g[a] // 2, g[a] - g[a] // 2)}
        if g[a] > 2:
            t.add((1, g[a] - 2))
        tiles.append(sorted(t))
    plane = g[0] * g[1] * g[2]
    points = list(itertools.product(*(sorted({0, gg - 1}) for gg in g)))
    points.append(tuple(gg // 2 for gg in g))
    for lo_ln in itertools.product(*tiles):
        lo, ln = tuple(v[0] for v in lo_ln), tuple(v[1] for v in lo_ln)
        for pos in range(plane):
            row = pos + plane * (K - 1)
            for p in points:
                a = (g, ks, Cn, K, row, lo, ln, p, 1, 3)
                assert _index(L, *a) == _want(*a), a


def test_window_test_agrees_with_the_footprints(L):
    """The window is exactly the set of entries that reach some output of the tile: checked
    against the tap test over all outputs, on a grid where the window wraps (13, r = 2)."""
    g, ks = (13, 11, 1), (5, 3, 1)
    for lo, ln in [((11, 9, 0), (2, 2, 1)), ((0, 0, 0), (4, 3, 1)), ((5, 4, 0), (8, 7, 1))]:
        for row in range(g[0] * g[1]):
            reach = False
            for px in range(lo[0], lo[0] + ln[0]):
                for py in range(lo[1], lo[1] + ln[1]):
                    reach |= _index(L, g, ks, 1, 1, row, lo, ln, (px, py, 0), 0, 0)[5] >= 0
            assert _index(L, g, ks, 1, 1, row, lo, ln, (lo[0], lo[1], 0), 0, 0)[4] == int(reach)


def test_index_hook_rejects_what_lies_outside_the_grid(L):
    eb = L.errbuf()
    out = np.zeros(8, dtype=np.int64)
    g, ks = (6, 5, 1), (3, 3, 1)
    for row, lo, ln, p, c in [(60, (0, 0, 0), (1, 1, 1), (0, 0, 0), 0),
                              (-1, (0, 0, 0), (1, 1, 1), (0, 0, 0), 0),
                              (0, (5, 0, 0), (2, 1, 1), (0, 0, 0), 0),
                              (0, (0, 0, 0), (1, 1, 1), (6, 0, 0), 0),
                              (0, (0, 0, 0), (1, 1, 1), (0, 0, 0), 1)]:
        rc = L.lib().ccsc_test_synth_index(_i3(g), _i3(ks), 1, 2, row, _i3(lo), _i3(ln), _i3(p), c,
                                           0, L.lptr(out), eb, len(eb))
        assert rc == L.CCSC_E_INVALID, (row, lo, ln, p, c)
