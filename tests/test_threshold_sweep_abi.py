"""CPU: ccsc_threshold_sweep* validate every argument before they touch a device (a NULL
context shows the reasons without a GPU); the threshold class the sweep's kernels give a value
(csrc/sweep_codes.hpp, through ccsc_test_sweep_class) agrees with the NumPy predicate
``~(abs(v) <= eps)`` counted over the list; learners.pick_eps on hand-made sweeps."""
import ctypes as C

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
            b=True, crop=1, eps=(0.5, 0.0, 0.25), E=3, nnz_out=True, l1_out=True, sse_out=True)
ENTRIES = ["ccsc_threshold_sweep", "ccsc_threshold_sweep_dev"]


def _sweep(L, entry, **kw):
    a = dict(GOOD, **kw)
    arr = dict(d=np.zeros(3 * 3 * 2), jc=np.array([0, 2, 4], dtype=np.int64),
               ir=np.zeros(4, dtype=np.int64), pr=np.zeros(4), b=np.zeros(6 * 5 * 2),
               nnz_out=np.zeros(16, dtype=np.int64), l1_out=np.zeros(16), sse_out=np.zeros(16))
    eps = None if a["eps"] is None else np.array(a["eps"], dtype=np.float64)
    eb = L.errbuf()
    fn = getattr(L.lib(), entry)
    if entry.endswith("_dev"):
        p = {k: (x.ctypes.data if a[k] else None) for k, x in arr.items()}
    else:
        p = {k: (L.lptr if x.dtype == np.int64 else L.dptr)(x if a[k] else None)
             for k, x in arr.items()}
    rc = fn(None, p["d"], _i3(a["ks"]), a["C"], a["K"], _i3(a["g"]), p["jc"], p["ir"], p["pr"],
            a["n"], a["nnz"], p["b"], a["crop"], L.dptr(eps), a["E"], p["nnz_out"], p["l1_out"],
            p["sse_out"], eb, len(eb))
    return rc, eb.value.decode()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kw,word", [
    (dict(d=False), "d"), (dict(ks=None), "ks"), (dict(g=None), "g"), (dict(jc=False), "jc"),
    (dict(ir=False), "ir"), (dict(pr=False), "pr"),
    (dict(ks=(2, 3, 1)), "ks[0]"), (dict(ks=(3, 4, 1)), "ks[1]"), (dict(ks=(3, 3, 2)), "ks[2]"),
    (dict(ks=(0, 3, 1)), "ks[0]"), (dict(ks=(3, -1, 1)), "ks[1]"), (dict(ks=(3, 3, 0)), "ks[2]"),
    (dict(ks=(7, 3, 1)), "ks[0]"), (dict(ks=(3, 7, 1)), "ks[1]"), (dict(ks=(3, 3, 3)), "ks[2]"),
    (dict(g=(0, 5, 1)), "g[0]"), (dict(C=0), "C"), (dict(K=0), "K"), (dict(n=-1), "n"),
    (dict(nnz=-1), "nnz"),
    (dict(b=False), "b"), (dict(eps=None), "eps"), (dict(E=0), "E"), (dict(E=-3), "E"),
    (dict(nnz_out=False), "nnz_out"), (dict(l1_out=False), "l1_out"),
    (dict(sse_out=False), "sse_out"),
    (dict(eps=(0.5, float("nan"), 0.25)), "eps[1]"), (dict(eps=(float("nan"),), E=1), "eps[0]")])
def test_rejections_are_invalid_and_name_the_argument(L, entry, kw, word):
    rc, msg = _sweep(L, entry, **kw)
    assert rc == L.CCSC_E_INVALID and word in msg and "ctx" not in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_limits_are_unsupported_with_a_reason(L, entry):
    rc, msg = _sweep(L, entry, g=(32768, 32768, 1), K=2)           # M = 2^31
    assert rc == L.CCSC_E_UNSUPPORTED and "2^31" in msg and "M" in msg, (rc, msg)
    rc, msg = _sweep(L, entry, g=(1025, 1025, 1), ks=(1025, 1025, 1), C=1 << 11, K=1)
    assert rc == L.CCSC_E_UNSUPPORTED and "filters" in msg and " d " in msg, (rc, msg)


@pytest.mark.parametrize("entry", ENTRIES)
def test_valid_arguments_reach_the_context_check(L, entry):
    inf = float("inf")
    for kw in (dict(), dict(crop=0),
               dict(n=0, b=False, nnz_out=False, l1_out=False, sse_out=False),
               dict(nnz=0, ir=False, pr=False), dict(eps=(-1.0, inf, -inf), E=3),
               dict(eps=(0.0,), E=1), dict(eps=tuple(range(9)), E=9),
               dict(ks=(5, 5, 1), g=(5, 5, 1)), dict(ks=(1, 1, 1))):
        rc, msg = _sweep(L, entry, **kw)
        assert rc == L.CCSC_E_INVALID and "NULL ctx" in msg, (kw, rc, msg)


# ---- the threshold class --------------------------------------------------------------------

TINY = 5e-324                    # the smallest denormal
VALUES = [0.0, -0.0, TINY, -TINY, 2 * TINY, 0.25, -0.25, 0.5, np.nextafter(0.5, 1), 1.0, -3.0,
          1e308, np.inf, -np.inf, np.nan, -np.nan]
LISTS = [
    [0.0], [-1.0], [np.inf], [-np.inf], [TINY], [0.25],
    [0.5, 0.25, 0.25, -1.0, 0.0, np.inf, TINY, 1.0],                     # E = 8, unsorted, a tie
    [1.0, 0.25, 0.5, 0.25, 0.0, -1.0, np.inf, 0.25, TINY],               # E = 9: two groups
    [0.25] * 9, [np.inf, -np.inf, 0.0], list(np.linspace(2.0, -2.0, 17)),
]


def _class(L, eps, v):
    e = np.array(eps, dtype=np.float64)
    m = C.c_int32(-1)
    eb = L.errbuf()
    L.check(L.lib().ccsc_test_sweep_class(L.dptr(e), len(e), float(v), C.byref(m), eb, len(eb)),
            eb)
    return m.value


@pytest.mark.parametrize("eps", LISTS, ids=lambda e: f"E{len(e)}-{e[0]}")
def test_class_is_the_numpy_predicate_counted_over_the_list(L, eps):
    e = np.sort(np.array(eps, dtype=np.float64))
    for v in VALUES:
        with np.errstate(invalid="ignore"):
            kept = ~(np.abs(v) <= e)
        want = int(kept.sum())
        assert _class(L, eps, v) == want, (eps, v)
        # monotone: over the ascending list the survived thresholds are the first ones
        assert np.array_equal(kept, np.arange(len(e)) < want), (eps, v)


def test_class_edges(L):
    assert _class(L, [0.0], 0.0) == 0 and _class(L, [0.0], -0.0) == 0      # zeros drop at 0 ...
    assert _class(L, [-1.0], 0.0) == 1 and _class(L, [-np.inf], -0.0) == 1  # ... not below it
    assert _class(L, [0.0], TINY) == 1 and _class(L, [TINY], -TINY) == 0
    assert _class(L, [0.5, 0.5, 0.5], -0.5) == 0                             # a tie is dropped
    assert _class(L, [0.5, 0.5, np.nextafter(0.5, 0)], 0.5) == 1
    assert _class(L, [np.inf], np.inf) == 0 and _class(L, [1e308], -np.inf) == 1
    assert _class(L, [np.inf, -1.0, 0.0] * 3, np.nan) == 9                   # a NaN is kept


def test_class_hook_rejections(L):
    eb = L.errbuf()
    m = C.c_int32(0)
    e = np.array([0.0, np.nan])
    fn = L.lib().ccsc_test_sweep_class
    assert fn(None, 1, 0.0, C.byref(m), eb, len(eb)) == L.CCSC_E_INVALID
    assert fn(L.dptr(e), 0, 0.0, C.byref(m), eb, len(eb)) == L.CCSC_E_INVALID
    assert fn(L.dptr(e), 2, 0.0, C.byref(m), eb, len(eb)) == L.CCSC_E_INVALID
    assert "eps[1]" in eb.value.decode()
    assert fn(L.dptr(e), 1, 0.0, None, eb, len(eb)) == L.CCSC_E_INVALID
    assert fn(L.dptr(e), 1, 1.0, C.byref(m), eb, len(eb)) == L.CCSC_OK and m.value == 1


# ---- pick_eps -------------------------------------------------------------------------------

def test_pick_eps_on_hand_made_sweeps():
    from ccsc_code_iccv2017_amd.learners import pick_eps
    sw = {"eps": np.array([0.3, 0.0, 0.1, 0.2]),
          "sse": np.array([[9.0, 9.0], [5.0, 5.0], [5.2, 5.2], [5.5, 5.6]])}
    assert pick_eps(sw, 0.0) == 0.0
    assert pick_eps(sw, 0.05) == 0.1            # 10.4 <= 10.5
    assert pick_eps(sw, 0.03) == 0.0            # 10.4 > 10.3
    assert pick_eps(sw, 0.2) == 0.2             # 11.1 <= 12, 18 is not
    assert pick_eps(sw, 1.0) == 0.3
    # the totals decide, not a single column; the order of the list does not matter
    sw = {"eps": [0.0, 1.0], "sse": np.array([[1.0, 10.0], [3.0, 8.5]])}
    assert pick_eps(sw, 0.05) == 1.0
    # not monotone: the largest qualifying threshold, even past one that does not qualify
    sw = {"eps": [0.0, 1.0, 2.0], "sse": np.array([[4.0], [9.0], [4.0]])}
    assert pick_eps(sw, 0.0) == 2.0
    # nothing else qualifies, a NaN total, one threshold: the smallest threshold
    assert pick_eps({"eps": [0.5, 0.1], "sse": np.array([[7.0], [1.0]])}, 0.5) == 0.1
    assert pick_eps({"eps": [0.1, 0.5], "sse": np.array([[np.nan], [1.0]])}, 0.5) == 0.1
    assert pick_eps({"eps": [0.25], "sse": np.array([[2.0, 3.0]])}, 0.0) == 0.25
    # a negative smallest threshold is the base
    assert pick_eps({"eps": [0.2, -1.0], "sse": np.array([[1.0], [1.0]])}, 0.0) == 0.2
    with pytest.raises(ValueError):
        pick_eps({"eps": [0.1, 0.2], "sse": np.zeros((3, 1))}, 0.1)
    with pytest.raises(ValueError):
        pick_eps(sw, -0.1)
