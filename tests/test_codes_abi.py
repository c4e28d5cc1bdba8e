"""CPU: the compressed-sparse-column entry points validate their arguments before they
touch a device (so no GPU is needed to see the reasons), and the one place the kernels'
offsets are computed (csrc/codes.hpp, through ccsc_test_codes_index) is exact in 64 bits at
sizes no test matrix reaches."""
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


def _count(L, entry, eps, jc):
    eb = L.errbuf()
    a = np.zeros((4, 2), order="F")
    fn = getattr(L.lib(), entry)
    if entry.startswith("ccsc_session"):
        rc = fn(None, eps, L.lptr(jc), None, None, eb, len(eb))
    elif entry.endswith("_dev"):
        rc = fn(None, a.ctypes.data, 4, 2, eps, None if jc is None else jc.ctypes.data, eb, len(eb))
    else:
        rc = fn(None, L.dptr(a), 4, 2, eps, L.lptr(jc), eb, len(eb))
    return rc, eb.value.decode()


def _fill(L, entry, eps, capacity):
    eb = L.errbuf()
    a = np.zeros((4, 2), order="F")
    ir = np.zeros(8, dtype=np.int64)
    pr = np.zeros(8)
    fn = getattr(L.lib(), entry)
    if entry.startswith("ccsc_session"):
        rc = fn(None, eps, L.lptr(ir), L.dptr(pr), capacity, eb, len(eb))
    elif entry.endswith("_dev"):
        rc = fn(None, a.ctypes.data, 4, 2, eps, ir.ctypes.data, pr.ctypes.data, capacity, eb,
                len(eb))
    else:
        rc = fn(None, L.dptr(a), 4, 2, eps, L.lptr(ir), L.dptr(pr), capacity, eb, len(eb))
    return rc, eb.value.decode()


COUNTS = ["ccsc_sparsify_count", "ccsc_sparsify_count_dev", "ccsc_session_codes_count"]
FILLS = ["ccsc_sparsify_fill", "ccsc_sparsify_fill_dev", "ccsc_session_codes_fill"]


@pytest.mark.parametrize("entry", COUNTS + FILLS)
@pytest.mark.parametrize("eps", [-1.0, -1e-300, float("-inf"), float("nan")])
def test_bad_eps_is_invalid_with_a_reason(L, entry, eps):
    jc = np.zeros(3, dtype=np.int64)
    rc, msg = _count(L, entry, eps, jc) if entry in COUNTS else _fill(L, entry, eps, 8)
    assert rc == L.CCSC_E_INVALID and "eps" in msg, (rc, msg)


@pytest.mark.parametrize("entry", COUNTS)
def test_null_jc_is_invalid_with_a_reason(L, entry):
    rc, msg = _count(L, entry, 0.5, None)
    assert rc == L.CCSC_E_INVALID and "jc" in msg, (rc, msg)


@pytest.mark.parametrize("entry", FILLS)
def test_negative_capacity_is_invalid_with_a_reason(L, entry):
    rc, msg = _fill(L, entry, 0.5, -1)
    assert rc == L.CCSC_E_INVALID and "capacity" in msg, (rc, msg)


def test_valid_arguments_pass_validation(L):
    """With eps, jc and the capacity in order the next complaint is the missing context or
    session -- legal values (0, +inf) are not rejected on the way."""
    jc = np.zeros(3, dtype=np.int64)
    for eps in (0.0, 0.5, float("inf")):
        rc, msg = _count(L, "ccsc_sparsify_count", eps, jc)
        assert rc == L.CCSC_E_INVALID and "ctx" in msg, (rc, msg)
        rc, msg = _fill(L, "ccsc_sparsify_fill", eps, 0)
        assert rc == L.CCSC_E_INVALID and "ctx" in msg, (rc, msg)
        rc, msg = _count(L, "ccsc_session_codes_count", eps, jc)
        assert rc == L.CCSC_E_STATE, (rc, msg)


def test_rows_from_2_pow_31_are_unsupported(L):
    eb = L.errbuf()
    jc = np.zeros(2, dtype=np.int64)
    a = np.zeros(1)
    rc = L.lib().ccsc_sparsify_count(None, L.dptr(a), 1 << 31, 1, 0.0, L.lptr(jc), eb, len(eb))
    assert rc == L.CCSC_E_UNSUPPORTED and b"2^31" in eb.value


TILE, RUN = 2048, 512     # rows of a column per workgroup, per wave


def _index(L, M, tile, wave, step, lane, tile_off, before, prefix):
    out = np.zeros(4, dtype=np.int64)
    eb = L.errbuf()
    L.check(L.lib().ccsc_test_codes_index(M, tile, wave, step, lane, tile_off, before, prefix,
                                          L.lptr(out), eb, len(eb)), eb)
    return [int(v) for v in out]


@pytest.mark.parametrize("M,col,tic", [
    (1, 0, 0), (2047, 3, 0), (2048, 3, 0), (2049, 3, 1), (1210000, 9999, 590),
    # element index and slots far past 2^32 (and past 2^62)
    ((1 << 31) - 1, 3_000_000_000, 1048575), (1210000, 7 * 10 ** 12, 123)])
def test_offset_arithmetic_is_exact_in_64_bits(L, M, col, tic):
    tpc = -(-M // TILE)
    tile = col * tpc + tic
    for wave, step, lane, prefix in [(0, 0, 0, 0), (3, 7, 63, 63), (1, 2, 5, 4)]:
        tile_off, before = (1 << 40) + 12345, 1500
        got = _index(L, M, tile, wave, step, lane, tile_off, before, prefix)
        row = tic * TILE + wave * RUN + step * 64 + lane
        assert got == [col, row, col * M + row, tile_off + before + prefix]
        assert col * M + row < 1 << 63


def test_index_hook_rejects_lanes_outside_the_tile(L):
    eb = L.errbuf()
    out = np.zeros(4, dtype=np.int64)
    for wave, step, lane in [(4, 0, 0), (0, 8, 0), (0, 0, 64)]:
        rc = L.lib().ccsc_test_codes_index(10, 0, wave, step, lane, 0, 0, 0, L.lptr(out), eb,
                                           len(eb))
        assert rc == L.CCSC_E_INVALID
