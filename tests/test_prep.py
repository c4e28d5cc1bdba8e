"""Nearest-sample fill and per-plane standardisation on the GPU: csrc/prep.hip behind
ccsc_nn_fill / ccsc_standardize / ccsc_unstandardize (and their _dev forms), synth.nn_fill,
synth.standardize, synth.unstandardize; and synth.interp_views.

Yardsticks, all in this module:
  nn_fill_ref       an all-pairs search with int64 squared distances; the samples are sorted
                    by column-major index and argmin takes the first minimum, so a tie goes
                    to the smallest column-major index.  The fill only copies values, so the
                    comparison is exact (bytes).
  standardize_ref   math.fsum-exact sums, then mean = S / N, sdev = sqrt(S2 / (N - 1)) with
                    the rounded mean in the deviations.
  interp_views_ref  the literal loop over ss = 2, 3, 4 in MATLAB order.

Standardisation bounds (derived, not measured; u = 2^-53):
  mean  |mean - ref| <= N u mean(|x|): an N-term sum in any order, divided by N.
  sdev  |sdev - ref| <= 2 N u ref for N >= 8: twice the first-order bound (N / 2 + 4) u of
        the two-pass form (the mean's error enters only quadratically); 16 u ref for N = 2, 7.
  out   (x - m) / s with the returned m and s, and x * s + m, are single correctly rounded
        operations: compared bit for bit with NumPy.
  round trip  |x' - x| <= 4 u (|x| + |m|).

The CPU tests hold the yardsticks themselves: the all-pairs distances to SciPy's Euclidean
distance transform, and the kernels' separable rule (nearest row per column, the upper on a
tie; then the nearest column, the left on a tie) to the all-pairs rule.

Inputs are seeded; arrays are shared between tests and never written."""
import ctypes as C
import functools
import math
import os
import re

import numpy as np
import pytest
import scipy.ndimage

from ccsc_code_iccv2017_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TILE_H, TILE_W = 64, 4    # kFillTileH, kFillTileW of csrc/prep.hip (test_constants_match_the_kernel)
CHUNK = 4096              # its kStdChunk
LAUNCH_LOG2 = 22          # its kPrepMaxBlocks: 2^22 workgroups per launch
STAGE_BYTES = 256 << 20   # prep_chunk of csrc/solve.cpp: the host entries' staging chunk
U = 2.0 ** -53


def _bits(a):
    return np.asfortranarray(a).tobytes(order="F")


# ---- yardsticks --------------------------------------------------------------------------

def nn_fill_ref(a, known=None):
    """(out, idx, d2) of one [H, W] plane; d2 is the squared distance to the chosen sample
    (-1 in a plane without a sample)."""
    H, W = a.shape
    k = (a != 0) if known is None else (known != 0)
    out = np.array(a, dtype=np.float64, order="F")
    idx = np.full((H, W), -1, dtype=np.int32, order="F")
    d2 = np.full((H, W), -1, dtype=np.int64, order="F")
    s = np.flatnonzero(k.ravel(order="F"))            # ascending column-major index
    if s.size == 0:
        return out, idx, d2
    si, sj = (s % H).astype(np.int64), (s // H).astype(np.int64)
    q = np.arange(H * W, dtype=np.int64)
    qi, qj = q % H, q // H
    D = (qi[:, None] - si[None, :]) ** 2 + (qj[:, None] - sj[None, :]) ** 2
    best = np.argmin(D, axis=1)                       # the first minimum
    src = s[best]
    idx[...] = src.reshape((H, W), order="F")
    d2[...] = D[q, best].reshape((H, W), order="F")
    flat = out.ravel(order="F")
    out = np.asfortranarray(flat[src].reshape((H, W), order="F"))
    return out, idx, d2


def separable_idx(known):
    """The kernels' rule on one plane: r(i, j) the nearest sample row of column j (the smaller
    row on a tie), then for (i, j) the column j' minimising ((j - j')^2 + (i - r(i, j'))^2, j')."""
    H, W = known.shape
    r = np.full((H, W), -1, dtype=np.int64)
    rows_i = np.arange(H, dtype=np.int64)
    for j in range(W):
        rows = np.flatnonzero(known[:, j])
        if rows.size:
            r[:, j] = rows[np.argmin(np.abs(rows_i[:, None] - rows[None, :]), axis=1)]
    idx = np.full((H, W), -1, dtype=np.int32, order="F")
    cols = np.arange(W, dtype=np.int64)
    big = np.iinfo(np.int64).max
    for i in range(H):
        rr = r[i]
        if not (rr >= 0).any():
            continue
        D = (cols[:, None] - cols[None, :]) ** 2 + ((i - rr) ** 2)[None, :]
        D[:, rr < 0] = big
        jp = np.argmin(D, axis=1)                     # the first minimum: the smallest j'
        idx[i] = rr[jp] + H * jp
    return idx


def standardize_ref(x2):
    """x2: [N, planes].  (mean, sdev) per plane."""
    N, P = x2.shape
    mean, sdev = np.empty(P), np.empty(P)
    for p in range(P):
        v = x2[:, p]
        m = math.fsum(v) / N
        mean[p] = m
        sdev[p] = math.sqrt(math.fsum((v - m) ** 2) / (N - 1))
    return mean, sdev


def interp_views_ref(s):
    s = np.array(s, dtype=np.float64)
    for ss in (2, 3, 4):                              # 1-based, as the driver writes it
        a = ss - 1
        new = (s[:, :, a + 1, 1:-1] + s[:, :, a - 1, 1:-1]) / 2
        s[:, :, a, 1:-1] = new
        new = (s[:, :, 1:-1, a + 1] + s[:, :, 1:-1, a - 1]) / 2
        s[:, :, 1:-1, a] = new
    return s


# ---- fill cases --------------------------------------------------------------------------

def _values(mask, seed):
    a = np.random.default_rng(seed).standard_normal(mask.shape) * mask
    return np.asfortranarray(a + 0.0)                 # no -0.0 outside the samples


def _mosaic(size, sb):
    """reconstruct_subsampling_hyperspectral.m:21-29: plane c samples offset (m, n) of every
    sb x sb cell, c = m * sb + n."""
    mask = np.zeros((size, size, sb * sb))
    c = 0
    for m in range(sb):
        for n in range(sb):
            mask[m::sb, n::sb, c] = 1
            c += 1
    return mask


def _line(shape):
    m = np.zeros(shape)
    m.reshape(-1)[[3, 11]] = 1
    return m


def _corner():
    m = np.zeros((40, 70))
    m[39, 69] = 1
    return m


@functools.lru_cache(maxsize=None)
def _case(name):
    """(a, reference out, reference idx, reference d2) of a named case; a is [H, W, planes]."""
    masks = {
        "1x1_sample": lambda: np.ones((1, 1)),
        "1x1_zero": lambda: np.zeros((1, 1)),
        "1x17_tie": lambda: _line((1, 17)),
        "17x1_tie": lambda: _line((17, 1)),
        "mosaic_36_p3": lambda: _mosaic(36, 3),
        "mosaic_34_p2": lambda: _mosaic(34, 2),
        "45x70_sparse": lambda: np.random.default_rng(5).random((45, 70)) < 0.02,
        "40x70_corner": _corner,
        "tile_plus_one": lambda: np.random.default_rng(6).random((TILE_H + 1, TILE_W + 1)) < 0.05,
        "300x200_sparse": lambda: np.random.default_rng(7).random((300, 200)) < 0.001,
    }
    mask = np.asarray(masks[name](), dtype=np.float64)
    mask = mask.reshape(mask.shape[:2] + (-1,))
    a = _values(mask, 11)
    refs = [nn_fill_ref(a[:, :, p]) for p in range(a.shape[2])]
    out = np.asfortranarray(np.stack([r[0] for r in refs], axis=2))
    idx = np.asfortranarray(np.stack([r[1] for r in refs], axis=2))
    d2 = np.stack([r[2] for r in refs], axis=2)
    for arr in (a, out, idx, d2):
        arr.setflags(write=False)
    return a, out, idx, d2


FILL_CASES = ["1x1_sample", "1x1_zero", "1x17_tie", "17x1_tie", "mosaic_36_p3", "mosaic_34_p2",
              "45x70_sparse", "40x70_corner", "tile_plus_one", "300x200_sparse"]


# ---- CPU: the yardsticks -----------------------------------------------------------------

@pytest.mark.parametrize("name", FILL_CASES)
def test_all_pairs_distances_are_the_distance_transform(name):
    a, _, _, d2 = _case(name)
    for p in range(a.shape[2]):
        known = a[:, :, p] != 0
        if not known.any():
            assert np.all(d2[:, :, p] == -1)
            continue
        edt = scipy.ndimage.distance_transform_edt(~known)
        assert np.array_equal(np.rint(edt ** 2).astype(np.int64), d2[:, :, p])


@pytest.mark.parametrize("name", FILL_CASES + ["37x29", "33x65"])
def test_separable_rule_is_the_all_pairs_rule(name):
    if name in FILL_CASES:
        a, _, idx, _ = _case(name)
    else:
        H, W = map(int, name.split("x"))
        a = _values(np.random.default_rng(H).random((H, W, 1)) < 0.03, 3)
        idx = np.stack([nn_fill_ref(a[:, :, 0])[1]], axis=2)
    for p in range(a.shape[2]):
        assert np.array_equal(separable_idx(a[:, :, p] != 0), idx[:, :, p])


def test_the_sparse_case_has_ties_and_the_corner_case_spans_the_plane():
    a, _, idx, d2 = _case("45x70_sparse")
    known = a[:, :, 0] != 0
    assert known.sum() == 70
    s = np.flatnonzero(known.ravel(order="F"))
    q = np.arange(known.size)
    D = (q[:, None] % 45 - s[None, :] % 45) ** 2 + (q[:, None] // 45 - s[None, :] // 45) ** 2
    tied = ((D == D.min(axis=1, keepdims=True)).sum(axis=1) >= 2) & ~known.ravel(order="F")
    assert tied.sum() == 160
    assert _case("40x70_corner")[3].max() == 6282
    for name in ("1x17_tie", "17x1_tie"):             # the midpoint goes to the smaller index
        assert _case(name)[2].ravel(order="F")[7] == 3
    assert np.all(_case("1x1_zero")[2] == -1) and np.all(_case("1x1_sample")[2] == 0)


def test_mosaic_midpoints_are_tied_at_period_2():
    a, _, _, _ = _case("mosaic_34_p2")
    known = a[:, :, 0] != 0
    assert known[0::2, 0::2].all() and known.sum() == 17 * 17
    assert _case("mosaic_36_p3")[0].shape == (36, 36, 9)


def test_interp_views_is_the_literal_loop():
    s = np.random.default_rng(9).standard_normal((6, 5, 5, 5))
    want = interp_views_ref(s)
    got = synth.interp_views(np.asfortranarray(s))
    assert got.shape == s.shape and _bits(got) == _bits(want)
    # sequential: ss = 3 reads what ss = 2 wrote, so one simultaneous update differs
    once = s.copy()
    once[:, :, 1:4, 1:-1] = (s[:, :, 2:5, 1:-1] + s[:, :, 0:3, 1:-1]) / 2
    assert not np.array_equal(once, want)
    import torch
    assert _bits(synth.interp_views(torch.as_tensor(s)).numpy()) == _bits(want)


def test_the_new_entries_are_bound():
    from ccsc_code_iccv2017_amd import _lib as L
    hdr = open(os.path.join(ROOT, "include", "ccsc.h")).read()
    for name in ("ccsc_nn_fill", "ccsc_standardize", "ccsc_unstandardize"):
        for entry in (name, name + "_dev"):
            assert entry in L.SIGNATURES
            assert re.search(r"int32_t %s\(" % entry, hdr)
    assert len(L.SIGNATURES["ccsc_nn_fill"][1]) == 10
    assert len(L.SIGNATURES["ccsc_standardize"][1]) == 9
    for fn in ("nn_fill", "standardize", "unstandardize", "interp_views"):
        assert callable(getattr(synth, fn))


def test_constants_match_the_kernel():
    src = open(os.path.join(ROOT, "ccsc_code_iccv2017_amd", "csrc", "prep.hip")).read()
    nt = int(re.search(r"constexpr int kPrepNT = (\d+);", src).group(1))
    assert int(re.search(r"constexpr int kFillTileH = (\d+);", src).group(1)) == TILE_H
    assert re.search(r"constexpr int kFillTileW = kPrepNT / kFillTileH;", src)
    assert nt // TILE_H == TILE_W
    assert int(re.search(r"constexpr int kStdChunk = (\d+);", src).group(1)) == CHUNK
    assert re.search(r"kPrepMaxBlocks = \(int64_t\)1 << (\d+);", src).group(1) == str(LAUNCH_LOG2)
    host = open(os.path.join(ROOT, "ccsc_code_iccv2017_amd", "csrc", "solve.cpp")).read()
    body = host[host.index("static int64_t prep_chunk("):]
    assert int(re.search(r"\((\d+)LL << 20\) / \(per \* 8\)", body).group(1)) << 20 == STAGE_BYTES


# ---- GPU: fill ---------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", FILL_CASES)
def test_fill_equals_the_all_pairs_search(name):
    a, out, idx, _ = _case(name)
    got, gi = synth.nn_fill(a, return_index=True)
    assert got.flags.f_contiguous and gi.dtype == np.int32 and gi.shape == a.shape
    print("pixels with another source:", int((gi != idx).sum()))
    assert np.array_equal(gi, idx)
    assert _bits(got) == _bits(out)
    assert _bits(synth.nn_fill(a)) == _bits(out)


@pytest.mark.gpu
def test_nan_is_a_sample_and_negative_zero_is_not():
    a = np.zeros((5, 6), order="F")
    a[1, 1] = np.nan
    a[4, 5] = 2.0
    a[0, 3] = -0.0
    a[3, 0] = -0.0
    out, idx, _ = nn_fill_ref(a)
    got, gi = synth.nn_fill(a, return_index=True)
    assert np.array_equal(gi, idx) and _bits(got) == _bits(out)
    assert np.isnan(got[0, 3]) and np.isnan(got[3, 0])


@pytest.mark.gpu
def test_batch_with_an_empty_plane_equals_single_planes_bitwise():
    base = _case("45x70_sparse")[0][:, :, 0]
    planes = [np.roll(base, 3 * p, axis=1) * (p != 2) + 0.0 for p in range(5)]
    a = np.asfortranarray(np.stack(planes, axis=2))
    whole, wi = synth.nn_fill(a, return_index=True)
    assert _bits(whole[:, :, 2]) == _bits(a[:, :, 2]) and np.all(wi[:, :, 2] == -1)
    for p in range(5):
        one, oi = synth.nn_fill(np.asfortranarray(a[:, :, p]), return_index=True)
        assert _bits(one) == _bits(whole[:, :, p]), p
        assert np.array_equal(oi, wi[:, :, p]), p
        assert np.array_equal(oi, nn_fill_ref(a[:, :, p])[1]), p


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["45x70_sparse", "mosaic_34_p2"])
def test_explicit_mask_overwrites_garbage_and_propagates_zeros(name):
    a = _case(name)[0]
    known = np.asfortranarray((a != 0).astype(np.float64))
    rng = np.random.default_rng(21)
    data = np.where(known != 0, a, rng.standard_normal(a.shape) + 5.0)    # garbage elsewhere
    zeroed = (rng.random(a.shape) < 0.3) & (known != 0)
    data = np.asfortranarray(np.where(zeroed, 0.0, data))                # true zeros at samples
    assert zeroed.any()
    refs = [nn_fill_ref(data[:, :, p], known[:, :, p]) for p in range(a.shape[2])]
    out = np.stack([r[0] for r in refs], axis=2)
    idx = np.stack([r[1] for r in refs], axis=2)
    got, gi = synth.nn_fill(data, known=known, return_index=True)
    assert np.array_equal(gi, idx) and _bits(got) == _bits(out)
    assert np.array_equal(gi, _case(name)[2])          # the mask alone decides the sources
    assert set(np.unique(got)) <= set(np.unique(data[known != 0]))


def _raw_fill(gpu_ctx, entry="ccsc_nn_fill", a=None, out=None, known=None, idx=None, n=1, H=4,
              W=4, null=()):
    """One raw ABI call on host arrays; returns (code, message, out)."""
    from ccsc_code_iccv2017_amd import _lib as L
    a = np.ones(16) if a is None else a
    out = np.full(a.size, -7.0) if out is None else out
    args = {"in": L.dptr(a), "known": L.dptr(known), "out": L.dptr(out), "idx": L.iptr(idx)}
    for name in null:
        args[name] = None
    if entry.endswith("_dev"):
        args = {k: C.cast(v, C.c_void_p) for k, v in args.items()}
    eb = L.errbuf()
    rc = getattr(L.lib(), entry)(gpu_ctx.ptr, args["in"], args["known"], args["out"],
                                 args["idx"], n, H, W, eb, len(eb))
    return rc, eb.value.decode(), out


@pytest.mark.gpu
def test_fill_in_place_host_and_device(gpu_ctx):
    import torch
    from ccsc_code_iccv2017_amd import _lib as L
    a, out, idx, _ = _case("mosaic_36_p3")
    H, W, n = a.shape
    x = np.array(a, order="F")
    rc, msg, _ = _raw_fill(gpu_ctx, a=x, out=x, n=n, H=H, W=W)
    assert rc == 0, msg
    assert _bits(x) == _bits(out)
    t = torch.as_tensor(np.array(a.transpose(2, 1, 0), order="C"), device="cuda")   # column-major a
    ti = torch.empty(t.shape, dtype=torch.int32, device="cuda")
    eb = L.errbuf()
    torch.cuda.synchronize()
    rc = L.lib().ccsc_nn_fill_dev(gpu_ctx.ptr, t.data_ptr(), None, t.data_ptr(), ti.data_ptr(),
                                  n, H, W, eb, len(eb))
    assert rc == 0, eb.value.decode()
    assert _bits(t.cpu().numpy().transpose(2, 1, 0)) == _bits(out)
    assert np.array_equal(ti.cpu().numpy().transpose(2, 1, 0), idx)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["45x70_sparse", "tile_plus_one", "mosaic_34_p2"])
def test_fill_host_entry_equals_device_entry_and_repeats_bitwise(name):
    import torch
    a = _case(name)[0]
    host, hi = synth.nn_fill(a, return_index=True)
    again, ai = synth.nn_fill(a, return_index=True)
    assert _bits(host) == _bits(again) and np.array_equal(hi, ai)
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    dev, di = synth.nn_fill(t, return_index=True)
    assert dev.is_cuda and dev.dtype == torch.float64 and tuple(dev.shape) == a.shape
    assert di.is_cuda and di.dtype == torch.int32 and tuple(di.shape) == a.shape
    assert _bits(dev.cpu().numpy()) == _bits(host)
    assert np.array_equal(di.cpu().numpy(), hi)


@pytest.mark.gpu
@pytest.mark.parametrize("kw,code,reason", [
    (dict(H=32769, W=1), -5, "above 32768"),
    (dict(H=1, W=32769), -5, "above 32768"),
    (dict(H=0, W=4, n=0), -1, "at least 1"),
    (dict(H=4, W=0), -1, "at least 1"),
    (dict(n=-1), -1, "n must be"),
    (dict(null=("in",)), -1, "NULL"),
    (dict(null=("out",)), -1, "NULL"),
], ids=lambda v: None if not isinstance(v, dict) else
   ",".join(f"{a}={b}" for a, b in v.items()).replace(" ", ""))
@pytest.mark.parametrize("entry", ["ccsc_nn_fill", "ccsc_nn_fill_dev"])
def test_fill_rejections_say_why_and_write_nothing(gpu_ctx, entry, kw, code, reason):
    """Both entries validate before they touch the device, so host pointers are safe to hand
    to the device entry here, and `out` keeps its fill."""
    rc, msg, out = _raw_fill(gpu_ctx, entry, **kw)
    assert rc == code, msg
    assert reason in msg
    assert np.all(out == -7.0)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["ccsc_nn_fill", "ccsc_nn_fill_dev"])
def test_fill_out_must_not_be_the_mask(gpu_ctx, entry):
    k = np.ones(16)
    rc, msg, _ = _raw_fill(gpu_ctx, entry, known=k, out=k)
    assert rc == -1 and "known" in msg
    assert np.all(k == 1.0)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["ccsc_nn_fill", "ccsc_nn_fill_dev"])
def test_fill_empty_batch_is_ok(gpu_ctx, entry):
    rc, msg, out = _raw_fill(gpu_ctx, entry, n=0)
    assert rc == 0, msg
    assert np.all(out == -7.0)


# ---- GPU: standardise --------------------------------------------------------------------

STD_N = [2, 7, 2500, CHUNK + 1, 3 * CHUNK + 5]
STD_PLANES = [1, 3, 25]


@functools.lru_cache(maxsize=None)
def _std_data(N):
    """[N, 25] standard normal + 10 (the first planes serve the smaller batches) and its
    reference (mean, sdev)."""
    x = np.asfortranarray(np.random.default_rng([31, N]).standard_normal((N, 25)) + 10.0)
    mean, sdev = standardize_ref(x)
    for arr in (x, mean, sdev):
        arr.setflags(write=False)
    return x, mean, sdev


def _shaped(x, N):
    """The [N, planes] array as the caller's array and its plane_dims: 50 x 50 views at 2500."""
    if N == 2500:
        return np.asfortranarray(x.reshape((50, 50, -1), order="F")), 2
    return x, 1


def _sdev_bound(N, ref):
    return (2 * N if N >= 8 else 16) * U * ref


@pytest.mark.gpu
@pytest.mark.parametrize("planes", STD_PLANES)
@pytest.mark.parametrize("N", STD_N)
def test_standardize_against_exact_sums(N, planes):
    x25, rm, rs = _std_data(N)
    x2 = np.asfortranarray(x25[:, :planes])
    x, pd = _shaped(x2, N)
    nb, m, s = synth.standardize(x, pd)
    assert nb.shape == x.shape and nb.flags.f_contiguous and m.shape == (planes,) == s.shape
    em = np.abs(m - rm[:planes])
    es = np.abs(s - rs[:planes])
    bm = N * U * np.abs(x2).mean(axis=0)
    bs = _sdev_bound(N, rs[:planes])
    print(f"mean: max share of the bound {float((em / bm).max()):.4f}; "
          f"sdev: {float((es / bs).max()):.4f}")
    assert np.all(em <= bm)
    assert np.all(es <= bs)
    sh = (1,) * pd + (planes,)
    assert _bits(nb) == _bits((x - m.reshape(sh)) / s.reshape(sh))
    back = synth.unstandardize(nb, m, s, pd)
    assert _bits(back) == _bits(nb * s.reshape(sh) + m.reshape(sh))
    assert np.all(np.abs(back - x) <= 4 * U * (np.abs(x) + np.abs(m.reshape(sh))))


@pytest.mark.gpu
@pytest.mark.parametrize("N", STD_N)
def test_standardize_is_batch_independent_repeatable_and_equal_on_the_device(N):
    import torch
    x25 = _std_data(N)[0]
    x, pd = _shaped(x25, N)
    nb, m, s = synth.standardize(x, pd)
    nb2, m2, s2 = synth.standardize(x, pd)
    assert (_bits(nb), _bits(m), _bits(s)) == (_bits(nb2), _bits(m2), _bits(s2))
    for p in (0, 7, 24):                              # odd planes start 8 bytes off at odd N
        one, pd1 = _shaped(np.asfortranarray(x25[:, p:p + 1]), N)
        nb1, m1, s1 = synth.standardize(one, pd1)
        assert _bits(m1) == _bits(m[p:p + 1]) and _bits(s1) == _bits(s[p:p + 1]), p
        assert _bits(nb1[..., 0]) == _bits(nb[..., p]), p
    t = torch.as_tensor(np.ascontiguousarray(x), device="cuda")
    dnb, dm, ds = synth.standardize(t, pd)
    assert dnb.is_cuda and dm.is_cuda and ds.is_cuda and tuple(dm.shape) == (25,)
    assert _bits(dnb.cpu().numpy()) == _bits(nb)
    assert _bits(dm.cpu().numpy()) == _bits(m) and _bits(ds.cpu().numpy()) == _bits(s)
    dback = synth.unstandardize(dnb, dm, ds, pd)
    assert dback.is_cuda
    assert _bits(dback.cpu().numpy()) == _bits(synth.unstandardize(nb, m, s, pd))


@pytest.mark.gpu
def test_standardize_a_whole_image():
    x = np.asfortranarray(_std_data(2500)[0][:, 3].reshape((50, 50), order="F"))
    nb, m, s = synth.standardize(x, 2)
    assert m.shape == () and s.shape == ()
    one, m1, s1 = synth.standardize(x[:, :, None], 2)
    assert _bits(nb) == _bits(one[:, :, 0]) and float(m) == float(m1[0]) and float(s) == float(s1[0])
    assert _bits(synth.unstandardize(nb, m, s, 2)) == _bits(nb * float(s) + float(m))


def _raw_std(gpu_ctx, entry="ccsc_standardize", planes=1, N=16, null=()):
    from ccsc_code_iccv2017_amd import _lib as L
    a, out = np.ones(16), np.full(16, -7.0)
    m, s = np.full(1, -7.0), np.full(1, -7.0)
    args = {"in": L.dptr(a), "out": L.dptr(out), "mean": L.dptr(m), "sdev": L.dptr(s)}
    for name in null:
        args[name] = None
    if entry.endswith("_dev"):
        args = {k: C.cast(v, C.c_void_p) for k, v in args.items()}
    eb = L.errbuf()
    rc = getattr(L.lib(), entry)(gpu_ctx.ptr, args["in"], args["out"], args["mean"], args["sdev"],
                                 planes, N, eb, len(eb))
    return rc, eb.value.decode(), (out, m, s)


@pytest.mark.gpu
@pytest.mark.parametrize("kw,code,reason", [
    (dict(N=1), -1, "at least 2"),
    (dict(N=0), -1, "at least 2"),
    (dict(N=1 << 31), -5, "2^31"),
    (dict(planes=-1), -1, "planes must be"),
    (dict(null=("in",)), -1, "NULL"),
    (dict(null=("out",)), -1, "NULL"),
    (dict(null=("mean",)), -1, "NULL"),
    (dict(null=("sdev",)), -1, "NULL"),
], ids=lambda v: None if not isinstance(v, dict) else
   ",".join(f"{a}={b}" for a, b in v.items()).replace(" ", ""))
@pytest.mark.parametrize("entry", ["ccsc_standardize", "ccsc_standardize_dev",
                                   "ccsc_unstandardize", "ccsc_unstandardize_dev"])
def test_standardize_rejections_say_why_and_write_nothing(gpu_ctx, entry, kw, code, reason):
    rc, msg, outs = _raw_std(gpu_ctx, entry, **kw)
    assert rc == code, msg
    assert reason in msg and entry.split("_")[1] in msg
    assert all(np.all(o == -7.0) for o in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["ccsc_standardize", "ccsc_standardize_dev",
                                   "ccsc_unstandardize", "ccsc_unstandardize_dev"])
def test_standardize_no_planes_is_ok(gpu_ctx, entry):
    rc, msg, outs = _raw_std(gpu_ctx, entry, planes=0)
    assert rc == 0, msg
    assert all(np.all(o == -7.0) for o in outs)


# ---- GPU: launch chunks and staging chunks -----------------------------------------------

@pytest.mark.gpu
def test_more_workgroups_than_one_launch():
    """One workgroup per 1-pixel plane, or per 2-value plane: the batch spills into a second
    launch, whose workgroups continue the numbering of the first."""
    n = (1 << LAUNCH_LOG2) + 3
    rng = np.random.default_rng(5)
    a = np.asfortranarray(rng.standard_normal((1, 1, n)) * (rng.random((1, 1, n)) < 0.5) + 0.0)
    got, gi = synth.nn_fill(a, return_index=True)
    assert _bits(got) == _bits(a)
    assert np.array_equal(gi.ravel(), np.where(a.ravel() != 0, 0, -1))
    x = np.asfortranarray(rng.standard_normal((2, n)) + 10.0)
    nb, m, s = synth.standardize(x, 1)
    assert _bits(m) == _bits((x[0] + x[1]) / 2)       # one rounded add, an exact halving
    ref = np.hypot(x[0] - m, x[1] - m)                # N - 1 = 1
    assert np.all(np.abs(s - ref) <= _sdev_bound(2, ref))
    assert _bits(nb) == _bits((x - m) / s)
    assert _bits(synth.unstandardize(nb, m, s, 1)) == _bits(nb * s + m)


@pytest.mark.gpu
def test_host_entries_stage_large_batches_in_chunks():
    """Two planes of 4099 x 4099 are 269 MB: the host entries stage one plane at a time.  A
    plane's results are the bits of a call on that plane alone, the fill's values are those
    at its indices, and the normalised planes are NumPy's (x - m) / s."""
    H = W = 4099
    assert 2 * H * W * 8 > STAGE_BYTES >= H * W * 8
    rng = np.random.default_rng(8)
    x = np.asfortranarray(rng.standard_normal((H, W, 2)) + 10.0)
    a = np.asfortranarray(x * (rng.random((H, W, 2)) < 1e-4))
    got, gi = synth.nn_fill(a, return_index=True)
    nb, m, s = synth.standardize(x, 2)
    for p in range(2):
        ap = np.asfortranarray(a[:, :, p])
        one, oi = synth.nn_fill(ap, return_index=True)
        assert np.array_equal(one, got[:, :, p]) and np.array_equal(oi, gi[:, :, p]), p
        assert gi[:, :, p].min() >= 0
        assert np.array_equal(got[:, :, p], ap.ravel(order="F")[gi[:, :, p]])
        assert np.array_equal(got[:, :, p][ap != 0], ap[ap != 0])
        nb1, m1, s1 = synth.standardize(np.asfortranarray(x[:, :, p]), 2)
        assert float(m1) == m[p] and float(s1) == s[p], p
        assert np.array_equal(nb1, nb[:, :, p]), p
    assert np.array_equal(nb, (x - m[None, None, :]) / s[None, None, :])
    back = synth.unstandardize(nb, m, s, 2)
    assert np.array_equal(back, nb * s[None, None, :] + m[None, None, :])


# ---- GPU: one driver-shaped case per pipeline --------------------------------------------

def _unit(k, axes):
    return k / np.sqrt((k ** 2).sum(axis=axes, keepdims=True))


@pytest.mark.gpu
def test_demosaicing_preparation_feeds_the_solver():
    """reconstruct_subsampling_hyperspectral.m:38-60 at 36 x 36 x 9: mask, fill, smooth_init
    on CUDA tensors, then the 2-3D solver."""
    import torch
    from ccsc_code_iccv2017_amd import solvers
    a, filled, _, _ = _case("mosaic_36_p3")
    mask = (a != 0).astype(np.float64)
    t = torch.as_tensor(np.ascontiguousarray(a), device="cuda")
    got = synth.smooth_init(synth.nn_fill(t))
    want = synth.smooth_init(torch.as_tensor(np.ascontiguousarray(filled), device="cuda"))
    assert got.is_cuda and _bits(got.cpu().numpy()) == _bits(want.cpu().numpy())
    d = _unit(np.random.default_rng(41).standard_normal((5, 5, 9, 4)), (0, 1, 2))
    z, rec = solvers.admm_solve_conv23D_weighted_sampling(
        a, d, mask, 1000.0, 1.0, 3, 1e-3, None, "none", got.cpu().numpy())
    assert rec.shape == a.shape and np.isfinite(rec).all() and np.isfinite(z).all()


@pytest.mark.gpu
def test_video_preparation_feeds_the_solver_and_is_undone():
    """reconstruct_subsampling_video.m:38-68 at 24 x 20 x 6: blur, standardise per frame,
    smooth_init (15 x 15), the video solver, un-standardise.  The frame means that
    unstandardize restores are the blurred clip's within the mean bound, and the round trip
    of the normalised clip returns the blurred clip within 4 u (|x| + |m|)."""
    from ccsc_code_iccv2017_amd import solvers
    rng = np.random.default_rng(43)
    clip = np.asfortranarray(rng.random((24, 20, 6)))
    psf = np.zeros((3, 3, 3))
    psf[:, :, 1] = rng.uniform(0.5, 1.0, (3, 3))
    psf /= psf.sum()
    b = synth.imfilter(clip, psf, "symmetric")
    nb, m, s = synth.standardize(b, 2)
    assert m.shape == (6,)
    frames = b.reshape((-1, 6), order="F")
    rm, rs = standardize_ref(frames)
    assert np.all(np.abs(m - rm) <= 480 * U * np.abs(frames).mean(axis=0))
    assert np.all(np.abs(s - rs) <= _sdev_bound(480, rs))
    smooth = synth.smooth_init(nb, size=15)
    d = _unit(rng.standard_normal((3, 3, 3, 3)), (0, 1, 2))
    z, Dz = solvers.admm_solve_video_weighted_sampling(
        nb, d, np.ones(b.shape), 1000.0, 0.125, 3, 1e-6, "none", psf, smooth)
    assert Dz.shape == b.shape
    rec = synth.unstandardize(Dz, m, s, 2)
    assert np.isfinite(rec).all() and np.isfinite(z).all()
    assert _bits(rec) == _bits(Dz * s[None, None, :] + m[None, None, :])
    back = synth.unstandardize(nb, m, s, 2)
    assert np.all(np.abs(back - b) <= 4 * U * (np.abs(b) + np.abs(m)[None, None, :]))
