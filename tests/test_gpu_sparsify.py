"""GPU: ccsc_sparsify* (csrc/codes.hip) against NumPy, bit for bit.

An entry is kept iff ``not (abs(a) <= eps)``; the expected triple is NumPy's own
``~(np.abs(a) <= eps)`` walked column by column.  Shapes: M around the 64-lane step, the
512-row wave run and the 2048-row tile (1, 63, 64, 65, 210, 4097 = two tiles and one row);
n = 1, 3, 70; one case of more than 2^16 one-tile columns, whose scan spans workgroups.
Offsets past 2^32 cannot be reached at test size: tests/test_codes_abi.py checks their
arithmetic on the host."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EPS = 0.5
PATTERNS = ["zeros", "full", "alternate", "first", "last", "special", "random"]


def _column(kind, M, rng):
    v = rng.standard_normal(M)
    small = 0.4 * EPS * rng.random(M)                     # dropped
    big = EPS * (1.5 + rng.random(M)) * rng.choice([-1.0, 1.0], M)   # kept
    if kind == "zeros":
        return np.zeros(M)
    if kind == "full":
        return big
    if kind == "alternate":
        return np.where(np.arange(M) % 2 == 0, big, small)
    if kind == "first":
        small[0] = big[0]
        return small
    if kind == "last":
        small[M - 1] = big[M - 1]
        return small
    if kind == "special":
        # NaN (kept), +-inf (kept), +-eps exactly (dropped), eps's neighbours, signed zeros
        s = [np.nan, np.inf, -np.inf, EPS, -EPS, np.nextafter(EPS, 1), -np.nextafter(EPS, 1),
             np.nextafter(EPS, 0), 0.0, -0.0, -np.nan]
        for i in range(M):
            v[i] = s[i % len(s)] if i % 3 != 2 or M < 4 else v[i]
        return v
    v[rng.integers(M)] = EPS                              # |entry| == eps: dropped
    return v


def _matrix(M, n, shift, seed):
    rng = np.random.default_rng(seed)
    cols = [_column(PATTERNS[(j + shift) % len(PATTERNS)], M, rng) for j in range(n)]
    return np.asfortranarray(np.stack(cols, axis=1))


def ref_csc(a, eps):
    """NumPy's triple: jc, ir, pr of ~(abs(a) <= eps), columns in order, rows ascending."""
    with np.errstate(invalid="ignore"):
        keep = ~(np.abs(a) <= eps)
    jc = np.concatenate([[0], np.cumsum(keep.sum(axis=0))]).astype(np.int64)
    cols, rows = np.nonzero(keep.T)
    return jc, rows.astype(np.int64), a[rows, cols].astype(np.float64)


def assert_same_bits(got, want):
    for g, w, name in zip(got[:3], want[:3], ("jc", "ir", "pr")):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (name, g.dtype, g.shape, w.shape)
        assert np.array_equal(g.view(np.uint64), w.view(np.uint64)), name


@pytest.mark.parametrize("n", [1, 3, 70])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 210, 4097])
def test_sparsify_matches_numpy_bitwise(gpu_ctx, monkeypatch, M, n):
    """Every column pattern at every shape; then the same input one column per chunk
    (CCSC_CODES_WS_MB=0) and every column sparsified alone: identical bits."""
    from ccsc_code_iccv2017_amd.learners import sparsify
    for shift in range(0, len(PATTERNS), n):
        a = _matrix(M, n, shift, seed=1000 * M + n)
        want = ref_csc(a, EPS)
        got = sparsify(a, EPS, ctx=gpu_ctx)
        assert got[3] == (M, n)
        assert_same_bits(got, want)
        monkeypatch.setenv("CCSC_CODES_WS_MB", "0")
        assert_same_bits(sparsify(a, EPS, ctx=gpu_ctx), want)
        monkeypatch.delenv("CCSC_CODES_WS_MB")
        for j in sorted({0, n // 2, n - 1}):
            jc, ir, pr, _ = sparsify(a[:, j:j + 1], EPS, ctx=gpu_ctx)
            sl = slice(want[0][j], want[0][j + 1])
            assert_same_bits((jc, ir, pr), (want[0][j:j + 2] - want[0][j], want[1][sl], want[2][sl]))


@pytest.mark.parametrize("eps", [0.0, EPS, np.inf])
def test_sparsify_threshold_edges(gpu_ctx, eps):
    """eps = 0 keeps every nonzero (not -0.0), +inf keeps only the NaNs, and an entry whose
    magnitude equals eps is dropped."""
    from ccsc_code_iccv2017_amd.learners import sparsify
    a = _matrix(210, 7, 0, seed=5)
    jc, ir, pr, _ = got = sparsify(a, eps, ctx=gpu_ctx)
    assert_same_bits(got, ref_csc(a, eps))
    if eps == 0.0:
        assert jc[-1] == np.count_nonzero(a)             # NaN != 0 counts, -0.0 does not
    elif np.isinf(eps):
        assert jc[-1] == np.isnan(a).sum() > 0 and np.isnan(pr).all()
    else:
        assert not np.any(np.abs(pr) == eps) and np.any(np.abs(a) == eps)


def test_sparsify_many_columns_scan_crosses_workgroups(gpu_ctx):
    """More than 2^16 columns of M = 4: one tile each, so the scan of the tile counts runs
    over 35 workgroups and the column offsets come from all of them."""
    from ccsc_code_iccv2017_amd.learners import sparsify
    rng = np.random.default_rng(65537)
    a = np.asfortranarray(rng.standard_normal((4, 70001)))
    a[:, 2048 * 3 - 1: 2048 * 3 + 2] = 7.0                # kept runs across a scan boundary
    a[:, 40000:44100] = 0.0                               # two empty scan workgroups
    got = sparsify(a, EPS, ctx=gpu_ctx)
    assert_same_bits(got, ref_csc(a, EPS))


def test_sparsify_more_tiles_than_one_launch_takes(gpu_ctx):
    """2^22 + 5 one-row columns: more tiles than the 2^22 workgroups a launch is given, so the
    count, the scan's last pass, the column offsets and the scatter each go in two launches
    with a workgroup offset (34 MB of input; the smallest shape that reaches that path)."""
    from ccsc_code_iccv2017_amd.learners import sparsify
    rng = np.random.default_rng(4194309)
    a = np.asfortranarray(rng.standard_normal((1, (1 << 22) + 5)))
    a[0, -7:] = [3.0, 0.0, -3.0, np.nan, EPS, 2.0, -0.1]      # both sides of the launch boundary
    got = sparsify(a, EPS, ctx=gpu_ctx)
    assert_same_bits(got, ref_csc(a, EPS))


@pytest.mark.parametrize("M,n", [(65, 70), (4097, 3)])
def test_sparsify_dev_equals_host(gpu_ctx, M, n):
    """A CUDA tensor goes through the _dev forms and stays on the device; same bits."""
    import torch
    from ccsc_code_iccv2017_amd.learners import sparsify
    a = _matrix(M, n, 2, seed=77)
    host = sparsify(a, EPS, ctx=gpu_ctx)
    t = torch.from_numpy(a).cuda()
    jc, ir, pr, shape = sparsify(t, EPS, ctx=gpu_ctx)
    assert jc.is_cuda and ir.is_cuda and pr.is_cuda and shape == (M, n)
    assert (jc.dtype, ir.dtype, pr.dtype) == (torch.int64, torch.int64, torch.float64)
    assert_same_bits((jc.cpu().numpy(), ir.cpu().numpy(), pr.cpu().numpy()), host)
    assert_same_bits(host, ref_csc(a, EPS))


@pytest.mark.parametrize("dev", [False, True])
def test_capacity_below_nnz_fails_and_writes_nothing(gpu_ctx, dev):
    import torch
    from ccsc_code_iccv2017_amd import _lib as L
    a = _matrix(210, 3, 1, seed=9)
    nnz = int(ref_csc(a, EPS)[0][-1])
    assert nnz > 1
    eb = L.errbuf()
    if dev:
        t = torch.from_numpy(a).cuda().t().contiguous()
        ir = torch.full((nnz,), -7, dtype=torch.int64, device="cuda")
        pr = torch.full((nnz,), -7.25, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        rc = L.lib().ccsc_sparsify_fill_dev(gpu_ctx.ptr, t.data_ptr(), 210, 3, EPS, ir.data_ptr(),
                                            pr.data_ptr(), nnz - 1, eb, len(eb))
        ir, pr = ir.cpu().numpy(), pr.cpu().numpy()
    else:
        ir = np.full(nnz, -7, dtype=np.int64)
        pr = np.full(nnz, -7.25)
        rc = L.lib().ccsc_sparsify_fill(gpu_ctx.ptr, L.dptr(a), 210, 3, EPS, L.lptr(ir),
                                        L.dptr(pr), nnz - 1, eb, len(eb))
    assert rc == L.CCSC_E_INVALID and str(nnz) in eb.value.decode(), eb.value
    assert np.all(ir == -7) and np.all(pr == -7.25)
    # the same buffers at capacity nnz succeed
    if not dev:
        eb = L.errbuf()
        L.check(L.lib().ccsc_sparsify_fill(gpu_ctx.ptr, L.dptr(a), 210, 3, EPS, L.lptr(ir),
                                           L.dptr(pr), nnz, eb, len(eb)), eb)
        assert_same_bits((ir, pr), ref_csc(a, EPS)[1:])


def test_sparsify_rejects_a_device_list_context(gpu_ctx):
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import learners as E
    mctx = E.Context.multi([0, 0])
    try:
        with pytest.raises(L.CCSCError) as ei:
            E.sparsify(np.ones((4, 2)), 0.5, ctx=mctx)
        assert ei.value.code == L.CCSC_E_UNSUPPORTED and "one-device context" in str(ei.value)
    finally:
        mctx.close()
