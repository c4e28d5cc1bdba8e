"""GPU: the sessions' codes as a compressed sparse column matrix (Session.codes_sparse,
ccsc_session_codes_count / _fill) on every learner and every z route.

Bit tests: a session is run, ``results(want_z=True)`` gives the dense z, and the triple,
densified, must equal ``np.where(~(np.abs(z) <= eps), z, 0)`` bit for bit for eps in
{0, 0.05 max|z|, 0.25 max|z|, inf}.  Two outer iterations, seed 7, injected d0 / z0.  The
sessions run with verbose 'none', so the 2D z-phases end on the pre-threshold state (and
the 110 grid on the register-line state) and the entry points have to materialise z.

Oracle tests: kept / dropped status against the float64 oracle away from the threshold
(entries with | |z_o| - eps | <= 1e-6 max|z_o| are left out, at most 0.1 % of them may be),
kept values at the project's 1e-7 relative bar for z."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-300)


def densify(triple):
    jc, ir, pr, (M, n) = triple
    assert jc.dtype == np.int64 and ir.dtype == np.int64 and pr.dtype == np.float64
    assert jc.shape == (n + 1,) and jc[0] == 0 and np.all(np.diff(jc) >= 0)
    assert ir.shape == pr.shape == (jc[-1],)
    cols = np.repeat(np.arange(n), np.diff(jc))
    if ir.size:
        assert ir.min() >= 0 and ir.max() < M
        inside = cols[1:] == cols[:-1]
        assert np.all(np.diff(ir)[inside] > 0)            # strictly ascending inside a column
    dense = np.zeros((M, n), order="F")
    dense[ir, cols] = pr
    return dense


def thresholded(z, eps):
    """What the triple must densify to: z's [M, n_local] matrix with the dropped entries 0."""
    zm = np.real(z).reshape(-1, z.shape[-1], order="F")
    with np.errstate(invalid="ignore"):
        return np.where(~(np.abs(zm) <= eps), zm, 0.0)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint64),
                                                 np.ascontiguousarray(b).view(np.uint64))


# name: (variant, sb, views | W, psf, K, n, ni, lambda_prior)
CASES = {
    "dP-11x10": ("dp", (11, 10), 1, 5, 3, 6, 3, 1.0),
    "dZ-K70": ("dz", (12, 12), 1, 5, 70, 16, 8, 1.0),
    "dZ-110-register-line": ("dz", (100, 100), 1, 11, 4, 4, 2, 1.0),
    "dP-54-global-passes": ("dp", (44, 44), 1, 11, 3, 4, 2, 1.0),
    "L3": ("L3", (8, 9, 7), 1, 3, 3, 4, 2, 0.1),       # test_learn_3d_matches_oracle's smallest
    "L4": ("L4", (10, 9), 2, 5, 3, 4, 2, 1.0),         # test_learn_4d_matches_oracle's smallest
    "HS23": ("hs", (10, 9), 3, 5, 4, 3, 0, 1.0),       # test_learn_hs23_matches_oracle's smallest
}


def _inputs(name):
    """(variant code, b, kernel_size, d0, z0, smooth_init, ni, lambda) of a case; the 2D
    cases draw as tests/test_gpu_parity.py::_case does."""
    from ccsc_code_iccv2017_amd import _lib as L
    v, sb, UV, psf, K, n, ni, lam = CASES[name]
    rng = np.random.default_rng(7)
    r = psf // 2
    g = tuple(s + 2 * r for s in sb)
    sm = None
    if v in ("dp", "dz"):
        b = rng.standard_normal(sb + (n,))
        d0 = rng.standard_normal((psf, psf, K))
        z0 = rng.standard_normal(g + (K, ni if v == "dz" else n))
        code, ks = (L.CCSC_DZPAR if v == "dz" else L.CCSC_DPAR), [psf, psf, K]
    elif v == "L3":
        b = rng.standard_normal(sb + (n,))
        d0 = rng.standard_normal((psf, psf, psf, K))
        z0 = rng.standard_normal(g + (K, n))
        code, ks = L.CCSC_L3D, [psf, psf, psf, K]
    elif v == "L4":
        b = rng.standard_normal(sb + (UV, UV, n))
        d0 = rng.standard_normal((psf, psf, UV, UV, K))
        z0 = rng.standard_normal(g + (1, 1, K, n))
        code, ks = L.CCSC_L4D, [psf, psf, UV, UV, K]
    else:
        b = rng.random(sb + (UV, n))
        sm = 0.5 * rng.random(sb + (UV, n))
        d0 = rng.standard_normal((psf, psf, K))
        z0 = rng.standard_normal(g + (K, n))
        code, ks = L.CCSC_HS23, [psf, psf, UV, K]
    return code, b, ks, d0, z0, sm, ni, lam


def _session(name, ctx, verbose="none", shard=None):
    from ccsc_code_iccv2017_amd import learners as E
    code, b, ks, d0, z0, sm, ni, lam = _inputs(name)
    p = E.make_problem(code, b.shape, ks, 1.0, lam, 2, 0.0, verbose, ni=ni or None)
    if shard is not None:
        b, z0 = b[..., shard], (z0 if code == E.L.CCSC_DZPAR else z0[..., shard])
    return E.Session(ctx, p, b, d0, z0, smooth_init=sm)


EPS_OF = {"0": lambda m: 0.0, "0.05max": lambda m: 0.05 * m, "0.25max": lambda m: 0.25 * m,
          "inf": lambda m: np.inf}


@pytest.mark.parametrize("name", list(CASES))
def test_codes_sparse_equals_thresholded_dense_bitwise(gpu_ctx, name):
    s = _session(name, gpu_ctx)
    try:
        s.step(2)
        z = s.results(want_z=True, want_DZ=False)[1]
        m = np.abs(z).max()
        assert np.isfinite(m) and m > 0
        for tag, f in EPS_OF.items():
            eps = f(m)
            t = s.codes_sparse(eps)
            assert t[3] == (z.size // z.shape[-1], z.shape[-1]) == (t[3][0], s.n_local), tag
            want = thresholded(z, eps)
            assert same_bits(densify(t), want), (name, tag)
            assert t[0][-1] == np.count_nonzero(want), tag
            if tag == "inf":
                assert t[0][-1] == 0
            if tag == "0.05max":
                assert 0 < t[0][-1] < z.size                  # the threshold does cut
        # the triple is reproducible, and one column per chunk gives the same bits
        a = s.codes_sparse(0.05 * m)
        os.environ["CCSC_CODES_WS_MB"] = "0"
        try:
            b = s.codes_sparse(0.05 * m)
        finally:
            del os.environ["CCSC_CODES_WS_MB"]
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x.view(np.uint64), y.view(np.uint64))
    finally:
        s.close()


def test_codes_sparse_before_the_first_step_is_the_initial_z(gpu_ctx):
    """No step yet: the codes are the injected z0 (the session's state is natural already)."""
    s = _session("dP-11x10", gpu_ctx)
    try:
        z0 = _inputs("dP-11x10")[4]
        assert same_bits(densify(s.codes_sparse(1.0)), thresholded(z0, 1.0))
    finally:
        s.close()


def test_fill_capacity_below_nnz_names_the_count_and_writes_nothing(gpu_ctx):
    from ccsc_code_iccv2017_amd import _lib as L
    s = _session("dP-11x10", gpu_ctx)
    try:
        s.step(1)
        nnz = int(s.codes_sparse(0.0)[0][-1])
        ir = np.full(nnz, -7, dtype=np.int64)
        pr = np.full(nnz, -7.25)
        eb = L.errbuf()
        rc = L.lib().ccsc_session_codes_fill(s.ptr, 0.0, L.lptr(ir), L.dptr(pr), nnz - 1, eb,
                                             len(eb))
        assert rc == L.CCSC_E_INVALID and str(nnz) in eb.value.decode(), eb.value
        assert np.all(ir == -7) and np.all(pr == -7.25)
    finally:
        s.close()


_oracle_cache = {}


def _oracle_z(name):
    if name not in _oracle_cache:
        from oracle import ccsc_oracle as O
        code, b, ks, d0, z0, sm, ni, lam = _inputs(name)
        fn = O.learn_2d_dzparallel if CASES[name][0] == "dz" else O.learn_2d_dparallel
        z = fn(b, ks, 1.0, lam, 2, 0.0, "none", {"d": d0, "z": z0}, ni=ni)[1]
        z.setflags(write=False)
        _oracle_cache[name] = z
    return _oracle_cache[name]


@pytest.mark.parametrize("frac", [0.05, 0.25])
@pytest.mark.parametrize("name", ["dP-11x10", "dZ-K70"])
def test_codes_sparse_matches_oracle_away_from_the_threshold(gpu_ctx, name, frac):
    z_o = _oracle_z(name)
    zo = z_o.reshape(-1, z_o.shape[-1], order="F")
    m = np.abs(zo).max()
    eps = frac * m
    s = _session(name, gpu_ctx)
    try:
        s.step(2)
        jc, ir, pr, shape = t = s.codes_sparse(eps)
    finally:
        s.close()
    assert shape == zo.shape
    dense = densify(t)
    kept_e = np.zeros(shape, dtype=bool)
    kept_e[ir, np.repeat(np.arange(shape[1]), np.diff(jc))] = True
    kept_o = ~(np.abs(zo) <= eps)
    judged = np.abs(np.abs(zo) - eps) > 1e-6 * m
    left_out = 1.0 - judged.mean()
    print(f"{name} eps = {frac} max|z_o|: kept {kept_o.mean():.4f} of the entries, "
          f"{(~judged).sum()} of {judged.size} left out")
    assert left_out <= 1e-3
    assert np.array_equal(kept_e[judged], kept_o[judged])
    both = judged & kept_o
    assert both.any()
    assert _rel(dense[both], zo[both]) < 1e-7


def test_codes_sparse_leaves_the_state_results_leaves(gpu_ctx):
    """step, dense z, step against step, sparse codes, step on the register-line route: the
    filters and the objective afterwards are the same bits."""
    out = []
    for sparse in (False, True):
        s = _session("dZ-110-register-line", gpu_ctx)
        try:
            s.step(1)
            if sparse:
                s.codes_sparse(0.1)
            else:
                s.results(want_z=True, want_DZ=False)
            s.step(1)
            out.append((s.results(want_z=False, want_DZ=False)[0], s.objective()))
        finally:
            s.close()
    assert same_bits(out[0][0], out[1][0])
    assert np.float64(out[0][1]).tobytes() == np.float64(out[1][1]).tobytes()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


RANK_CASE, RANK_EPS = "dP-11x10", 0.1


def _rank_worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ccsc_code_iccv2017_amd import learners as E

    def host_comm(op, arr):
        t = torch.from_numpy(arr)
        if op == 0:
            dist.all_reduce(t)
        else:
            dist.broadcast(t, src=0)

    ctx = E.Context(0, rank, world, host_comm=host_comm)
    code, b, ks, d0, z0, sm, ni, lam = _inputs(RANK_CASE)
    p = E.make_problem(code, b.shape, ks, 1.0, lam, 2, 0.0, "none", ni=ni)
    b0, nb = E.shard(E.resolve(p), rank, world)
    s = _session(RANK_CASE, ctx, shard=slice(b0 * ni, (b0 + nb) * ni))
    s.step(2)
    jc, ir, pr, shape = s.codes_sparse(RANK_EPS)
    z = s.results(want_z=True, want_DZ=False)[1]
    np.savez(os.path.join(out_dir, f"r{rank}.npz"), jc=jc, ir=ir, pr=pr, shape=shape, z=z,
             first=b0 * ni, count=nb * ni)
    s.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


def test_two_rank_triples_concatenate_to_the_one_rank_triple(tmp_path, gpu_ctx):
    """Two ranks on the host transport (one block each): every rank's triple covers its
    shard, and the two, with the second's jc shifted, are the one-rank triple bit for bit."""
    import torch.multiprocessing as mp
    mp.start_processes(_rank_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True,
                       start_method="spawn")
    parts = [np.load(tmp_path / f"r{r}.npz") for r in range(2)]
    s = _session(RANK_CASE, gpu_ctx)
    try:
        s.step(2)
        jc1, ir1, pr1, shape1 = s.codes_sparse(RANK_EPS)
    finally:
        s.close()
    assert [int(q["first"]) for q in parts] == [0, 3] and [int(q["count"]) for q in parts] == [3, 3]
    for q in parts:   # a rank's triple is its own shard's dense z, thresholded
        t = (q["jc"], q["ir"], q["pr"], tuple(int(v) for v in q["shape"]))
        assert t[3] == (shape1[0], int(q["count"]))
        assert same_bits(densify(t), thresholded(q["z"], RANK_EPS))
    jc = np.concatenate([parts[0]["jc"], parts[0]["jc"][-1] + parts[1]["jc"][1:]])
    ir = np.concatenate([q["ir"] for q in parts])
    pr = np.concatenate([q["pr"] for q in parts])
    assert np.array_equal(jc, jc1) and np.array_equal(ir, ir1)
    assert np.array_equal(pr.view(np.uint64), pr1.view(np.uint64))


def test_learner_keyword_sparse_z_returns_the_session_triple(gpu_ctx):
    from ccsc_code_iccv2017_amd import learners as E
    name = "dZ-K70"
    code, b, ks, d0, z0, sm, ni, lam = _inputs(name)
    args = (b, ks, 1.0, lam, 2, 0.0, "brief", {"d": d0, "z": z0})
    d1, z1, DZ1, it1 = E.admm_learn_conv2D_large_dzParallel(*args, ni=ni, ctx=gpu_ctx)
    eps = 0.05 * np.abs(z1).max()
    d2, z2, DZ2, it2 = E.admm_learn_conv2D_large_dzParallel(*args, ni=ni, ctx=gpu_ctx,
                                                            sparse_z=eps)
    s = _session(name, gpu_ctx, verbose="brief")
    try:
        s.step(2)
        want = s.codes_sparse(eps)
        sp = None
        try:
            import scipy.sparse  # noqa: F401
        except ImportError:
            pass
        else:
            sp = s.codes_sparse(eps, as_scipy=True)
    finally:
        s.close()
    assert isinstance(z2, tuple) and z2[3] == want[3] == (z1.size // z1.shape[-1], z1.shape[-1])
    for x, y in zip(z2[:3], want[:3]):
        assert x.dtype == y.dtype and np.array_equal(x.view(np.uint64), y.view(np.uint64))
    assert same_bits(densify(z2), thresholded(z1, eps))
    assert same_bits(d2, d1) and same_bits(DZ2, DZ1)
    for k in ("obj_vals_d", "obj_vals_z"):
        assert np.array_equal(it2[k], it1[k])
    for k in ("n_d", "n_z", "d_diff", "z_diff", "obj_d", "obj_z"):
        assert np.array_equal(it2["trace"][k], it1["trace"][k], equal_nan=True), k
    if sp is not None:
        assert sp.shape == want[3] and sp.nnz == want[0][-1]
        assert same_bits(np.asfortranarray(sp.toarray()), densify(want))


@pytest.mark.parametrize("name", ["L3", "L4", "HS23", "dP-11x10"])
def test_every_learner_takes_sparse_z(gpu_ctx, name):
    """The other four wrappers: the z_res position holds the triple of the dense run's z."""
    from ccsc_code_iccv2017_amd import learners as E
    code, b, ks, d0, z0, sm, ni, lam = _inputs(name)
    fn = {"L3": E.admm_learn_conv3D_large, "L4": E.admm_learn_conv4D_lightfield,
          "HS23": E.admm_learn, "dP-11x10": E.admm_learn_conv2D_large_dParallel}[name]
    args = (b, ks, 1.0, lam, 2, 0.0, "none", {"d": d0, "z": z0})
    kw = dict(ctx=gpu_ctx)
    if name == "HS23":
        kw["smooth_init"] = sm
    else:
        kw["ni"] = ni
    dense = fn(*args, **kw)
    eps = 0.05 * np.abs(dense[1]).max()
    sparse = fn(*args, sparse_z=eps, **kw)
    assert same_bits(sparse[0], dense[0]) and same_bits(sparse[2], dense[2])
    assert isinstance(sparse[1], tuple)
    assert same_bits(densify(sparse[1]), thresholded(dense[1], eps))


def test_sparse_z_on_a_device_list_is_rejected(gpu_ctx):
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import learners as E
    code, b, ks, d0, z0, sm, ni, lam = _inputs("dP-11x10")
    mctx = E.Context.multi([0, 0])
    try:
        with pytest.raises(L.CCSCError) as ei:
            E.admm_learn_conv2D_large_dParallel(b, ks, 1.0, lam, 1, 0.0, "none",
                                                {"d": d0, "z": z0}, ni=ni, ctx=mctx, sparse_z=0.1)
        assert "one-device context" in str(ei.value)
    finally:
        mctx.close()
