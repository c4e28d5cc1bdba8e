"""GPU, 2 ranks sharing the box's one MI355X: the engine's sharded path
(contiguous block shards, owner-of-block-1 logic, per-d-iteration consensus
all-reduce, per-outer broadcast of block 1's filter spectrum, tol norms)
through the C-ABI, with the exchanges carried by the host-staged transport
over gloo.  Must equal the single-rank engine and the oracle.  (8-GPU RCCL runs
are the driver's; RCCL differs only in the transport calls.)

Every learner is here: the 2D learners and the 2-3D learner from explicit inits, the 3D and
4D learners sharded 2 + 1 blocks (device list and sessions, LDS-resident and global-pass
grids), and every learner from the device RNG (init = None), where the sharded draw must be
the one-rank draw (tests/rng_ref.py restates the stream).  The spawned 3D / 4D and
device-RNG cases share one process pair (fixture pair_dir).  Not covered: launch_randn's
chunk boundary at 2^30 elements, which needs more than 8.6 GB of draws on the host to
observe; by reading, its `out + c0` and `offset + c0` advance together."""
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _case(variant, big=False):
    rng = np.random.default_rng(99)
    ni, N, psf, K = 2, 3, 5, 3          # 3 blocks over 2 ranks: 2 + 1
    # big: 150 x 149 patches (a 154 x 153 slice past one CU's LDS: the global-pass path)
    sx, sy = (150, 149) if big else (12, 11)
    b = rng.standard_normal((sx, sy, ni * N))
    d0 = rng.standard_normal((psf, psf, K))
    X, Y = sx + 4, sy + 4
    z0 = rng.standard_normal((X, Y, K, ni if variant == "dz" else ni * N))
    return b, d0, z0, ni, N, [psf, psf, K]


def _worker(rank, world, port, out_dir, variant, tol, big):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ccsc_code_iccv2017_amd import learners as E

    def host_comm(op, arr):
        t = torch.from_numpy(arr)        # shares memory with the engine's staging buffer
        if op == 0:
            dist.all_reduce(t)
        else:
            dist.broadcast(t, src=0)

    b, d0, z0, ni, N, ks = _case(variant, big)
    v = E.L.CCSC_DZPAR if variant == "dz" else E.L.CCSC_DPAR
    p = E.make_problem(v, b.shape, ks, 1.0, 1.0, 2, tol, "brief", ni=ni, trace_objective=True)
    ctx = E.Context(0, rank, world, host_comm=host_comm)
    b0, nb = E.shard(E.resolve(p), rank, world)
    bl = b[:, :, b0 * ni:(b0 + nb) * ni]
    zl = z0 if variant == "dz" else z0[..., b0 * ni:(b0 + nb) * ni]
    s = E.Session(ctx, p, bl, d0, zl)
    s.step(2)
    d_res, z_res, DZ, _ = s.results()
    it = s.iterlog()
    np.savez(os.path.join(out_dir, f"{variant}_r{rank}.npz"), d=d_res, z=z_res, DZ=DZ,
             oz=it["trace"]["obj_z"], od=it["trace"]["obj_d"], zd=it["trace"]["z_diff"])
    s.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("variant,tol,big", [("dz", 0.0, False), ("dp", 1e-12, False),
                                             # global-pass slices: the sharded
                                             # support / d-norm / objective exchanges and the
                                             # session's state handling on that path
                                             ("dz", 0.0, True), ("dp", 1e-3, True)])
def test_two_ranks_equal_one_rank(tmp_path, gpu_ctx, variant, tol, big):
    """Session.step over two ranks (the bench's path) equals the oracle."""
    import torch.multiprocessing as mp
    from ccsc_code_iccv2017_amd import learners as E
    from oracle import ccsc_oracle as O

    mp.start_processes(_worker, args=(2, _free_port(), str(tmp_path), variant, tol, big),
                       nprocs=2, join=True, start_method="spawn")
    parts = [np.load(tmp_path / f"{variant}_r{r}.npz") for r in range(2)]
    b, d0, z0, ni, N, ks = _case(variant, big)
    fn = O.learn_2d_dzparallel if variant == "dz" else O.learn_2d_dparallel
    d_o, z_o, DZ_o, it_o, tr_o = fn(b, ks, 1.0, 1.0, 2, tol, "brief", {"d": d0, "z": z0}, ni=ni,
                                    trace_objective=True)
    z = np.concatenate([q["z"] for q in parts], axis=3)
    DZ = np.concatenate([q["DZ"] for q in parts], axis=3)
    for q in parts:   # every rank returns block 1's filters and the global objectives
        np.testing.assert_allclose(q["d"], d_o, rtol=0, atol=1e-9 * np.abs(d_o).max())
        np.testing.assert_allclose(q["oz"], np.array(tr_o["obj_z"]), rtol=1e-9)
        np.testing.assert_allclose(q["od"], np.array(tr_o["obj_d"]), rtol=1e-9)
    np.testing.assert_allclose(z, z_o, rtol=0, atol=1e-9 * np.abs(z_o).max())
    np.testing.assert_allclose(DZ, DZ_o, rtol=0, atol=1e-9 * np.abs(DZ_o).max())
    if tol > 0:
        np.testing.assert_allclose(parts[0]["zd"], np.array(tr_o["z_diff"]), rtol=1e-6)


@pytest.mark.parametrize("variant,tol,nblk", [("dz", 0.0, 3), ("dp", 0.0, 2), ("dz", 1e-12, 2)])
def test_multi_device_context_equals_one_device(gpu_ctx, variant, tol, nblk):
    """ccsc_create_multi({0, 0}) + one ccsc_learn over the whole problem (the MEX path of
    one MATLAB call over several GPUs; a repeated device exchanges through host memory,
    distinct devices through RCCL) gives the one-device result: blocks sharded by
    ccsc_shard, outputs written back at each rank's patch offset, iterlog from rank 0."""
    from ccsc_code_iccv2017_amd import learners as E
    rng = np.random.default_rng(31)
    ni, K, psf = 2, 3, 5
    n = ni * nblk
    b = rng.standard_normal((12, 11, n))
    d0 = rng.standard_normal((psf, psf, K))
    z0 = rng.standard_normal((16, 15, K, ni if variant == "dz" else n))
    fn = (E.admm_learn_conv2D_large_dzParallel if variant == "dz"
          else E.admm_learn_conv2D_large_dParallel)
    args = (b, [psf, psf, K], 1.0, 1.0, 2, tol, "brief", {"d": d0, "z": z0})
    d1, z1, DZ1, it1 = fn(*args, ni=ni, ctx=gpu_ctx)
    mctx = E.Context.multi([0, 0])
    try:
        d2, z2, DZ2, it2 = fn(*args, ni=ni, ctx=mctx)
    finally:
        mctx.close()
    np.testing.assert_allclose(d2, d1, rtol=0, atol=1e-10 * np.abs(d1).max())
    np.testing.assert_allclose(z2, z1, rtol=0, atol=1e-10 * np.abs(z1).max())
    np.testing.assert_allclose(DZ2, DZ1, rtol=0, atol=1e-10 * np.abs(DZ1).max())
    np.testing.assert_allclose(it2["obj_vals_z"], it1["obj_vals_z"], rtol=1e-10)
    if tol > 0:
        np.testing.assert_array_equal(it2["trace"]["n_z"], it1["trace"]["n_z"])


def test_multi_device_context_rejects_sessions(gpu_ctx):
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import learners as E
    mctx = E.Context.multi([0, 0])
    try:
        p = E.make_problem(L.CCSC_DZPAR, (12, 11, 4), [5, 5, 3], 1.0, 1.0, 1, 0.0, "none", ni=2)
        with pytest.raises(L.CCSCError) as ei:
            E.Session(mctx, p, np.zeros((12, 11, 4)))
        assert "one-device context" in str(ei.value)
    finally:
        mctx.close()


def _small_dz(seed=31, nblk=3):
    rng = np.random.default_rng(seed)
    ni, K, psf = 2, 3, 5
    n = ni * nblk
    b = rng.standard_normal((12, 11, n))
    d0 = rng.standard_normal((psf, psf, K))
    z0 = rng.standard_normal((16, 15, K, ni))
    return (b, [psf, psf, K], 1.0, 1.0, 3, 0.0, "brief", {"d": d0, "z": z0}), ni


@pytest.mark.parametrize("fail", ["1:1", "0:0", "1:0"])
def test_failing_rank_aborts_group_and_context_recovers(gpu_ctx, monkeypatch, fail):
    """One rank of a multi-device learn fails (test fault injection, CCSC_TEST_FAIL_RANK
    = rank:outer) while the other is blocked in its next exchange: the call returns that
    rank's error (no hang, no crash), and the SAME context then learns again and
    matches the one-device result -- the MEX keeps its context cached across calls."""
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import learners as E
    args, ni = _small_dz()
    d1, z1, DZ1, it1 = E.admm_learn_conv2D_large_dzParallel(*args, ni=ni, ctx=gpu_ctx)
    mctx = E.Context.multi([0, 0])
    try:
        assert mctx.comm_ranks() == (2, "host")
        monkeypatch.setenv("CCSC_TEST_FAIL_RANK", fail)
        with pytest.raises(L.CCSCError) as ei:
            E.admm_learn_conv2D_large_dzParallel(*args, ni=ni, ctx=mctx)
        assert "injected fault" in str(ei.value) and f"rank {fail.split(':')[0]}" in str(ei.value)
        monkeypatch.delenv("CCSC_TEST_FAIL_RANK")
        d2, z2, DZ2, it2 = E.admm_learn_conv2D_large_dzParallel(*args, ni=ni, ctx=mctx)
    finally:
        mctx.close()
    np.testing.assert_allclose(d2, d1, rtol=0, atol=1e-10 * np.abs(d1).max())
    np.testing.assert_allclose(z2, z1, rtol=0, atol=1e-10 * np.abs(z1).max())
    np.testing.assert_allclose(it2["obj_vals_z"], it1["obj_vals_z"], rtol=1e-10)


@pytest.mark.parametrize("variant", ["dz", "dp"])
def test_rccl_self_group_executes_and_recovers(gpu_ctx, monkeypatch, variant):
    """The RCCL transport on a one-GPU box: a one-device multi context
    under the test hook CCSC_TEST_RCCL_SELF=1 carries a 1-rank RCCL communicator created
    non-blocking (ncclCommInitRankConfig), and every consensus exchange goes through
    collective(): ncclAllReduce per d-iteration, ncclBroadcast per outer iteration
    (dP:114-121, :143), each polled by wait_comm.  A 1-rank all-reduce and broadcast are
    identities, so the learn must equal the transport-free one bit for bit.  Then an injected
    failure aborts the communicator (abort_group -> ncclCommAbort) and the same context
    re-creates it (reset_group) and learns the same result again."""
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import learners as E
    args, ni = _small_dz(nblk=3)
    fn = (E.admm_learn_conv2D_large_dzParallel if variant == "dz"
          else E.admm_learn_conv2D_large_dParallel)
    if variant == "dp":
        b, ks, lr, lp, mi, tol, vb, init = args
        rng = np.random.default_rng(5)
        init = {"d": init["d"], "z": rng.standard_normal((16, 15, ks[2], b.shape[2]))}
        args = (b, ks, lr, lp, mi, tol, vb, init)
    d1, z1, DZ1, it1 = fn(*args, ni=ni, ctx=gpu_ctx)
    monkeypatch.setenv("CCSC_TEST_RCCL_SELF", "1")
    mctx = E.Context.multi([0])
    monkeypatch.delenv("CCSC_TEST_RCCL_SELF")
    try:
        assert mctx.comm_ranks() == (1, "rccl")
        d2, z2, DZ2, it2 = fn(*args, ni=ni, ctx=mctx)
        np.testing.assert_array_equal(d2, d1)
        np.testing.assert_array_equal(z2, z1)
        np.testing.assert_array_equal(DZ2, DZ1)
        np.testing.assert_array_equal(it2["obj_vals_z"], it1["obj_vals_z"])
        monkeypatch.setenv("CCSC_TEST_FAIL_RANK", "0:1")
        with pytest.raises(L.CCSCError) as ei:
            fn(*args, ni=ni, ctx=mctx)
        assert "injected fault" in str(ei.value)
        monkeypatch.delenv("CCSC_TEST_FAIL_RANK")
        with pytest.raises(L.CCSCError):
            mctx.comm_ranks()                 # aborted until the next learn re-creates it
        d3, _, _, it3 = fn(*args, ni=ni, ctx=mctx)
        assert mctx.comm_ranks() == (1, "rccl")
        np.testing.assert_array_equal(d3, d1)
        np.testing.assert_array_equal(it3["obj_vals_z"], it1["obj_vals_z"])
    finally:
        mctx.close()


def test_one_rank_context_reports_no_transport(gpu_ctx):
    assert gpu_ctx.comm_ranks() == (1, "none")


def _visible_gpus():
    import torch
    return torch.cuda.device_count()


@pytest.mark.skipif("_visible_gpus() < 2", reason="needs >= 2 GPUs (runs on the driver's 8-GPU node)")
def test_distinct_devices_over_rccl_equal_one_device(gpu_ctx):
    """ccsc_create_multi over distinct GPUs: ncclCommInitAll, RCCL all-reduce per
    d-iteration and broadcast per outer iteration (dP:114-121, :143) -- the MATLAB
    drop-in over a node.  ncclCommCount must report every device; the result equals
    the one-device learn; an injected failure on the last rank aborts the
    communicators and the context recovers with fresh ones."""
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import learners as E
    ndev = min(_visible_gpus(), 8)
    args, ni = _small_dz(nblk=ndev + 1)
    d1, z1, DZ1, it1 = E.admm_learn_conv2D_large_dzParallel(*args, ni=ni, ctx=gpu_ctx)
    mctx = E.Context.multi(list(range(ndev)))
    try:
        assert mctx.comm_ranks() == (ndev, "rccl")
        d2, z2, DZ2, it2 = E.admm_learn_conv2D_large_dzParallel(*args, ni=ni, ctx=mctx)
        np.testing.assert_allclose(d2, d1, rtol=0, atol=1e-10 * np.abs(d1).max())
        np.testing.assert_allclose(z2, z1, rtol=0, atol=1e-10 * np.abs(z1).max())
        np.testing.assert_allclose(DZ2, DZ1, rtol=0, atol=1e-10 * np.abs(DZ1).max())
        np.testing.assert_allclose(it2["obj_vals_z"], it1["obj_vals_z"], rtol=1e-10)
        os.environ["CCSC_TEST_FAIL_RANK"] = f"{ndev - 1}:1"
        try:
            with pytest.raises(L.CCSCError) as ei:
                E.admm_learn_conv2D_large_dzParallel(*args, ni=ni, ctx=mctx)
            assert "injected fault" in str(ei.value)
        finally:
            del os.environ["CCSC_TEST_FAIL_RANK"]
        d3, _, _, _ = E.admm_learn_conv2D_large_dzParallel(*args, ni=ni, ctx=mctx)
        assert mctx.comm_ranks() == (ndev, "rccl")
        np.testing.assert_allclose(d3, d1, rtol=0, atol=1e-10 * np.abs(d1).max())
    finally:
        mctx.close()


def _hs_case():
    rng = np.random.default_rng(77)
    sb, W, psf, K, n = (12, 11), 3, 5, 4, 5      # 5 images over 2 ranks: 3 + 2
    r = psf // 2
    b = rng.random(sb + (W, n))
    sm = 0.5 * rng.random(sb + (W, n))
    init = {"d": rng.standard_normal((psf, psf, K)),
            "z": rng.standard_normal((sb[0] + 2 * r, sb[1] + 2 * r, K, n))}
    return b, sm, init, [psf, psf, W, K]


def _hs_worker(rank, world, port, out_dir, K):
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

    b, sm, init, ks = _hs_case()
    ks = ks[:3] + [K]
    d0 = init["d"] if K == 4 else np.random.default_rng(5).standard_normal((ks[0], ks[1], K))
    z0 = init["z"] if K == 4 else np.random.default_rng(6).standard_normal(init["z"].shape[:2] + (K, b.shape[-1]))
    p = E.make_problem(E.L.CCSC_HS23, b.shape, ks, 1.0, 0.2, 3, 0.0, "brief")
    ctx = E.Context(0, rank, world, host_comm=host_comm)
    i0, ni = E.shard(E.resolve(p), rank, world)
    s = E.Session(ctx, p, b[..., i0:i0 + ni], d0, z0[..., i0:i0 + ni], smooth_init=sm[..., i0:i0 + ni])
    done = False
    while s.outer < 3 and not done:
        done = s.step(1)
    d_res, z_res, DZ, obj = s.results(want_obj=True)
    it = s.iterlog()
    np.savez(os.path.join(out_dir, f"hs_r{rank}.npz"), d=d_res, z=z_res, DZ=DZ, obj=obj,
             oz=it["trace"]["obj_z"], od=it["trace"]["obj_d"], i0=i0, ni=ni)
    s.close()
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("K", [4, 100])
def test_hs23_two_ranks_equal_oracle(tmp_path, gpu_ctx, K):
    """The 2-3D learner over two ranks (VERDICT r05 missing item 5; L23's d-solve couples every
    image per frequency, admm_learn.m:289-295): images sharded 3 + 2, each rank's Gram (on the
    matrix cores, gramchol_big.hip) and right-hand sides Z^H xi1 summed over the ranks, the
    objective's sums and max(b) reduced -- equals the oracle on the whole problem."""
    import torch.multiprocessing as mp
    from oracle import ccsc_oracle as O

    mp.start_processes(_hs_worker, args=(2, _free_port(), str(tmp_path), K), nprocs=2, join=True,
                       start_method="spawn")
    parts = [np.load(tmp_path / f"hs_r{r}.npz") for r in range(2)]
    b, sm, init, ks = _hs_case()
    ks = ks[:3] + [K]
    if K != 4:
        init = {"d": np.random.default_rng(5).standard_normal((ks[0], ks[1], K)),
                "z": np.random.default_rng(6).standard_normal(init["z"].shape[:2] + (K, b.shape[-1]))}
    d_o, z_o, Dz_o, obj_o, tr_o = O.learn_hs23(b, ks, 1.0, 0.2, 3, 0.0, "brief", init, sm)
    assert [int(q["ni"]) for q in parts] == [3, 2]
    z = np.concatenate([q["z"] for q in parts], axis=3)
    Dz = np.concatenate([q["DZ"] for q in parts], axis=3)
    for q in parts:
        np.testing.assert_allclose(q["d"], d_o, rtol=0, atol=1e-8 * np.abs(d_o).max())
        assert abs(float(q["obj"]) - obj_o) <= 1e-9 * abs(obj_o)
        for i in range(tr_o["outer"]):
            np.testing.assert_allclose(q["oz"][i], tr_o["obj_z"][i], rtol=1e-9)
            np.testing.assert_allclose(q["od"][i], tr_o["obj_d"][i], rtol=1e-9)
    np.testing.assert_allclose(z, z_o, rtol=0, atol=1e-8 * np.abs(z_o).max())
    np.testing.assert_allclose(Dz, Dz_o, rtol=0, atol=1e-8 * np.abs(Dz_o).max())


# ---------------------------------------------------------------------------
# The 3D / 4D learners sharded, and the device RNG under sharding
# ---------------------------------------------------------------------------
def _rel(a, b):
    return np.linalg.norm((a - b).ravel()) / np.linalg.norm(b.ravel())


# three blocks over two ranks (2 + 1): the ranks differ in size
# name: (variant, sb, views per axis, psf, K, n, ni, lambda_prior, max_it, tol)
_ND = {
    "L3": ("L3", (8, 9, 7), 1, 3, 3, 6, 2, 0.1, 2, 0.0),
    "L3-tol": ("L3", (10, 10, 6), 1, 5, 4, 9, 3, 0.1, 3, 2e-2),   # test_learn_3d_matches_oracle's
    "L4": ("L4", (10, 9), 2, 5, 3, 6, 2, 1.0, 2, 0.0),
    "L4-3x3": ("L4", (9, 9), 3, 5, 2, 9, 3, 1.0, 2, 0.0),
}
_nd_cache = {}


def _nd_case(name):
    """(b, kernel_size, init, learner arguments) of a small sharded 3D / 4D case."""
    v, sb, UV, psf, K, n, ni, lam, max_it, tol = _ND[name]
    rng = np.random.default_rng(41)
    r = psf // 2
    g = tuple(s + 2 * r for s in sb)
    if v == "L3":
        b = rng.standard_normal(sb + (n,))
        ks = [psf, psf, psf, K]
        init = {"d": rng.standard_normal((psf, psf, psf, K)), "z": rng.standard_normal(g + (K, n))}
    else:
        b = rng.standard_normal(sb + (UV, UV, n))
        ks = [psf, psf, UV, UV, K]
        init = {"d": rng.standard_normal((psf, psf, UV, UV, K)),
                "z": rng.standard_normal(g + (1, 1, K, n))}
    return v, b, ks, init, (1.0, lam, max_it, tol, "brief"), ni


def _nd_oracle(name):
    """The float64 oracle of a case, computed once for the tests that share it."""
    if name not in _nd_cache:
        from oracle import ccsc_oracle as O
        v, b, ks, init, args, ni = _nd_case(name)
        fn = O.learn_3d if v == "L3" else O.learn_4d
        d, z, DZ, obj, _, tr = fn(b, ks, *args, init, ni=ni, trace_objective=True)
        for a in (d, z, DZ):
            a.setflags(write=False)
        _nd_cache[name] = (d, np.real(z), DZ, obj, tr)
    return _nd_cache[name]


def _nd_learn(name, ctx, init="case", **kw):
    from ccsc_code_iccv2017_amd import learners as E
    v, b, ks, init_c, args, ni = _nd_case(name)
    fn = E.admm_learn_conv3D_large if v == "L3" else E.admm_learn_conv4D_lightfield
    d, z, DZ, obj, it = fn(b, ks, *args, init_c if init == "case" else init, ni=ni, ctx=ctx, **kw)
    return d, np.real(z), DZ, obj, it


def _assert_close(got, want, bar):
    for g, w in zip(got, want):
        np.testing.assert_allclose(g, w, rtol=0, atol=bar * np.abs(w).max())


@pytest.mark.parametrize("name", list(_ND))
def test_multi_device_3d_4d_equal_oracle(gpu_ctx, name):
    """The 3D and 4D learners on a multi-device context: learn_group's offsets for these
    variants (b patches with the views and sb[2], z patches of K P, the cropped 4D DZ against
    the uncropped 3D one, K U V psf^2 filter scratch on the ranks past 0) -- equal to the
    oracle on the whole problem at the one-rank bars, and to the one-device engine."""
    from ccsc_code_iccv2017_amd import learners as E
    tol = _ND[name][-1]
    d_o, z_o, DZ_o, obj_o, tr_o = _nd_oracle(name)
    d1, z1, DZ1, obj1, it1 = _nd_learn(name, gpu_ctx)
    mctx = E.Context.multi([0, 0])
    try:
        d2, z2, DZ2, obj2, it2 = _nd_learn(name, mctx)
    finally:
        mctx.close()
    assert d2.shape == d_o.shape and z2.shape == z_o.shape and DZ2.shape == DZ_o.shape
    assert _rel(d2, d_o) < 1e-7
    assert _rel(z2, z_o) < 1e-7
    assert _rel(DZ2, DZ_o) < 1e-7
    assert abs(obj2 - obj_o) <= 1e-9 * abs(obj_o)
    if tol > 0:
        np.testing.assert_array_equal(it2["trace"]["n_d"], np.array(tr_o["n_d"]))
        np.testing.assert_array_equal(it2["trace"]["n_z"], np.array(tr_o["n_z"]))
    _assert_close((d2, z2, DZ2), (d1, z1, DZ1), 1e-10)
    assert abs(obj2 - obj1) <= 1e-10 * abs(obj1)
    np.testing.assert_array_equal(it2["trace"]["n_d"], it1["trace"]["n_d"])
    np.testing.assert_array_equal(it2["trace"]["n_z"], it1["trace"]["n_z"])


@pytest.mark.parametrize("variant", ["L3", "L4"])
def test_multi_device_3d_4d_global_pass_equal_one_device(gpu_ctx, variant):
    """Sharded 3D / 4D learns on grids past one CU's LDS (the global line passes), two blocks
    over two ranks, against the one-device engine -- which test_learn_3d_grids_past_lds_match_
    oracle and test_learn_4d_grid_past_lds_matches_oracle pin to the oracle on these very
    inputs (tol > 0: the sharded change norms stop the inner loops at the same counts)."""
    from ccsc_code_iccv2017_amd import learners as E
    if variant == "L3":
        rng = np.random.default_rng(29)
        sb, psf, K, n = (150, 150, 4), 3, 2, 4
        g = tuple(s + 2 * (psf // 2) for s in sb)
        b = rng.standard_normal(sb + (n,))
        init = {"d": rng.standard_normal((psf, psf, psf, K)), "z": rng.standard_normal(g + (K, n))}
        fn, args = E.admm_learn_conv3D_large, (b, [psf] * 3 + [K], 1.0, 0.1, 2, 5e-2, "all", init)
    else:
        rng = np.random.default_rng(21)
        sb, UV, psf, K, n = (150, 150), 2, 11, 3, 4
        r = psf // 2
        b = rng.standard_normal(sb + (UV, UV, n))
        init = {"d": rng.standard_normal((psf, psf, UV, UV, K)),
                "z": rng.standard_normal((sb[0] + 2 * r, sb[1] + 2 * r, 1, 1, K, n))}
        fn, args = (E.admm_learn_conv4D_lightfield,
                    (b, [psf, psf, UV, UV, K], 1.0, 1.0, 2, 1e-3, "all", init))
    d1, z1, DZ1, obj1, it1 = fn(*args, ni=2, ctx=gpu_ctx)
    mctx = E.Context.multi([0, 0])
    try:
        d2, z2, DZ2, obj2, it2 = fn(*args, ni=2, ctx=mctx)
    finally:
        mctx.close()
    _assert_close((d2, z2.real, DZ2), (d1, z1.real, DZ1), 1e-10)
    assert abs(obj2 - obj1) <= 1e-10 * abs(obj1)
    np.testing.assert_array_equal(it2["trace"]["n_d"], it1["trace"]["n_d"])
    np.testing.assert_array_equal(it2["trace"]["n_z"], it1["trace"]["n_z"])


# dP with ONE patch per block on an 11 x 9 patch: K P = 3 * 15 * 13 = 585, so rank 1's
# codes start at the odd stream element 585 -- the sine half of a Box-Muller pair
_ODD = dict(sb=(11, 9), psf=5, K=3, ni=1, n=2)
# name: (variant, sb, views per axis, psf, K, n, ni, lambda_prior)
_RNG = {
    "dP": ("dp", (12, 11), 1, 5, 3, 6, 2, 1.0),
    "dP-odd": ("dp", _ODD["sb"], 1, _ODD["psf"], _ODD["K"], _ODD["n"], _ODD["ni"], 1.0),
    # (dZ and 3D: theta_div = 1, so lambda_prior = 1 thresholds the small grids' codes to
    # ~1e-7 and leaves nothing to compare)
    "dZ": ("dz", (12, 11), 1, 5, 3, 6, 2, 0.1),
    "L3": ("L3", (8, 9, 7), 1, 3, 3, 6, 2, 0.1),
    "L4": ("L4", (10, 9), 2, 5, 3, 6, 2, 1.0),
}


@pytest.mark.parametrize("name", list(_RNG))
def test_device_rng_init_is_shard_invariant(gpu_ctx, name):
    """init = None: every rank of a multi-device learn draws its patches' part of the one
    global code stream (offset = first local patch * K * P; dZ: the one block draw, on every
    rank) and the same filters, so two outer iterations from the device draw end where the
    one-device learn with the same seed ends."""
    from ccsc_code_iccv2017_amd import learners as E
    v, sb, UV, psf, K, n, ni, lam = _RNG[name]
    b = np.random.default_rng(43).standard_normal(sb + ((UV, UV) if v == "L4" else ()) + (n,))
    fn, ks = {"dp": (E.admm_learn_conv2D_large_dParallel, [psf, psf, K]),
              "dz": (E.admm_learn_conv2D_large_dzParallel, [psf, psf, K]),
              "L3": (E.admm_learn_conv3D_large, [psf, psf, psf, K]),
              "L4": (E.admm_learn_conv4D_lightfield, [psf, psf, UV, UV, K])}[v]
    args = (b, ks, 1.0, lam, 2, 0.0, "brief", None)
    one = fn(*args, ni=ni, seed=977, ctx=gpu_ctx)
    mctx = E.Context.multi([0, 0])
    try:
        two = fn(*args, ni=ni, seed=977, ctx=mctx)
        other = fn(*args, ni=ni, seed=978, ctx=mctx)
    finally:
        mctx.close()
    assert np.abs(one[1]).max() > 1e-2   # the learn left codes to compare
    _assert_close([np.real(a) for a in two[:3]], [np.real(a) for a in one[:3]], 1e-10)
    assert _rel(other[0], one[0]) > 1e-3   # the seed is what decides the draw


def _host_comm():
    import torch
    import torch.distributed as dist

    def host_comm(op, arr):
        t = torch.from_numpy(arr)        # shares memory with the engine's staging buffer
        if op == 0:
            dist.all_reduce(t)
        else:
            dist.broadcast(t, src=0)
    return host_comm


def _odd_case():
    from ccsc_code_iccv2017_amd import learners as E
    c = _ODD
    b = np.random.default_rng(47).standard_normal(c["sb"] + (c["n"],))
    p = E.make_problem(E.L.CCSC_DPAR, b.shape, [c["psf"], c["psf"], c["K"]], 1.0, 1.0, 2, 0.0,
                       "brief", ni=c["ni"], seed=4711)
    return b, p


def _hs_rng_problem(b, ks):
    from ccsc_code_iccv2017_amd import learners as E
    return E.make_problem(E.L.CCSC_HS23, b.shape, ks, 1.0, 0.2, 3, 0.0, "brief", seed=4713)


def _rng_session_run(ctx, p, b, out, smooth_init=None):
    """A session from the device draw: z and d at step 0, then the state after two steps."""
    from ccsc_code_iccv2017_amd import learners as E
    s = E.Session(ctx, p, b, None, None, smooth_init=smooth_init)
    try:
        d0, z0, _, _ = s.results(want_DZ=False)
        s.step(2)
        d, z, DZ, _ = s.results()
    finally:
        s.close()
    np.savez(out, d0=d0, z0=z0, d=d, z=z, DZ=DZ)


def _pair_worker(rank, world, port, out_dir):
    """Every spawned two-rank case of this module in ONE process pair (a pair costs a
    process start, a gloo rendezvous and a HIP initialisation each): the sharded 3D and 4D
    sessions over the host transport, then the HS23 and dP sessions drawn on the device."""
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from ccsc_code_iccv2017_amd import learners as E
    ctx = E.Context(0, rank, world, host_comm=_host_comm())
    for name in ("L3", "L4"):
        v, b, ks, init, (lr, lam, max_it, tol, vb), ni = _nd_case(name)
        p = E.make_problem(E.L.CCSC_L3D if v == "L3" else E.L.CCSC_L4D, b.shape, ks, lr, lam,
                           max_it, tol, vb, ni=ni, trace_objective=True)
        b0, nb = E.shard(E.resolve(p), rank, world)
        sl = slice(b0 * ni, (b0 + nb) * ni)
        s = E.Session(ctx, p, b[..., sl], init["d"], init["z"][..., sl])
        s.step(max_it)
        d, z, DZ, obj = s.results(want_obj=True)
        it = s.iterlog()
        np.savez(os.path.join(out_dir, f"{name}_r{rank}.npz"), d=d, z=z, DZ=DZ, obj=obj,
                 oz=it["trace"]["obj_z"], od=it["trace"]["obj_d"], b0=b0, nb=nb)
        s.close()
    b, sm, _, ks = _hs_case()
    p = _hs_rng_problem(b, ks)
    i0, nl = E.shard(E.resolve(p), rank, world)
    _rng_session_run(ctx, p, b[..., i0:i0 + nl], os.path.join(out_dir, f"hsrng_r{rank}.npz"),
                     smooth_init=sm[..., i0:i0 + nl])
    b, p = _odd_case()
    b0, nb = E.shard(E.resolve(p), rank, world)
    _rng_session_run(ctx, p, b[..., b0:b0 + nb], os.path.join(out_dir, f"dprng_r{rank}.npz"))
    ctx.close()
    dist.barrier()
    dist.destroy_process_group()


@pytest.fixture(scope="module")
def pair_dir(tmp_path_factory):
    import torch.multiprocessing as mp
    out = tmp_path_factory.mktemp("pair")
    mp.start_processes(_pair_worker, args=(2, _free_port(), str(out)), nprocs=2, join=True,
                       start_method="spawn")
    return out


@pytest.mark.parametrize("name", ["L3", "L4"])
def test_3d_4d_two_rank_sessions_equal_oracle(gpu_ctx, pair_dir, name):
    """Session.step of the 3D / 4D learners over two ranks and the host transport (the
    bench's path for C4 / C5): every rank returns block 1's filters, the final objective and
    the global objective traces; the ranks' codes and reconstructions, concatenated, are the
    oracle's."""
    d_o, z_o, DZ_o, obj_o, tr_o = _nd_oracle(name)
    parts = [np.load(pair_dir / f"{name}_r{r}.npz") for r in range(2)]
    assert [int(q["nb"]) for q in parts] == [2, 1]
    for q in parts:
        assert _rel(q["d"], d_o) < 1e-7
        assert abs(float(q["obj"]) - obj_o) <= 1e-9 * abs(obj_o)
        np.testing.assert_allclose(q["oz"], np.array(tr_o["obj_z"]), rtol=1e-9)
        np.testing.assert_allclose(q["od"], np.array(tr_o["obj_d"]), rtol=1e-9)
    z = np.concatenate([q["z"] for q in parts], axis=-1)
    DZ = np.concatenate([q["DZ"] for q in parts], axis=-1)
    assert z.shape == z_o.shape and DZ.shape == DZ_o.shape
    assert _rel(z, z_o) < 1e-7
    assert _rel(DZ, DZ_o) < 1e-7


def _check_rng_pair(tmp_path, gpu_ctx, pair_dir, tag, p, b, bar, split, smooth_init=None):
    from rng_ref import FILTER_SEED_XOR, randn_ref
    _rng_session_run(gpu_ctx, p, b, tmp_path / "one.npz", smooth_init=smooth_init)
    one = np.load(tmp_path / "one.npz")
    parts = [np.load(pair_dir / f"{tag}_r{r}.npz") for r in range(2)]
    assert [q["z0"].shape[-1] for q in parts] == split
    z0 = np.concatenate([q["z0"] for q in parts], axis=-1)
    ref = randn_ref(z0.size, p.seed).reshape(z0.shape, order="F")
    print(f"{tag}: step-0 max |z - randn_ref| = {np.abs(z0 - ref).max():.3e}; ranks hold "
          f"{[q['z0'].shape[-1] for q in parts]} patches")
    # the ranks' draws, side by side, ARE the one-rank draw and the reference stream
    assert np.array_equal(z0, one["z0"]), (
        f"sharded step-0 codes differ from the one-rank draw: max |diff| = "
        f"{np.abs(z0 - one['z0']).max():.3e}, first differing patch "
        f"{int(np.argmax(np.any(z0 != one['z0'], axis=tuple(range(z0.ndim - 1)))))}")
    np.testing.assert_allclose(z0, ref, rtol=0, atol=1e-13)
    for q in parts:
        assert np.array_equal(q["d0"], one["d0"])
        dref = randn_ref(one["d0"][..., 0, :].size if tag == "hsrng" else one["d0"].size,
                         int(p.seed) ^ FILTER_SEED_XOR)
        got = q["d0"][:, :, 0, :] if tag == "hsrng" else q["d0"]
        np.testing.assert_allclose(got, dref.reshape(got.shape, order="F"), rtol=0, atol=1e-13)
        np.testing.assert_allclose(q["d"], one["d"], rtol=0, atol=bar * np.abs(one["d"]).max())
    for k in ("z", "DZ"):
        got = np.concatenate([q[k] for q in parts], axis=-1)
        np.testing.assert_allclose(got, one[k], rtol=0, atol=bar * np.abs(one[k]).max())


def test_hs23_device_rng_two_ranks_equal_one_rank(tmp_path, gpu_ctx, pair_dir):
    """The 2-3D learner with z0 = NULL over two ranks (images 3 + 2): rank 1 draws from
    stream element 3 K P on, so the ranks' step-0 codes are bit for bit the one-rank draw and
    within 1e-13 of tests/rng_ref.py (measured 1.8e-15); two steps later the runs still agree.
    (With every rank drawing from element 0, as the engine did before this test, rank 1's
    first images repeat rank 0's codes: max |diff| 4.9, first differing image 3.)"""
    from ccsc_code_iccv2017_amd import learners as E
    b, sm, _, ks = _hs_case()
    p = E.resolve(_hs_rng_problem(b, ks))
    _check_rng_pair(tmp_path, gpu_ctx, pair_dir, "hsrng", p, b, 1e-8, [3, 2], smooth_init=sm)


def test_dp_device_rng_odd_offset_two_ranks_equal_one_rank(tmp_path, gpu_ctx, pair_dir):
    """dP sessions with z0 = NULL over two ranks, rank 1 starting at the odd stream element
    585 (the sine half of a pair first): step-0 codes bit for bit the one-rank draw and within
    1e-13 of tests/rng_ref.py (measured 1.6e-15), and equal runs after two steps."""
    from ccsc_code_iccv2017_amd import learners as E
    b, p = _odd_case()
    _check_rng_pair(tmp_path, gpu_ctx, pair_dir, "dprng", E.resolve(p), b, 1e-9, [1, 1])
