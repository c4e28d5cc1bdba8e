"""Local contrast normalisation of images of any size: the tiled multi-workgroup path of
csrc/localcn.hip (k_cn_stats .. k_cn_store) behind ccsc_local_cn / ccsc_local_cn_dev.

References: the loop restatement of tests/test_synth.py (local_cn_loop) up to 1600
pixels, else synth.local_cn on CPU tensors, which the CPU tests of tests/test_synth.py
pin to that loop.  Tolerance against either: atol = 2e-6 * max(1, |ref|.max()), rtol = 0,
the bound of tests/test_synth.py's GPU test.

Inputs per shape: `random` (seeded standard normal) and `zero_half` (zeros, columns
< 0.3 * W standard normal).  On zero_half more than half of the 13x13 windows hold only
zeros once W > 30, so the median std is exactly 0 whatever the summation order and the
zero-median branch (CreateImages.m:340-347) is taken; test_zero_half_has_zero_median
asserts that on the CPU for every shape listed in ZERO_MEDIAN."""
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from ccsc_code_iccv2017_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_synth import local_cn_loop  # noqa: E402

T = synth.CN_TILE   # the tiled path's tile edge (kCnTile in csrc/localcn.hip)

REJECTED_TODAY = [(111, 111), (7, 1800), (1800, 7), (256, 256), (720, 1280)]
SEAMS = [(7, 7), (T + 1, 9), (9, T + 1), (T + 5, 2 * T + 3), (2 * T + 6, T + 7)]
BOTH_PATHS = [(100, 100), (17, 23)]
# shapes whose zero_half has an exactly-zero median std (asserted on the CPU below)
ZERO_MEDIAN = [(111, 111), (7, 1800), (256, 256), (720, 1280), (9, T + 1), (T + 5, 2 * T + 3),
               (2 * T + 6, T + 7), (100, 100), (130, 70)]


@functools.lru_cache(maxsize=None)
def _image(kind, shape):
    """One input image; the arrays are shared between tests and never written."""
    H, W = shape
    rng = np.random.default_rng([H, W, {"random": 1, "zero_half": 2, "random2": 3}.get(kind, 0)])
    if kind == "constant":
        a = np.full(shape, 0.75)
    elif kind == "zero_half":
        a = np.zeros(shape)
        nz = int(math.ceil(0.3 * W))                 # columns < 0.3 * W
        a[:, :nz] = rng.standard_normal((H, nz))
    else:
        a = rng.standard_normal(shape)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _reference(kind, shape):
    img = _image(kind, shape)
    if shape[0] * shape[1] <= 1600:
        ref = local_cn_loop(img.copy())
    else:
        ref = synth.local_cn(torch.as_tensor(img.copy())[None])[0].numpy()
    ref.setflags(write=False)
    return ref


def _gpu(imgs):
    """synth.local_cn on CUDA tensors for a list of equally sized images."""
    t = torch.as_tensor(np.stack(imgs), dtype=torch.float64, device="cuda")
    return synth.local_cn(t).cpu().numpy()


def _assert_close(got, ref):
    atol = 2e-6 * max(1.0, np.abs(ref).max())
    err = np.abs(got - ref).max()
    print(f"max |got - ref| = {err:.3e}, bound {atol:.3e}")
    assert err <= atol
    # single storage: every output value is a float32
    assert np.array_equal(got.astype(np.float32).astype(np.float64), got)


# ---- CPU ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ZERO_MEDIAN, ids=lambda s: f"{s[0]}x{s[1]}")
def test_zero_half_has_zero_median(shape):
    """zero_half really takes CI:340-347 at this shape: the round(N/2)-th smallest std is
    exactly 0 and nonzero stds exist."""
    img = torch.as_tensor(_image("zero_half", shape).copy())[None]
    k = synth.fspecial_gaussian(13, 3 * 1.591)
    lmn = synth.rconv2(img, k)
    lstd = torch.sqrt(torch.clamp(synth.rconv2(img * img, k) - lmn * lmn, min=0)).flatten()
    lq = int(math.floor(lstd.numel() / 2 + 0.5))
    assert torch.kthvalue(lstd, lq).values.item() == 0.0
    assert bool((lstd > 0).any())


def test_localcn_gateway_compiles_warning_free():
    stub = os.path.join(ROOT, "tests", "mex_stub")
    r = subprocess.run(["gcc", "-std=c11", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter",
                        "-fsyntax-only", "-I", stub, "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "matlab", "ccsc_localcn_mex.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_local_cn_m_is_the_function_the_reference_calls():
    txt = open(os.path.join(ROOT, "matlab", "local_cn.m")).read()
    assert txt.splitlines()[0].strip() == "function I = local_cn(I)"
    assert "ccsc_localcn_mex(" in txt


def test_tile_edge_matches_the_kernel():
    src = open(os.path.join(ROOT, "ccsc_code_iccv2017_amd", "csrc", "localcn.hip")).read()
    assert int(re.search(r"constexpr int kCnTile = (\d+);", src).group(1)) == T


# ---- GPU ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "zero_half"])
@pytest.mark.parametrize("shape", REJECTED_TODAY, ids=lambda s: f"{s[0]}x{s[1]}")
def test_shapes_past_the_lds_limit(shape, kind):
    """Shapes past 12288 pixels, which only the tiled path serves (CCSC_E_UNSUPPORTED
    without it)."""
    _assert_close(_gpu([_image(kind, shape)])[0], _reference(kind, shape))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "zero_half", "constant"])
@pytest.mark.parametrize("shape", SEAMS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_tile_seams_forced_tiled(monkeypatch, shape, kind):
    """One tile, one-pixel ragged tiles and ragged tiles under 6 pixels, whose halo
    reflects back across the tile seam; a constant image has every std 0 and must come
    out exactly 0."""
    monkeypatch.setenv("CCSC_CN_TILED", "1")
    got = _gpu([_image(kind, shape)])[0]
    _assert_close(got, _reference(kind, shape))
    if kind == "constant":
        assert np.all(got == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["random", "zero_half", "constant"])
@pytest.mark.parametrize("shape", BOTH_PATHS, ids=lambda s: f"{s[0]}x{s[1]}")
def test_same_threshold_on_both_paths(monkeypatch, shape, kind):
    """The shared 13x13 accumulate gives both paths the same lmn, lstd and threshold: the
    outputs differ at most by one ulp of the single-precision mean and one more rounding
    of the subtraction."""
    img = _image(kind, shape)
    lds = _gpu([img])[0]
    monkeypatch.setenv("CCSC_CN_TILED", "1")
    tiled = _gpu([img])[0]
    bound = 2 * 2.0 ** -23 * max(1.0, np.abs(lds).max())
    diff = np.abs(tiled - lds).max()
    print(f"max |tiled - lds| = {diff:.3e}, bound {bound:.3e}")
    assert diff <= bound


@pytest.mark.gpu
@pytest.mark.parametrize("ws_mb", [None, "0"])
def test_batch_equals_single_images_bitwise(monkeypatch, gpu_ctx, ws_mb):
    """Images of one batch take different median branches and do not see each other; with
    CCSC_CN_WS_MB=0 every image is its own chunk; the host entry gives the same bits."""
    from ccsc_code_iccv2017_amd import _lib as L
    shape = (111, 111)
    imgs = [_image(k, shape) for k in ("random", "zero_half", "constant", "random2")]
    singles = np.stack([_gpu([im])[0] for im in imgs])
    if ws_mb is not None:
        monkeypatch.setenv("CCSC_CN_WS_MB", ws_mb)
    assert np.array_equal(_gpu(imgs), singles)
    b = np.asfortranarray(np.stack(imgs, axis=2))
    out = np.zeros_like(b, order="F")
    eb = L.errbuf()
    L.check(L.lib().ccsc_local_cn(gpu_ctx.ptr, L.dptr(b), L.dptr(out), 4, shape[0], shape[1], eb,
                                  len(eb)), eb)
    assert np.array_equal(np.moveaxis(out, 2, 0), singles)


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True], ids=["natural", "forced_tiled"])
def test_reproducible_and_in_place(monkeypatch, gpu_ctx, forced):
    """The same call twice gives the same bits, and ccsc_local_cn_dev with out == in the
    bits of the call with separate arrays."""
    from ccsc_code_iccv2017_amd import _lib as L
    if forced:
        monkeypatch.setenv("CCSC_CN_TILED", "1")
    H, W = 130, 70
    imgs = np.stack([_image("random", (H, W)), _image("zero_half", (H, W))])
    x = torch.as_tensor(imgs, device="cuda").transpose(1, 2).contiguous()   # column-major [H, W]

    def run(src, dst):
        torch.cuda.synchronize()
        eb = L.errbuf()
        L.check(L.lib().ccsc_local_cn_dev(gpu_ctx.ptr, src.data_ptr(), dst.data_ptr(), 2, H, W, eb,
                                          len(eb)), eb)
        return dst.cpu().numpy()

    first = run(x, torch.empty_like(x))
    assert np.array_equal(run(x, torch.empty_like(x)), first)
    y = x.clone()
    assert np.array_equal(run(y, y), first)
    _assert_close(first[0].T, _reference("random", (H, W)))


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(6, 50), (50, 6)])
def test_too_small_images_are_rejected(shape):
    from ccsc_code_iccv2017_amd import _lib as L
    with pytest.raises(L.CCSCError) as e:
        synth.local_cn(torch.zeros((1,) + shape, dtype=torch.float64, device="cuda"))
    assert e.value.code == L.CCSC_E_UNSUPPORTED
    assert "at least 7 pixels" in str(e.value)
