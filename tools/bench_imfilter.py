"""Times the GPU image filter (ccsc_imfilter_dev, csrc/imfilter.hip) on the filters the
reference's drivers apply before they call the engine:

  smooth_init_c3   13 x 13 on 100 x 100 x 31 x 100      (config C3's smooth_init)
  video_smooth     15 x 15 on 1280 x 720 x 64           (the video driver's smooth_init)
  video_psf        3 x 3 x 3 on 1280 x 720 x 64         (the video driver's blur)
  images_256_k31   31 x 31 on 1000 images of 256 x 256  (the largest kernel extent)

Each call is timed between two device events around the whole call (the upload of the
taps, the launches, the final synchronise), after warm-up calls on the same shape; the
median over the timed calls is reported with min and max, as GB/s over the compulsory
16 B per pixel (one fp64 read, one fp64 write) and as the fp64 rate of its 2 flop per
tap and pixel.  Inputs are seeded standard normal, kernels fspecial('gaussian') or, for
the psf, seeded random.  For smooth_init_c3 the tool also times what the Python side did
before: synth.gauss_symmetric(b, device="cuda") from and to NumPy, host copies included,
and its conv2d alone on resident tensors (padded input and weight already on the device).
One JSON line per workload.  Needs a GPU: without one it fails.

Usage: python tools/bench_imfilter.py [--warmup 2] [--calls 7] [--only NAME]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [  # name, n, dims (H, W, T), kernel extents
    ("smooth_init_c3", 31 * 100, (100, 100, 1), (13, 13, 1)),
    ("video_smooth", 1, (1280, 720, 64), (15, 15, 1)),
    ("video_psf", 1, (1280, 720, 64), (3, 3, 3)),
    ("images_256_k31", 1000, (256, 256, 1), (31, 31, 1)),
]


def _stats(ms):
    return {"ms_per_call_median": round(statistics.median(ms), 4),
            "ms_per_call_min": round(min(ms), 4), "ms_per_call_max": round(max(ms), 4)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--only", default=None, help="run one workload by name")
    args = ap.parse_args()

    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("bench_imfilter: no GPU (this tool only measures on the device)", file=sys.stderr)
        return 2
    import torch.nn.functional as Fnn
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import synth
    from ccsc_code_iccv2017_amd.learners import Context

    def timed(fn):
        """Device-event times (ms) of fn, which ends synchronised."""
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.calls):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms

    with Context(0) as ctx:
        for name, n, dims, kdims in WORKLOADS:
            if args.only and args.only != name:
                continue
            H, W, T = dims
            g = torch.Generator(device="cuda").manual_seed(2017)
            x = torch.randn((n, T, W, H), dtype=torch.float64, device="cuda", generator=g)
            out = torch.empty_like(x)
            if kdims[2] == 1:
                k = np.asfortranarray(synth.fspecial_gaussian(kdims[0], 3 * 1.591))
            else:
                k = np.asfortranarray(np.random.default_rng(2017).standard_normal(kdims))
            nd = 3 if T > 1 else 2
            cd = (C.c_int32 * 3)(*dims)
            ck = (C.c_int32 * 3)(*kdims)

            def call():
                eb = L.errbuf()
                L.check(L.lib().ccsc_imfilter_dev(ctx.ptr, x.data_ptr(), out.data_ptr(), n, nd, cd,
                                                  L.dptr(k), ck, L.PAD["symmetric"], eb, len(eb)),
                        eb)

            ms = timed(call)            # synchronises its own stream before returning
            med = statistics.median(ms)
            pixels = n * H * W * T
            taps = kdims[0] * kdims[1] * kdims[2]
            rec = {"workload": name, "n": n, "dims": list(dims), "kernel": list(kdims),
                   "calls": args.calls, **_stats(ms),
                   "GBps_16B_per_pixel": round(16.0 * pixels / (med * 1e-3) / 1e9, 2),
                   "fp64_TFLOPs": round(2.0 * taps * pixels / (med * 1e-3) / 1e12, 3),
                   "finite": bool(torch.isfinite(out).all().item())}
            if name == "smooth_init_c3":
                # the former path, end to end: NumPy in, padded by fancy indexing, conv2d, NumPy out
                b = np.asfortranarray(x.cpu().numpy().reshape(n, W, H).transpose(2, 1, 0))
                host_ms = []
                for i in range(args.warmup + args.calls):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    synth.gauss_symmetric(b, device="cuda")      # ends in a copy to the host
                    if i >= args.warmup:
                        host_ms.append((time.perf_counter() - t0) * 1e3)
                rec["gauss_symmetric_cuda_host_to_host"] = _stats(host_ms)
                # its conv2d alone, on resident tensors
                h = (kdims[0] - 1) // 2
                ix = torch.as_tensor(np.pad(np.arange(H), h, mode="symmetric"), device="cuda")
                iy = torch.as_tensor(np.pad(np.arange(W), h, mode="symmetric"), device="cuda")
                tp = x.reshape(n, W, H)[:, iy][:, :, ix][:, None].contiguous()
                kk = torch.as_tensor(np.ascontiguousarray(k.T[::-1, ::-1]), device="cuda")
                kk = kk[None, None]

                def conv():
                    Fnn.conv2d(tp, kk)
                    torch.cuda.synchronize()

                rec["conv2d_resident"] = _stats(timed(conv))
                del tp, b
            print(json.dumps(rec), flush=True)
            del x, out
    return 0


if __name__ == "__main__":
    sys.exit(main())
