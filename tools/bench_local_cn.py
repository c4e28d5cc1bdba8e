"""Times the GPU local contrast normalisation (ccsc_local_cn_dev, csrc/localcn.hip) on
image sizes past the synthetic patches:

  frames_720p   64 frames of 1280 x 720          (tiled path)
  images_256    1000 images of 256 x 256         (tiled path)
  patches_lds   10^4 images of 100 x 100         (LDS kernel, one workgroup per image)
  patches_tiled the same with CCSC_CN_TILED=1    (tiled path, for reference)

Each call is timed between two device events around the whole call (workspace
allocation, every stage, the final synchronise), after warm-up calls on the same
shape; the median over the timed calls is reported as ms per image and as GB/s over
the compulsory 16 B per pixel (one fp64 read, one fp64 write).  Inputs are seeded
standard normal.  One JSON line per workload.  Needs a GPU: without one it fails.

Usage: python tools/bench_local_cn.py [--warmup 2] [--calls 7] [--only NAME]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = [  # name, n, H, W, CCSC_CN_TILED
    ("frames_720p", 64, 720, 1280, None),
    ("images_256", 1000, 256, 256, None),
    ("patches_lds", 10000, 100, 100, None),
    ("patches_tiled", 10000, 100, 100, "1"),
]


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--only", default=None, help="run one workload by name")
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("bench_local_cn: no GPU (this tool only measures on the device)", file=sys.stderr)
        return 2
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd.learners import Context

    with Context(0) as ctx:
        for name, n, H, W, tiled in WORKLOADS:
            if args.only and args.only != name:
                continue
            if tiled is None:
                os.environ.pop("CCSC_CN_TILED", None)
            else:
                os.environ["CCSC_CN_TILED"] = tiled
            g = torch.Generator(device="cuda").manual_seed(2017)
            x = torch.randn((n, W, H), dtype=torch.float64, device="cuda", generator=g)
            out = torch.empty_like(x)

            def call():
                eb = L.errbuf()
                L.check(L.lib().ccsc_local_cn_dev(ctx.ptr, x.data_ptr(), out.data_ptr(), n, H, W,
                                                  eb, len(eb)), eb)

            for _ in range(args.warmup):
                call()
            ms = []
            for _ in range(args.calls):
                e0 = torch.cuda.Event(enable_timing=True)
                e1 = torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                call()                      # synchronises its own stream before returning
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            med = statistics.median(ms)
            print(json.dumps({
                "workload": name, "n": n, "H": H, "W": W,
                "path": "tiled" if tiled == "1" or H * W > 12288 else "lds",
                "calls": args.calls, "ms_per_call_median": round(med, 4),
                "ms_per_call_min": round(min(ms), 4), "ms_per_call_max": round(max(ms), 4),
                "ms_per_image": round(med / n, 6),
                "GBps_16B_per_pixel": round(16.0 * n * H * W / (med * 1e-3) / 1e9, 2),
                "finite": bool(torch.isfinite(out).all().item()),
            }), flush=True)
            del x, out
    os.environ.pop("CCSC_CN_TILED", None)
    return 0


if __name__ == "__main__":
    sys.exit(main())
