"""Times the two preparation steps of csrc/prep.hip on the shapes the reference's
reconstruction drivers give them:

  fill_mosaic      512 x 512 x 16, the demosaicing driver's period-4 mosaic: plane c holds
                   the samples at offset ((c - 1) div 4, (c - 1) mod 4) of every 4 x 4 cell
  fill_random      512 x 512 x 16, a 0.1 %-dense random mask (the long-search case)
  frames           standardise / un-standardise 64 frames of 1280 x 720
  views            standardise / un-standardise 25 views of 376 x 541

Each call is timed between two device events around the whole _dev call (the workspace
allocation, the launches, the final synchronise), after warm-up calls on the same shape; the
median over the timed calls is reported with min and max, and as GB/s over the compulsory
bytes: fill 16 B per pixel (one fp64 read, one fp64 write), standardise 32 B per value (three
reads, one write), un-standardise 16 B per value.  In the same run the tool times what a
caller has without these entries: scipy.ndimage.distance_transform_edt(return_indices=True)
plus the gather on the host (host clock), and the torch expressions
(x - mean) / std(unbiased) and x * s + m on resident tensors (device events).
One JSON line per workload.  Needs a GPU: without one it fails.

Usage: python tools/bench_prep.py [--warmup 2] [--calls 7] [--only NAME]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FILL = [("fill_mosaic", 512, 512, 16), ("fill_random", 512, 512, 16)]
STD = [("frames", 1280 * 720, 64), ("views", 376 * 541, 25)]


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
    import scipy.ndimage
    import torch
    if not torch.cuda.is_available():
        print("bench_prep: no GPU (this tool only measures on the device)", file=sys.stderr)
        return 2
    from ccsc_code_iccv2017_amd import _lib as L
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

    def host_timed(fn):
        ms = []
        for i in range(args.warmup + args.calls):
            t0 = time.perf_counter()
            fn()
            if i >= args.warmup:
                ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    with Context(0) as ctx:
        for name, H, W, n in FILL:
            if args.only and args.only != name:
                continue
            rng = np.random.default_rng(2017)
            mask = np.zeros((n, W, H), dtype=bool)            # memory order of [H, W, n]
            if name == "fill_mosaic":
                for c in range(n):
                    mask[c, c % 4::4, c // 4::4] = True       # rows offset c div 4, columns c mod 4
            else:
                mask = rng.random((n, W, H)) < 0.001
            a = rng.standard_normal((n, W, H)) * mask
            x = torch.as_tensor(a, device="cuda")
            out = torch.empty_like(x)
            idx = torch.empty(x.shape, dtype=torch.int32, device="cuda")

            def call():
                eb = L.errbuf()
                L.check(L.lib().ccsc_nn_fill_dev(ctx.ptr, x.data_ptr(), None, out.data_ptr(),
                                                 idx.data_ptr(), n, H, W, eb, len(eb)), eb)

            ms = timed(call)
            med = statistics.median(ms)
            pixels = n * H * W

            def scipy_fill():
                res = np.empty_like(a)
                for c in range(n):
                    p = a[c]
                    ind = scipy.ndimage.distance_transform_edt(p == 0, return_distances=False,
                                                               return_indices=True)
                    res[c] = p[tuple(ind)]
                return res

            want = scipy_fill()
            got = out.cpu().numpy()
            # ties may go to another of the equally near samples in SciPy: compare distances
            gi = idx.cpu().numpy().astype(np.int64)
            jj, ii = np.meshgrid(np.arange(W), np.arange(H), indexing="ij")
            d2 = (gi % H - ii) ** 2 + (gi // H - jj) ** 2
            edt2 = np.stack([np.rint(scipy.ndimage.distance_transform_edt(a[c] == 0) ** 2)
                             for c in range(n)])
            rec = {"workload": name, "planes": n, "H": H, "W": W, "calls": args.calls,
                   "samples": int(mask.sum()), **_stats(ms),
                   "GBps_16B_per_pixel": round(16.0 * pixels / (med * 1e-3) / 1e9, 2),
                   "distances_equal_scipy_edt": bool(np.array_equal(d2, edt2)),
                   "values_equal_scipy_fill": float((got == want).mean()),
                   "scipy_edt_and_gather_host": _stats(host_timed(scipy_fill))}
            print(json.dumps(rec), flush=True)
            del x, out, idx

        for name, N, planes in STD:
            if args.only and args.only != name:
                continue
            g = torch.Generator(device="cuda").manual_seed(2017)
            x = torch.randn((planes, N), dtype=torch.float64, device="cuda", generator=g) + 10.0
            out = torch.empty_like(x)
            back = torch.empty_like(x)
            mean = torch.empty(planes, dtype=torch.float64, device="cuda")
            sdev = torch.empty_like(mean)

            def fwd():
                eb = L.errbuf()
                L.check(L.lib().ccsc_standardize_dev(ctx.ptr, x.data_ptr(), out.data_ptr(),
                                                     mean.data_ptr(), sdev.data_ptr(), planes, N,
                                                     eb, len(eb)), eb)

            def inv():
                eb = L.errbuf()
                L.check(L.lib().ccsc_unstandardize_dev(ctx.ptr, out.data_ptr(), back.data_ptr(),
                                                       mean.data_ptr(), sdev.data_ptr(), planes,
                                                       N, eb, len(eb)), eb)

            def torch_fwd():
                m = x.mean(dim=1, keepdim=True)
                s = x.std(dim=1, unbiased=True, keepdim=True)
                r = (x - m) / s
                torch.cuda.synchronize()
                return r, m, s

            tr, tm, ts = torch_fwd()

            def torch_inv():
                r = tr * ts + tm
                torch.cuda.synchronize()
                return r

            f_ms, i_ms = timed(fwd), timed(inv)
            fm, im = statistics.median(f_ms), statistics.median(i_ms)
            vals = planes * N
            rec = {"workload": name, "planes": planes, "N": N, "calls": args.calls,
                   "standardize": {**_stats(f_ms),
                                   "GBps_32B_per_value": round(32.0 * vals / (fm * 1e-3) / 1e9, 2)},
                   "unstandardize": {**_stats(i_ms),
                                     "GBps_16B_per_value": round(16.0 * vals / (im * 1e-3) / 1e9, 2)},
                   "torch_standardize_resident": _stats(timed(torch_fwd)),
                   "torch_unstandardize_resident": _stats(timed(torch_inv)),
                   "max_rel_diff_to_torch": float(((out - tr).abs().max() / tr.abs().max()).item()),
                   "round_trip_max_abs": float((back - x).abs().max().item())}
            print(json.dumps(rec), flush=True)
            del x, out, back, tr
    return 0


if __name__ == "__main__":
    sys.exit(main())
