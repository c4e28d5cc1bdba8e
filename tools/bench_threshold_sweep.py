"""Times the threshold sweep (learners.threshold_sweep through ccsc_threshold_sweep_dev,
csrc/sweep_codes.hip) against the route that existed before it, built only from entry points
that were there: per threshold, a boolean filter of the device triple, learners.synthesize(...,
crop=True) on the device, and ((b - out) ** 2) summed per column with torch.

Workload: C1's shape (110 x 110 grid, K = 100 filters of 11 x 11, n = 1000 columns), codes
drawn as tools/bench_synth_codes.py draws them at kept shares of 1 % and 9 % (every row kept
with that probability, standard normal values, ascending rows), data b standard normal on the
interior (crop = 1).  E = 1, 4 and 8 thresholds at the quantiles 0, 1/E, ..., (E - 1)/E of |v|:
the smallest threshold, 0, keeps every entry of the triple.  Everything is on the device, so no
host copy is in either figure; the baseline's column index of every entry is formed once,
outside its clock.  Per (share, E): the median milliseconds of both routes after warm-up (host
clock around calls that end in a device synchronise), their ratio, and the largest relative
difference in sse.  Also the 3D shape (74 x 74 x 42, K = 49, 11^3, n = 20 columns) at one
share.  One JSON line.  Needs a GPU.

Usage: python tools/bench_threshold_sweep.py [--n 1000] [--shares 0.01,0.09] [--E 1,4,8]
           [--calls 3] [--warmup 1] [--n3d 20] [--share3d 0.01]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1000)
    ap.add_argument("--shares", default="0.01,0.09")
    ap.add_argument("--E", default="1,4,8")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n3d", type=int, default=20)
    ap.add_argument("--share3d", type=float, default=0.01)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("bench_threshold_sweep: no GPU (this tool only measures on the device)",
              file=sys.stderr)
        return 2
    from ccsc_code_iccv2017_amd import learners as E
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    Es = [int(v) for v in args.E.split(",")]

    def clock(fn):
        for _ in range(args.warmup):
            fn()
        ms = []
        for _ in range(args.calls):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms), 3), [round(v, 3) for v in ms]

    def draw(M, n, share):
        """As tools/bench_synth_codes.py: each row of each column kept with probability
        `share`, ascending rows, standard normal values."""
        counts, rows = [], []
        step = max(1, min(n, (1 << 28) // M))
        for c0 in range(0, n, step):
            m = min(step, n - c0)
            keep = torch.rand((m, M), device=dev, generator=gen) < share
            counts.append(keep.sum(dim=1))
            rows.append(keep.nonzero()[:, 1])
            del keep
        jc = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        jc[1:] = torch.cumsum(torch.cat(counts), 0)
        ir = torch.cat(rows)
        pr = torch.randn(ir.shape[0], dtype=torch.float64, device=dev, generator=gen)
        return jc, ir, pr, (M, n)

    def thresholds(pr, count):
        """0 and the quantiles k / count of |v| (from a sample: torch.quantile's input limit)."""
        a = pr.abs()
        if a.numel() > 1 << 22:
            a = a[torch.randint(a.numel(), (1 << 22,), device=dev, generator=gen)]
        q = torch.quantile(a, torch.arange(1, count, device=dev, dtype=torch.float64) / count)
        return [0.0] + [float(v) for v in q.cpu()]

    def measure(d, codes, b, g, sdims, ctx):
        jc, ir, pr, (M, n) = codes
        col = torch.repeat_interleave(torch.arange(n, device=dev), jc[1:] - jc[:-1])
        rows = []
        for count in Es:
            eps = thresholds(pr, count)
            got = [None]

            def sweep():
                got[0] = E.threshold_sweep(d, codes, b, eps, g, spatial_dims=sdims, ctx=ctx)

            base = [None]

            def baseline():
                sse = []
                for t in eps:
                    keep = ~(pr.abs() <= t)
                    fjc = torch.zeros(n + 1, dtype=torch.int64, device=dev)
                    fjc[1:] = torch.cumsum(torch.bincount(col[keep], minlength=n), 0)
                    out = E.synthesize(d, (fjc, ir[keep], pr[keep], (M, n)), g,
                                       spatial_dims=sdims, crop=True, ctx=ctx)
                    sse.append(((b - out) ** 2).reshape(-1, n).sum(dim=0))
                    del out
                base[0] = torch.stack(sse)

            s_ms, s_all = clock(sweep)
            b_ms, b_all = clock(baseline)
            rel = float(((got[0]["sse"] - base[0]).abs() / base[0]).max())
            rows.append({"E": count, "sweep_ms": s_ms, "sweep_ms_all": s_all,
                         "baseline_ms": b_ms, "baseline_ms_all": b_all,
                         "baseline_over_sweep": round(b_ms / s_ms, 3),
                         "max_rel_diff_sse": rel,
                         "kept_at_largest_eps": int(got[0]["nnz"][-1].sum())})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
            del got, base
            torch.cuda.empty_cache()
        return rows

    with E.Context(0) as ctx:
        g, K, s, n = (110, 110), 100, 11, args.n
        M = g[0] * g[1] * K
        d = torch.randn((s, s, K), dtype=torch.float64, device=dev, generator=gen)
        # column-major memory, as the entry point takes it: no copy inside the clock
        b = torch.randn((n, g[1] - s + 1, g[0] - s + 1), dtype=torch.float64, device=dev,
                        generator=gen).permute(2, 1, 0)
        res = {"tool": "bench_threshold_sweep", "grid": list(g), "K": K, "ks": [s, s], "n": n,
               "rows": M, "calls": args.calls, "warmup": args.warmup, "shares": []}
        for share in [float(v) for v in args.shares.split(",")]:
            codes = draw(M, n, share)
            res["shares"].append({"share": share, "nnz": int(codes[0][-1]),
                                  "runs": measure(d, codes, b, g, 2, ctx)})
            del codes
            torch.cuda.empty_cache()
        del b
        g3, K3, s3, n3 = (74, 74, 42), 49, 11, args.n3d
        M3 = g3[0] * g3[1] * g3[2] * K3
        d3 = torch.randn((s3, s3, s3, K3), dtype=torch.float64, device=dev, generator=gen)
        b3 = torch.randn((n3,) + tuple(v - s3 + 1 for v in reversed(g3)), dtype=torch.float64,
                         device=dev, generator=gen).permute(3, 2, 1, 0)
        codes = draw(M3, n3, args.share3d)
        res["shape3d"] = {"grid": list(g3), "K": K3, "ks": [s3] * 3, "n": n3,
                          "share": args.share3d, "nnz": int(codes[0][-1]),
                          "runs": measure(d3, codes, b3, g3, 3, ctx)}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
