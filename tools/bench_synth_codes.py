"""Times the synthesis from sparse codes (learners.synthesize through ccsc_synthesize_dev,
csrc/synth_codes.hip) against the only other route to the same reconstructions: the dense
[X, Y, K, n] codes through torch.fft.rfft2, the filter spectra, the sum over k and irfft2, on
the same GPU.

Workload: C1's shape (110 x 110 grid, K = 100 filters of 11 x 11, n = 1000 columns) with
codes drawn at kept shares of about 0.05 %, 1 %, 9 % and 60 % (the range DESIGN 7d reports):
every entry is kept with that probability, values are standard normal, rows ascend inside a
column as a session emits them.  Both routes take their inputs on the device, so no host
copy is in either figure; the FFT route's dense codes are expanded from the same triple
before its clock starts, `--fft-cols` columns at a time (its time does not depend on the
share).  Per share: nnz, the median milliseconds per call of both routes after warm-up (host
clock around calls that end in a device synchronise) and the largest difference between the
two results on the first columns.  Also: the host form (NumPy in and out) at one share, and
the 3D shape (74 x 74 x 42, K = 49, 11^3) at one share.  One JSON line.  Needs a GPU.

Usage: python tools/bench_synth_codes.py [--n 1000] [--shares 0.0005,0.01,0.09,0.6]
           [--calls 3] [--warmup 1] [--n3d 20] [--share3d 0.01] [--host-share 0.01]
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
    ap.add_argument("--shares", default="0.0005,0.01,0.09,0.6")
    ap.add_argument("--calls", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--fft-cols", type=int, default=100)
    ap.add_argument("--n3d", type=int, default=20)
    ap.add_argument("--share3d", type=float, default=0.01)
    ap.add_argument("--host-share", type=float, default=0.01)
    args = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        print("bench_synth_codes: no GPU (this tool only measures on the device)",
              file=sys.stderr)
        return 2
    from ccsc_code_iccv2017_amd import learners as E
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)

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
        """A CSC triple on the device: each of the M rows of each column kept with
        probability `share`, ascending rows, standard normal values."""
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

    def dense_chunk(codes, c0, c1, g, K):
        """[c1 - c0, K, Y, X] dense codes of columns c0 .. c1 (row-major of the column-major
        [X, Y, K] column)."""
        jc, ir, pr, (M, _) = codes
        lo, hi = int(jc[c0]), int(jc[c1])
        cols = torch.repeat_interleave(torch.arange(c1 - c0, device=dev), jc[c0 + 1:c1 + 1] -
                                       jc[c0:c1])
        z = torch.zeros((c1 - c0) * M, dtype=torch.float64, device=dev)
        z[cols * M + ir[lo:hi]] = pr[lo:hi]
        return z.view(c1 - c0, K, g[1], g[0])

    with E.Context(0) as ctx:
        # ---- 2D: C1's shape -------------------------------------------------------------
        g, K, s, n = (110, 110), 100, 11, args.n
        M = g[0] * g[1] * K
        d = torch.randn((s, s, K), dtype=torch.float64, device=dev, generator=gen)
        # the embedded filters' spectra [K, Y, X/2 + 1]: circshift(padarray(d), -r)
        emb = torch.zeros((K, g[1], g[0]), dtype=torch.float64, device=dev)
        emb[:, :s, :s] = d.permute(2, 1, 0)
        dhat = torch.fft.rfft2(torch.roll(emb, (-(s // 2), -(s // 2)), dims=(1, 2)))
        res = {"tool": "bench_synth_codes", "grid": list(g), "K": K, "ks": [s, s], "n": n,
               "rows": M, "calls": args.calls, "warmup": args.warmup, "shares": []}
        for share in [float(v) for v in args.shares.split(",")]:
            codes = draw(M, n, share)
            nnz = int(codes[0][-1])
            out = [None]

            def direct():
                out[0] = E.synthesize(d, codes, g, ctx=ctx)
            d_ms, d_all = clock(direct)
            # the FFT route, fft_cols columns at a time: only the transforms are timed
            f_ms, worst = 0.0, 0.0
            for c0 in range(0, n, args.fft_cols):
                c1 = min(n, c0 + args.fft_cols)
                z = dense_chunk(codes, c0, c1, g, K)
                rec = [None]

                def fft():
                    rec[0] = torch.fft.irfft2((torch.fft.rfft2(z) * dhat).sum(dim=1),
                                              s=(g[1], g[0]))
                f_ms += clock(fft)[0]
                if c0 == 0:   # [cols, Y, X] against the direct form's [X, Y, cols]
                    worst = float((rec[0].permute(2, 1, 0) - out[0][..., c0:c1]).abs().max())
                del z, rec
            res["shares"].append({"share": share, "nnz": nnz,
                                  "density": round(nnz / (M * n), 6), "direct_ms": d_ms,
                                  "direct_ms_all": d_all, "fft_ms": round(f_ms, 3),
                                  "max_abs_diff": worst})
            print(json.dumps(res["shares"][-1]), file=sys.stderr, flush=True)
            if share == args.host_share:
                h = tuple(a.cpu().numpy() for a in codes[:3]) + (codes[3],)
                dh = d.cpu().numpy()
                res["host_form"] = {"share": share, "nnz": nnz,
                                    "ms": clock(lambda: E.synthesize(dh, h, g, ctx=ctx))[0]}
            del codes, out
            torch.cuda.empty_cache()
        # ---- 3D ------------------------------------------------------------------------
        g3, K3, s3, n3 = (74, 74, 42), 49, 11, args.n3d
        M3 = g3[0] * g3[1] * g3[2] * K3
        d3 = torch.randn((s3, s3, s3, K3), dtype=torch.float64, device=dev, generator=gen)
        codes = draw(M3, n3, args.share3d)
        ms3, all3 = clock(lambda: E.synthesize(d3, codes, g3, spatial_dims=3, ctx=ctx))
        res["shape3d"] = {"grid": list(g3), "K": K3, "ks": [s3] * 3, "n": n3,
                          "share": args.share3d, "nnz": int(codes[0][-1]), "direct_ms": ms3,
                          "direct_ms_all": all3}
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
