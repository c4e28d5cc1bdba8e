"""Times getting the learned codes out of a session: the compressed sparse column path
(ccsc_session_codes_count + ccsc_session_codes_fill, csrc/codes.hip) against the dense
``results(want_z=True)`` fetch of the same session.

Workload: C1's shape (2D dParallel, K = 100 filters of 11 x 11, 100 x 100 patches on the
110 x 110 grid, n = 1000 patches in 10 blocks), d0 / z0 from the device RNG, one outer
iteration.  The dense z is [110, 110, 100, n] float64: 9.68 GB at n = 1000.

Per threshold eps = frac * max|z| the tool reports nnz, the bytes the path moves to the
host (8 (n + 1) for jc, 16 per kept entry for ir and pr), and the host-clock milliseconds
of the count call and of the fill call (each returns synchronised; the fill call includes
its own count pass); beside them the milliseconds and bytes of the dense fetch (the host
array is allocated before the clock starts and touched, so no page faults are timed in
either path).  It also checks the first and last local patch of every triple against the
dense z.  One JSON line.  Needs a GPU: without one it fails.

Usage: python tools/bench_codes.py [--n 1000] [--fracs 0.01,0.05,0.25] [--calls 3]
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
    ap.add_argument("--n", type=int, default=1000, help="patches (a multiple of 100)")
    ap.add_argument("--fracs", default="0.01,0.05,0.25", help="eps as fractions of max|z|")
    ap.add_argument("--calls", type=int, default=3)
    args = ap.parse_args()

    import ctypes as C
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        print("bench_codes: no GPU (this tool only measures on the device)", file=sys.stderr)
        return 2
    from ccsc_code_iccv2017_amd import _lib as L
    from ccsc_code_iccv2017_amd import learners as E

    n, K, ks = args.n, 100, [11, 11, 100]
    rng = np.random.default_rng(7)
    b = rng.standard_normal((100, 100, n))
    lib = L.lib()

    def clock(fn):
        ms = []
        for _ in range(args.calls):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return round(statistics.median(ms), 3)

    with E.Context(0) as ctx:
        p = E.make_problem(L.CCSC_DPAR, b.shape, ks, 1.0, 1.0, 1, 0.0, "none", seed=11)
        s = E.Session(ctx, p, b)
        try:
            s.step(1)
            M, nl = 110 * 110 * K, s.n_local
            z = np.zeros((110, 110, K, nl), order="F")
            out = L.Outputs(L.dptr(None), L.dptr(z), L.dptr(None), L.dptr(None))   # z_res alone
            eb = L.errbuf()

            def dense():
                L.check(lib.ccsc_session_results(s.ptr, C.byref(out), eb, len(eb)), eb)
            dense()                                           # touches the pages
            dense_ms = clock(dense)
            zmax = float(max(z.max(), -z.min()))
            res = {"tool": "bench_codes", "shape": [110, 110, K, nl], "rows": M, "cols": nl,
                   "zmax": zmax, "dense": {"ms": dense_ms, "bytes": z.nbytes}, "sparse": []}
            jc = np.zeros(nl + 1, dtype=np.int64)
            for frac in [float(f) for f in args.fracs.split(",")]:
                eps = frac * zmax

                def count():
                    L.check(lib.ccsc_session_codes_count(s.ptr, eps, L.lptr(jc), None, None, eb,
                                                         len(eb)), eb)
                count()
                nnz = int(jc[-1])
                ir = np.zeros(nnz, dtype=np.int64)
                pr = np.zeros(nnz)

                def fill():
                    L.check(lib.ccsc_session_codes_fill(s.ptr, eps, L.lptr(ir), L.dptr(pr), nnz,
                                                        eb, len(eb)), eb)
                fill()
                for c in (0, nl - 1):                         # spot check against the dense z
                    col = z[..., c].reshape(-1, order="F")
                    keep = np.flatnonzero(~(np.abs(col) <= eps))
                    sl = slice(jc[c], jc[c + 1])
                    if not (np.array_equal(ir[sl], keep) and np.array_equal(pr[sl], col[keep])):
                        print(f"bench_codes: patch {c} differs from the dense z", file=sys.stderr)
                        return 1
                res["sparse"].append({"frac": frac, "eps": eps, "nnz": nnz,
                                      "density": round(nnz / (M * nl), 6),
                                      "bytes": 16 * nnz + 8 * (nl + 1),
                                      "count_ms": clock(count), "fill_ms": clock(fill)})
        finally:
            s.close()
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
