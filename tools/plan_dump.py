"""Host-only dump of what the library decides before it touches a device, one JSON line each
(two builds compare with `diff`): per learner problem the resolved fields, ccsc_supported's
verdict, the shards and the device memory plan; per transform family and length 1..2048 the
reported plan.  python tools/plan_dump.py [--lib path/to/libccsc.so] [--out dump.jsonl]"""
import argparse
import itertools
import json
import os
import sys
from pathlib import Path

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ccsc_code_iccv2017_amd import _lib as L, learners as E      # noqa: E402

PSF = 11
KS = (8, 64, 72, 100, 112, 113, 120, 128, 150, 170, 192, 193, 200, 260, 400, 401, 450)
NIS = (1, 2, 8, 12, 100, 121)
GRIDS2 = ((24, 24), (74, 74), (100, 100), (110, 110), (128, 128), (130, 130), (160, 160),
          (262, 160))
GRIDS3 = ((74, 74, 42), (130, 130, 32), (64, 64, 252))


def problems():
    """(label, Problem) over the pruned product: padded grids (b is the grid less the filter
    border), eight blocks per problem so that 1, 2 and 8 ranks all have work."""
    for tol, df in itertools.product((0.0, 1e-3), ("auto", "cholesky", "woodbury")):
        kw = dict(lambda_residual=1.0, lambda_prior=1.0, max_it=3, tol=tol, verbose="none",
                  dfactor=df)
        for K, ni in itertools.product(KS, NIS):
            for g in GRIDS2:
                sb = (g[0] - PSF + 1, g[1] - PSF + 1)
                for name, var in (("dP", L.CCSC_DPAR), ("dZ", L.CCSC_DZPAR)):
                    yield (f"{name} {g} K={K} ni={ni} tol={tol} {df}",
                           E.make_problem(var, sb + (8 * ni,), (PSF, PSF, K), ni=ni, **kw))
                for v in ((1, 2, 5) if ni <= 12 else (1,)):
                    yield (f"4D {g} views={v} K={K} ni={ni} tol={tol} {df}",
                           E.make_problem(L.CCSC_L4D, sb + (v, v, 8 * ni), (PSF, PSF, v, v, K),
                                          ni=ni, **kw))
            for g in GRIDS3:
                sb = tuple(e - PSF + 1 for e in g)
                yield (f"3D {g} K={K} ni={ni} tol={tol} {df}",
                       E.make_problem(L.CCSC_L3D, sb + (8 * ni,), (PSF, PSF, PSF, K), ni=ni, **kw))
        hs_grids = GRIDS2 if df != "cholesky" else ()   # (the 2-3D learner has no dfactor)
        for K, W, n, g in itertools.product(KS, (3, 31), (4, 100, 101), hs_grids):
            sb = (g[0] - PSF + 1, g[1] - PSF + 1)
            yield (f"L23 {g} W={W} K={K} n={n} tol={tol} {df}",
                   E.make_problem(L.CCSC_HS23, sb + (W, n), (PSF, PSF, W, K), **kw))


def guarded(fn):
    try:
        return fn()
    except L.CCSCError as e:
        return {"error": e.code, "message": str(e)}


def problem_line(label, p):
    out = {"problem": label}
    q = guarded(lambda: E.resolve(p))
    if isinstance(q, dict):
        out["resolve"] = q
        return out
    out["resolved"] = {f: (list(getattr(q, f)) if f in ("sb", "views") else getattr(q, f))
                       for f, _ in L.Problem._fields_}
    eb = L.errbuf()
    out["supported"] = [L.lib().ccsc_supported(q, eb, len(eb)), eb.value.decode(errors="replace")]
    for nr in (1, 2, 8):
        out[f"shard{nr}"] = [guarded(lambda: E.shard(q, r, nr)) for r in sorted({0, nr - 1})]
        out[f"plan_bytes{nr}"] = [guarded(lambda: E.plan_bytes(q, r, nr))
                                  for r in sorted({0, nr - 1})]
    return out


def fft_lines():
    for n in range(1, 2049):
        for fam, name, dims in ((L.FFT_SLICE2D, "slice2d", (n, n)),
                                (L.FFT_TTILE, "ttile", (n // 2 + 1, 1, n)),
                                (L.FFT_LINE2D, "line2d", (n, n)),
                                (L.FFT_LINE3D, "line3d", (n, n, 6)),
                                (L.FFT_LINE3D, "line3d", (6, 6, n))):
            yield {"fft": name, "dims": dims, "plan": guarded(lambda: E.fft_plan(fam, *dims))}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--lib", help="library to load instead of the in-tree build")
    ap.add_argument("--out", type=argparse.FileType("w"), default=sys.stdout)
    a = ap.parse_args()
    if a.lib:
        L.LIB_PATH = Path(a.lib).resolve()
    lines = itertools.chain((problem_line(label, p) for label, p in problems()), fft_lines())
    a.out.writelines(json.dumps(line) + "\n" for line in lines)


if __name__ == "__main__":
    main()
