"""Developer/report tool: k penalty evaluations on the banded direct back-end with everything in HBM, two ways, on the SAME
handle and factor, alternating in one process:

  A  k calls of fpsq_band_qp_objgrad (one point per pair of sweeps over the factor);
  B  one fpsq_band_qp_objgrad_block of k points, each with a linear term D[j] and a right-hand side B[j] of its own
     (8 points per pair of sweeps, on the fp64 matrix cores).

   python tools/band_qp_objgrad_block.py --shape headline                 # A/B table for k = 1, 2, 4, 8, 16
   python tools/band_qp_objgrad_block.py --shape headline --hessian 8     # the same with a sparse Q of half width 8
   python tools/band_qp_objgrad_block.py --shape headline --only-b --ks 8 # B alone: the run for rocprofv3 --kernel-trace --stats
   python tools/band_qp_objgrad_block.py --shape headline --regress       # the entries that existed before: objgrad, hprod,
                                                                          # hprod_block(k = 8); runs on an older build too
Shapes: headline = pde_control_like(n=1e6, m=1e5) (tools/band_headline.py), aug2dc = aug2dc_like(N=100), small (rehearsal).
Prints device-event times per call (median of the repeats and their spread), the time per point and per tile of 8 and, from
the shape alone, the factor bytes the sweeps stream per call over the call's time.  The distance between A and B is measured
with D = None, B = None (the single entry evaluates the model's own d and b); the timed B calls carry D and B."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fps_amd  # noqa: E402,F401
from fps_amd import problems  # noqa: E402
from fps_amd.device_qp import DeviceBandEqQP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="headline", choices=["headline", "aug2dc", "small"])
ap.add_argument("--hessian", type=int, default=0, help="half width of a sparse symmetric Q (0: the diagonal model)")
ap.add_argument("--ks", default="1,2,4,8,16")
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--only-a", action="store_true")
ap.add_argument("--only-b", action="store_true")
ap.add_argument("--regress", action="store_true")
args = ap.parse_args()

qp = {"headline": lambda: problems.pde_control_like(n=1_000_000, m=100_000),
      "aug2dc": lambda: problems.aug2dc_like(N=100),
      "small": lambda: problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3)}[args.shape]()
if args.hessian:
    qp = problems.with_sparse_hessian(qp, args.hessian, 11)
sigma, rho, eta = 1e3, 1.0, 0.5
delta = float(np.sqrt(np.finfo(float).eps))
on = torch.device("cuda", 0)
ks = [int(k) for k in args.ks.split(",")]
kmax = max(ks + [8])

band = DeviceBandEqQP(qp, sigma=sigma, rho=rho, delta=delta, eta=eta)
rng = np.random.default_rng(0)
X, D, XK = (torch.from_numpy(rng.standard_normal((kmax, qp.n))).to(on) for _ in range(3))
B = torch.from_numpy(rng.standard_normal((kmax, qp.m))).to(on)
GA, GB = torch.empty_like(X), torch.empty_like(X)
SA, SB = torch.empty_like(X), torch.empty_like(X)
YA, YB = torch.empty_like(B), torch.empty_like(B)
band.objgrad(X[0], gx=GA[0], ys=YA[0], gs=SA[0], xk=XK[0])   # factorises
info = band.info()
print(f"{qp.name}{' + sparse Q, half width %d' % args.hessian if args.hessian else ''}: n={qp.n} m={qp.m} nnz={qp.nnz}; "
      f"blocks {info['nblocks']}, half bandwidth {info['bandwidth_blocks']}, chains {info['chains']}, factor "
      f"{info['factor_bytes'] / 1e9:.3f} GB; form {info['last_form_ms']:.2f} ms, Cholesky {info['last_chol_ms']:.2f} ms (once)")


def call_a(k):
    for j in range(k):
        band.objgrad(X[j], gx=GA[j], ys=YA[j], gs=SA[j], xk=XK[j])


def call_b(k, family=True):
    fx, rc = band.objgrad_block(X[:k], GX=GB[:k], YS=YB[:k], GS=SB[:k], XK=XK[:k], D=D[:k] if family else None,
                                B=B[:k] if family else None)
    assert rc == 0
    return fx


def timed(fn, k):
    for _ in range(args.warmup):
        fn(k)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.calls):
        fn(k)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.calls


def line(name, tt):
    return (f"{name}: median {float(np.median(tt)):.4f} ms per call, repeats {[round(v, 4) for v in tt]} "
            f"(spread {max(tt) - min(tt):.4f}; {args.calls} calls each)")


if args.regress:
    HA = torch.empty_like(X)
    entries = {"objgrad": lambda k: call_a(1), "hprod": lambda k: band.hprod(X[0], HA[0]),
               "hprod_block(k=8)": lambda k: band.hprod_block(X[:8], HA[:8])}
    tt = {name: [] for name in entries}
    for r in range(args.repeats):
        for name, fn in entries.items():
            tt[name].append(timed(fn, 0))
    for name in entries:
        print(line(name, tt[name]))
    band.close()
    sys.exit(0)

rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
fb = 2 * info["factor_bytes"]   # one pair of sweeps
for k in ks:
    tiles = (k + 7) // 8
    if args.only_a or args.only_b:
        fn, name = (call_a, "A") if args.only_a else (call_b, "B")
        print(line(f"k={k} {name} alone", [timed(fn, k) for _ in range(args.repeats)]))
        continue
    fa = [band.objgrad(X[j], gx=GA[j], ys=YA[j], gs=SA[j], xk=XK[j])[0] for j in range(k)]
    fb_ = call_b(k, family=False)
    torch.cuda.synchronize()
    err = max(max(rel(GB[j], GA[j]), rel(YB[j], YA[j]), rel(SB[j], SA[j]), abs(fb_[j] - fa[j]) / abs(fa[j])) for j in range(k))
    assert err < 1e-9, err
    ta, tb = [], []
    for r in range(args.repeats):
        ta.append(timed(call_a, k))
        tb.append(timed(call_b, k))
    ma, mb = float(np.median(ta)), float(np.median(tb))
    sa = max(ta) - min(ta)
    print(f"k={k}: A median {ma:.4f} ms {[round(v, 4) for v in ta]} (spread {sa:.4f}); B median {mb:.4f} ms "
          f"{[round(v, 4) for v in tb]} (spread {max(tb) - min(tb):.4f}); A - B = {ma - mb:.4f} "
          f"({'above' if ma - mb > sa else 'NOT above'} the spread of A), A / B = {ma / mb:.2f}; per point A {ma / k:.4f}, "
          f"B {mb / k:.4f} ms; B per tile {mb / tiles:.4f} ms; factor bytes over the call's time: A {k * fb / ma / 1e9:.3f}, "
          f"B {tiles * fb / mb / 1e9:.3f} TB/s; B against A max rel {err:.1e}")
band.close()
