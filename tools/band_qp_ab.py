"""Developer/report tool: one objgrad on the banded direct back-end with everything in HBM, two ways, on the SAME handle
and factor, alternating in one process:

  A  what the entry points older than fpsq_band_qp_* allow: torch for g, f and the epilogue, DeviceEqQP.jac_mul (the
     iterative handle's A / A' products) for c = A x - b and rho A'c, fpsq_band_solve_two_mixed with device pointers in
     between (the caller has to synchronise its stream first: that entry reads device arguments in place on a stream of
     its own), one .item() for phi;
  B  fpsq_band_qp_objgrad (DeviceBandEqQP.objgrad).

   python tools/band_qp_ab.py --shape headline            # A/B table, outputs compared to 1e-12
   python tools/band_qp_ab.py --shape headline --only-b   # B alone: the run to put under rocprofv3 --kernel-trace --stats
Shapes: headline = pde_control_like(n=1e6, m=1e5) (tools/band_headline.py), aug2dc = aug2dc_like(N=100), small (rehearsal).
Prints device-event times per evaluation (median of the repeats and their spread) and, from the shapes alone, the bytes
the two product kernels of B move."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fps_amd  # noqa: E402,F401
from fps_amd import problems  # noqa: E402
from fps_amd.device_qp import DeviceBandEqQP, DeviceEqQP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="headline", choices=["headline", "aug2dc", "small"])
ap.add_argument("--evals", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--only-b", action="store_true")
args = ap.parse_args()

qp = {"headline": lambda: problems.pde_control_like(n=1_000_000, m=100_000),
      "aug2dc": lambda: problems.aug2dc_like(N=100),
      "small": lambda: problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3)}[args.shape]()
sigma, rho, eta = 1e3, 1.0, 0.5
delta = float(np.sqrt(np.finfo(float).eps))
on = torch.device("cuda", 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(on)  # noqa: E731

band = DeviceBandEqQP(qp, sigma=sigma, rho=rho, delta=delta, eta=eta)
xs = [t(qp.point(k)) for k in range(8)]
xk = t(qp.xhat)
gxB, gsB = (torch.empty(qp.n, dtype=torch.float64, device=on) for _ in range(2))
ysB = torch.empty(qp.m, dtype=torch.float64, device=on)


def eval_b(x):
    return band.objgrad(x, gx=gxB, ys=ysB, gs=gsB, xk=xk)[0]


eval_b(xs[0])   # factorises
info = band.info()
print(f"{qp.name}: n={qp.n} m={qp.m} nnz={qp.nnz}; blocks {info['nblocks']}, half bandwidth {info['bandwidth_blocks']}, "
      f"chains {info['chains']}, reordered {info['reordered']}; form {info['last_form_ms']:.2f} ms, Cholesky "
      f"{info['last_chol_ms']:.2f} ms (once)")
mpad = info["nblocks"] * 128
prologue = qp.nnz * 12 + (qp.m + 1) * 4 + qp.n * 16 + qp.m * 8 + mpad * 24 + qp.n * 24
epilogue = qp.nnz * 12 + (qp.n + 1) * 4 + mpad * 24 + qp.n * 8 * 6 + qp.m * 8
print(f"bytes from shapes: k_bq_pack {qp.n * 40}, k_bq_prologue {prologue} (CSR values + indices, the packed [g, x] once, b, r, "
      f"c, and x, q, d for f), k_bq_epilogue {epilogue} (CSR of A', [q1, q2] and c once, x, xk, q, d, gx, gs, ys)")


def timed(fn):
    for k in range(args.warmup):
        fn(xs[k % len(xs)])
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(args.evals):
        fn(xs[k % len(xs)])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.evals


if args.only_b:
    print(f"B alone: {timed(eval_b):.4f} ms per evaluation ({args.evals} evaluations)")
    band.close()
    sys.exit(0)

# ---- A: the same evaluation from the older entry points
it = DeviceEqQP(qp, sigma=sigma, rho=rho, delta=delta, eta=eta)
lib = band._lib
q, d, b = t(qp.qdiag), t(qp.d), t(qp.b)
c = torch.empty(qp.m, dtype=torch.float64, device=on)
p1, p2, gxA, gsA = (torch.empty(qp.n, dtype=torch.float64, device=on) for _ in range(4))
q1, q2 = (torch.empty(qp.m, dtype=torch.float64, device=on) for _ in range(2))


def eval_a(x):
    g = q * x + d
    f = torch.dot(x, 0.5 * q * x + d)
    c.copy_(b)
    it.jac_mul(0, 1.0, x, -1.0, c)                     # c = A x - b
    torch.cuda.synchronize()                           # fpsq_band_solve_two_mixed reads g and c in place on its own stream
    rc = lib.fpsq_band_solve_two_mixed(band._h, g.data_ptr(), c.data_ptr(), p1.data_ptr(), q1.data_ptr(), p2.data_ptr(),
                                       q2.data_ptr())
    assert rc == 0, lib.fpsq_band_last_error(band._h)
    ys = q1 + sigma * q2
    torch.add(p1, p2, alpha=sigma, out=gsA)
    dx = x - xk
    torch.addcmul(gsA, sigma - q, p2, out=gxA)
    gxA.add_(dx, alpha=eta)
    it.jac_mul(1, rho, c, 1.0, gxA)                    # + rho A'c
    phi = f - torch.dot(c, ys) + 0.5 * rho * torch.dot(c, c) + 0.5 * eta * torch.dot(dx, dx)
    return phi.item(), ys


rel = lambda a, bb: float((a - bb).abs().max() / bb.abs().max())  # noqa: E731
fa, ysA = eval_a(xs[1])
fb = eval_b(xs[1])
errs = {"phi": abs(fa - fb) / abs(fa), "gx": rel(gxB, gxA), "ys": rel(ysB, ysA), "gs": rel(gsB, gsA)}
print("B against A (relative, max norm):", {k: f"{v:.2e}" for k, v in errs.items()})
assert max(errs.values()) < 1e-12, errs
ta, tb = [], []
for r in range(args.repeats):
    ta.append(timed(eval_a))
    tb.append(timed(eval_b))
ma, mb = float(np.median(ta)), float(np.median(tb))
print(f"A: median {ma:.4f} ms per evaluation, repeats {[round(v, 4) for v in ta]} (spread {max(ta) - min(ta):.4f})")
print(f"B: median {mb:.4f} ms per evaluation, repeats {[round(v, 4) for v in tb]} (spread {max(tb) - min(tb):.4f})")
print(f"A - B = {ma - mb:.4f} ms ({'above' if ma - mb > max(ta) - min(ta) else 'NOT above'} the spread of A); "
      f"sweeps + both products inside B (device events of the library): {band.info()['last_solve_ms']:.4f} ms")
it.close()
band.close()
