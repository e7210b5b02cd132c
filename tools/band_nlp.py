"""Developer/report tool: the device-resident model with nonlinear constraints on the banded back-end (fpsq_band_nlp_*) next to
its comparison points on the linear model, everything in HBM:

  nlp objgrad      one fpsq_band_nlp_objgrad (values, factorisation, sweeps, two-array products)
  lin fact+objgrad fpsq_band_factorize + fpsq_band_qp_objgrad: the same factor and sweeps without the second value array
  nlp hprod 2 / 1  fpsq_band_nlp_hprod, both modes, against   lin hprod   fpsq_band_qp_hprod

   python tools/band_nlp.py --shape headline --only nlp     # one side, in this process: also the run for rocprofv3 --kernel-trace --stats
   python tools/band_nlp.py --shape headline --only lin     # (runs on an older build of the library too)
   python tools/band_nlp.py --shape headline --pairs 3 [--other-lib /path/to/parent/libfpsq.so]
        # both sides (and the linear side on ANOTHER build) in fresh child processes, alternating
ONE SIDE PER PROCESS: in a process that holds two band handles the Cholesky of the handle created second took twice as long
(measured: 47.6 instead of 24.7 ms at the headline shape, 4.4 instead of 2.4 on the grid; alone in a process the same
handle gives 24.7) -- as if its two elimination chains ran one after the other, presumably because the four chain streams
and torch's share the runtime's four hardware queues.  That is a property of the process, not of either model.
Shapes: headline = pde_control_like(n=1e6, m=1e5), aug2dc = aug2dc_like(N=100), small (rehearsal).  Prints the median of the
repeats and their spread per evaluation (device events around evaluations that each end in a synchronise) and the library's own
split of its last factorisation (form / Cholesky) and evaluation.  Accuracy is the tests' business (tests/test_gpu_band_nlp.py)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="headline", choices=["headline", "aug2dc", "small"])
ap.add_argument("--evals", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--curv", type=float, default=0.3)
ap.add_argument("--only", default="nlp", choices=["nlp", "lin"], help="the side this process runs")
ap.add_argument("--pairs", type=int, default=0)
ap.add_argument("--other-lib", default=None)
ap.add_argument("--json", action="store_true", help="(child of --pairs) print one JSON line")
args = ap.parse_args()

if args.pairs:   # this process never opens the GPU: every measurement is a fresh child
    assert args.other_lib is None or os.path.exists(args.other_lib)
    sides = [("this lin", None, "lin"), ("this nlp", None, "nlp")]
    if args.other_lib:
        sides.insert(0, ("other lin", args.other_lib, "lin"))
    rows = []
    for p in range(args.pairs):
        row = {}
        for tag, lib, only in sides:
            env = dict(os.environ)
            env.pop("FPSQ_LIB_PATH", None)
            if lib:
                env["FPSQ_LIB_PATH"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", args.shape, "--json", "--evals",
                                  str(args.evals), "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--curv",
                                  str(args.curv), "--only", only], env=env, check=True, capture_output=True, text=True,
                                 timeout=900).stdout
            row.update({f"{tag.split()[0]} {k}": v for k, v in json.loads(out.strip().splitlines()[-1]).items()})
        rows.append(row)
        print(f"pair {p}: " + ", ".join(f"{k} {v:.4f}" for k, v in row.items()), flush=True)
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    for k in rows[0]:
        v = [r[k] for r in rows]
        print(f"{k}: median {med[k]:.4f} ms (spread {max(v) - min(v):.4f})")
    ref = "other" if args.other_lib else "this"
    for new, old in (("nlp objgrad", "lin fact+objgrad"), ("nlp hprod 2", "lin hprod"), ("nlp hprod 1", "lin hprod")):
        print(f"this {new} - {ref} {old} = {med['this ' + new] - med[ref + ' ' + old]:+.4f} ms "
              f"(x {med['this ' + new] / med[ref + ' ' + old]:.3f})")
    sys.exit(0)

import torch  # noqa: E402

import fps_amd  # noqa: E402,F401
from fps_amd import _lib, problems  # noqa: E402

if args.only == "lin":   # another build of the library may predate fpsq_band_nlp_*; the linear model needs none of it
    _probe = C.CDLL(_lib.LIB_PATH)
    _lib.SYMBOLS = [s for s in _lib.SYMBOLS if hasattr(_probe, s[0])]

from fps_amd.device_qp import DeviceBandEqQP  # noqa: E402

qp = {"headline": lambda: problems.pde_control_like(n=1_000_000, m=100_000),
      "aug2dc": lambda: problems.aug2dc_like(N=100),
      "small": lambda: problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3)}[args.shape]()
sigma, rho, eta = 1e3, 1.0, 0.5
delta = float(np.sqrt(np.finfo(float).eps))
on = torch.device("cuda", 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(on)  # noqa: E731
xs = [t(qp.point(k)) for k in range(8)]
xk = t(qp.xhat)
gx, gs, Hv = (torch.empty(qp.n, dtype=torch.float64, device=on) for _ in range(3))
ys = torch.empty(qp.m, dtype=torch.float64, device=on)
vals_dev = t(qp.vals)

fns, closers, infos = {}, [], {}
if args.only == "lin":
    lin = DeviceBandEqQP(qp, sigma=sigma, rho=rho, delta=delta, eta=eta)
    lin.objgrad(xs[0], gx=gx)   # factorises, registers the stream
    llib, lh, lq = lin._lib, lin._h, lin._q

    def lin_fact_objgrad(x):
        fx = C.c_double()
        assert llib.fpsq_band_factorize(lh, vals_dev.data_ptr(), delta, None) == 0
        assert llib.fpsq_band_qp_objgrad(lh, lq, x.data_ptr(), sigma, rho, eta, xk.data_ptr(), C.byref(fx), gx.data_ptr(),
                                         ys.data_ptr(), gs.data_ptr()) == 0

    def lin_hprod(x):
        assert llib.fpsq_band_qp_hprod(lh, lq, x.data_ptr(), sigma, rho, eta, 2, Hv.data_ptr()) == 0

    fns.update({"lin fact+objgrad": lin_fact_objgrad, "lin hprod": lin_hprod})
    closers.append(lin.close)
    infos["lin"] = lin.info
else:
    from fps_amd.device_qp import DeviceBandSepQuadNLP  # noqa: E402

    dev = DeviceBandSepQuadNLP(problems.with_quadratic_constraints(qp, curv=args.curv, seed=7), sigma=sigma, rho=rho,
                               delta=delta, eta=eta)

    def nlp_objgrad(x):
        assert dev.objgrad(x, gx=gx, ys=ys, gs=gs, xk=xk)[1] == 0

    nlp_objgrad(xs[0])
    fns.update({"nlp objgrad": nlp_objgrad, "nlp hprod 2": lambda v: dev.hprod(v, Hv, 2), "nlp hprod 1": lambda v: dev.hprod(v, Hv, 1)})
    closers.append(dev.close)
    infos["nlp"] = dev.info


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


res = {k: [] for k in fns}
split = {}
for r in range(args.repeats):
    for k, fn in fns.items():   # (an nlp hprod runs at the point of the nlp objgrad timed just before it)
        res[k].append(timed(fn))
        i = infos[k[:3]]()
        split[k] = (i["last_form_ms"], i["last_chol_ms"], i["last_solve_ms"])
med = {k: float(np.median(v)) for k, v in res.items()}
if args.json:
    print(json.dumps(med))
else:
    i = next(iter(infos.values()))()
    print(f"{qp.name}: n={qp.n} m={qp.m} nnz={qp.nnz}; blocks {i['nblocks']}, half bandwidth {i['bandwidth_blocks']}, chains "
          f"{i['chains']}; {args.evals} evaluations after {args.warmup}, {args.repeats} repeats, entries alternating")
    for k, v in res.items():
        f, c, s = split[k]
        print(f"{k}: median {med[k]:.4f} ms, repeats {[round(a, 4) for a in v]} (spread {max(v) - min(v):.4f}); the library's "
              f"device events of its last call: form {f:.3f} Cholesky {c:.3f} evaluation {s:.3f} ms")
    z = qp.nnz
    print(f"bytes from shapes (values and indices of the sparse passes): linear prologue / epilogue {12 * z} each; nlp values "
          f"{28 * z} + {24 * z} (stored: a, h, column index, J written; transposed: ta, th, J' written), nlp prologue / "
          f"epilogue {20 * z} each, "
          f"hprod 1: epilogue {20 * z}, H (gs .* v) {12 * z}, J'z {12 * z}")
for c in closers:
    c()
