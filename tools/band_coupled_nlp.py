"""Developer/report tool: what the coupling terms cost on the device-resident nonlinear model of the banded back-end.  The
COUPLED model (fpsq_band_nlp_create_coupled with its terms) against the SEPARABLE model on the same handle kind, pattern, a and
h (fpsq_band_nlp_create), everything in HBM:

  objgrad     one fpsq_band_nlp_objgrad (values, factorisation, sweeps, products; coupled: + assembly of Wo, + finish)
  hprod 2     fpsq_band_nlp_hprod Val(2)  (coupled: bq_launches' sparse form on Q = diag(qe) - Wo(ys), + k_bcn_hcv)
  hprod 1     fpsq_band_nlp_hprod Val(1)  (coupled: + k_bcn_finish_h1; ghjvprod, k_bn_hgv<LG, true>, walks the partner lists)

   python tools/band_coupled_nlp.py --shape bilinear --only coupled   # one side, in this process (also the run for a kernel trace)
   python tools/band_coupled_nlp.py --shape bilinear --pairs 5        # both sides in fresh child processes, interleaved
ONE SIDE PER PROCESS, as tools/band_nlp.py explains (a second band handle in a process factorises slower).  Shapes: bilinear =
bilinear_control_like(N=1e5) (the separable side has h = 0 and the explicit zero: a linear model evaluated by the nonlinear
launches), aug2dc = aug2dc_like(N=100) with 2 terms per row, headline = pde_control_like(n=1e6, m=1e5) with 2 terms per row, small
(rehearsal).  Prints per evaluation the median of the repeats and their spread (device events around evaluations that each end
in a synchronise); --pairs prints the median over the pairs and the differences.  Accuracy is the tests' business
(tests/test_gpu_band_coupled_nlp.py)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="bilinear", choices=["bilinear", "aug2dc", "headline", "small"])
ap.add_argument("--evals", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--curv", type=float, default=0.3)
ap.add_argument("--terms-per-row", type=int, default=2)
ap.add_argument("--only", default="coupled", choices=["coupled", "separable"], help="the side this process runs")
ap.add_argument("--pairs", type=int, default=0)
ap.add_argument("--json", action="store_true", help="(child of --pairs) print one JSON line")
args = ap.parse_args()

if args.pairs:   # this process never opens the GPU: every measurement is a fresh child
    rows = []
    for p in range(args.pairs):
        row = {}
        for only in ("separable", "coupled"):
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", args.shape, "--json", "--evals",
                                  str(args.evals), "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--curv",
                                  str(args.curv), "--terms-per-row", str(args.terms_per_row), "--only", only], check=True,
                                 capture_output=True, text=True, timeout=900).stdout
            row.update({f"{only} {k}": v for k, v in json.loads(out.strip().splitlines()[-1]).items()})
        rows.append(row)
        print(f"pair {p}: " + ", ".join(f"{k} {v:.4f}" for k, v in row.items()), flush=True)
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    for k in rows[0]:
        v = [r[k] for r in rows]
        print(f"{k}: median {med[k]:.4f} ms (spread {max(v) - min(v):.4f})")
    for k in ("objgrad", "hprod 2", "hprod 1"):
        print(f"coupled {k} - separable {k} = {med['coupled ' + k] - med['separable ' + k]:+.4f} ms "
              f"(x {med['coupled ' + k] / med['separable ' + k]:.3f})")
    sys.exit(0)

import torch  # noqa: E402

import fps_amd  # noqa: E402,F401
from fps_amd import problems  # noqa: E402
from fps_amd.device_qp import DeviceBandCoupledQuadNLP, DeviceBandSepQuadNLP  # noqa: E402

if args.shape == "bilinear":
    data = problems.bilinear_control_like(N=100_000)
else:
    base = {"headline": lambda: problems.pde_control_like(n=1_000_000, m=100_000),
            "aug2dc": lambda: problems.aug2dc_like(N=100),
            "small": lambda: problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3)}[args.shape]()
    data = problems.with_coupled_constraints(base, curv=args.curv, pairs=args.terms_per_row, seed=7)
qp = data.qp
sigma, rho, eta = 1e3, 1.0, 0.5
delta = float(np.sqrt(np.finfo(float).eps))
on = torch.device("cuda", 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(on)  # noqa: E731
xs = [t(qp.point(k)) for k in range(8)]
xk = t(qp.xhat)
gx, gs, Hv = (torch.empty(qp.n, dtype=torch.float64, device=on) for _ in range(3))
ys = torch.empty(qp.m, dtype=torch.float64, device=on)

if args.only == "coupled":
    dev = DeviceBandCoupledQuadNLP(data, sigma=sigma, rho=rho, delta=delta, eta=eta)
else:
    dev = DeviceBandSepQuadNLP(problems.SepQuadNLP(qp, data.hvals, data.b), sigma=sigma, rho=rho, delta=delta, eta=eta)


def objgrad(x):
    assert dev.objgrad(x, gx=gx, ys=ys, gs=gs, xk=xk)[1] == 0


objgrad(xs[0])
fns = {"objgrad": objgrad, "hprod 2": lambda v: dev.hprod(v, Hv, 2), "hprod 1": lambda v: dev.hprod(v, Hv, 1)}


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
    for k, fn in fns.items():   # (an hprod runs at the point of the objgrad timed just before it)
        res[k].append(timed(fn))
        i = dev.info()
        split[k] = (i["last_form_ms"], i["last_chol_ms"], i["last_solve_ms"])
med = {k: float(np.median(v)) for k, v in res.items()}
if args.json:
    print(json.dumps(med))
else:
    i = dev.info()
    print(f"{qp.name} ({args.only}): n={qp.n} m={qp.m} nnz={qp.nnz} terms={data.nterms}; blocks {i['nblocks']}, half bandwidth "
          f"{i['bandwidth_blocks']}, chains {i['chains']}; {args.evals} evaluations after {args.warmup}, {args.repeats} repeats")
    for k, v in res.items():
        f, c, s = split[k]
        print(f"{k}: median {med[k]:.4f} ms, repeats {[round(a, 4) for a in v]} (spread {max(v) - min(v):.4f}); the library's "
              f"device events of its last call: form {f:.3f} Cholesky {c:.3f} evaluation {s:.3f} ms")
dev.close()
