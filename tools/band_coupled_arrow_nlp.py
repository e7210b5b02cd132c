"""Developer/report tool: what coupling terms on long columns cost on the device-resident nonlinear model of the banded
back-end, everything in HBM.  Three sides on the SAME arrow handle (fpsq_band_create_arrow), pattern, a and h:

  separable   DeviceArrowBandSepQuadNLP      fpsq_band_nlp_create_arrow: the model without the terms
  split       DeviceArrowBandCoupledQuadNLP  fpsq_band_nlp_create_coupled_arrow, the default: the long columns' rows of S apart
                                             from the CSR, one workgroup each (k_bq_long_rows)
  whole       the same under FPSQ_BAND_NLP_LONG_ROWS=0: the long rows inside S, walked by the lane-group kernels -- the
              independent form the split one is measured against

  objgrad     one fpsq_band_nlp_objgrad (values, factorisation, sweeps, products; coupled: + assembly of Wo, + finish [+ long rows])
  hprod 2     fpsq_band_nlp_hprod Val(2)  (coupled: bq_launches' sparse form on Q = diag(qe) - Wo(ys), + k_bcn_hcv [+ 2 long-row launches])
  hprod 1     fpsq_band_nlp_hprod Val(1)  (coupled: + k_bcn_finish_h1 [+ 2 long-row launches])

   python tools/band_coupled_arrow_nlp.py --shape fft --only split    # one side, in this process (also the run for a kernel trace)
   python tools/band_coupled_arrow_nlp.py --shape fft --pairs 5       # the three sides in fresh child processes, interleaved
ONE SIDE PER PROCESS, as tools/band_nlp.py explains (a second band handle in a process factorises slower).  Shapes: aug2dc =
with_arrow(aug2dc_like(N=100), 2, 16) with 2 terms per row, fft = free_final_time_like(N=1e5) (the separable side keeps h and the
explicit zeros), headline = with_arrow(pde_control_like(n=1e6, m=1e5), 3, 5) with 2 terms per row, small (rehearsal).  Prints per
evaluation the median of the repeats and their spread (device events around evaluations that each end in a synchronise);
--pairs prints the median over the pairs, the spreads and the differences.  The launch counts it prints are read off the
drivers' branches for the handle at hand (csrc/fpsq_band_nlp.hip.h, bq_launches), the factorisation and the sweeps not counted.
Accuracy is the tests' business (tests/test_gpu_band_coupled_arrow_nlp.py)."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIDES = ("separable", "whole", "split")

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="fft", choices=["fft", "aug2dc", "headline", "small"])
ap.add_argument("--evals", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--curv", type=float, default=0.3)
ap.add_argument("--terms-per-row", type=int, default=2)
ap.add_argument("--only", default="split", choices=SIDES, help="the side this process runs")
ap.add_argument("--pairs", type=int, default=0)
ap.add_argument("--json", action="store_true", help="(child of --pairs) print one JSON line")
args = ap.parse_args()

if args.pairs:   # this process never opens the GPU: every measurement is a fresh child
    rows = []
    for p in range(args.pairs):
        row = {}
        for only in SIDES:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", args.shape, "--json", "--evals",
                                  str(args.evals), "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--curv",
                                  str(args.curv), "--terms-per-row", str(args.terms_per_row), "--only", only], check=True,
                                 capture_output=True, text=True, timeout=900).stdout
            got = json.loads(out.strip().splitlines()[-1])
            if p == 0:
                print(f"{only}: {got.pop('what')}")
            got.pop("what", None)
            row.update({f"{only} {k}": v for k, v in got.items()})
        rows.append(row)
        print(f"pair {p}: " + ", ".join(f"{k} {v:.4f}" for k, v in row.items()), flush=True)
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    spread = {k: max(r[k] for r in rows) - min(r[k] for r in rows) for k in rows[0]}
    for k in rows[0]:
        print(f"{k}: median {med[k]:.4f} ms (spread {spread[k]:.4f})")
    for k in ("objgrad", "hprod 2", "hprod 1"):
        print(f"split {k} - separable {k} = {med['split ' + k] - med['separable ' + k]:+.4f} ms "
              f"(x {med['split ' + k] / med['separable ' + k]:.3f})")
        d = med["split " + k] - med["whole " + k]
        print(f"split {k} - whole {k} = {d:+.4f} ms (x {med['split ' + k] / med['whole ' + k]:.3f}); the whole form's spread "
              f"{spread['whole ' + k]:.4f}: the split form is {'NOT ' if d <= spread['whole ' + k] else ''}slower by more than it")
    sys.exit(0)

if args.only == "whole":
    os.environ["FPSQ_BAND_NLP_LONG_ROWS"] = "0"   # (read when the model is created)
else:
    os.environ.pop("FPSQ_BAND_NLP_LONG_ROWS", None)

import torch  # noqa: E402

import fps_amd  # noqa: E402,F401
from fps_amd import problems  # noqa: E402
from fps_amd.device_qp import DeviceArrowBandCoupledQuadNLP, DeviceArrowBandSepQuadNLP  # noqa: E402

if args.shape == "fft":
    data = problems.free_final_time_like(N=100_000)
else:
    base, s_r, s_c = {"headline": lambda: (problems.pde_control_like(n=1_000_000, m=100_000), 3, 5),
                      "aug2dc": lambda: (problems.aug2dc_like(N=100), 2, 16),
                      "small": lambda: (problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3), 3, 5)
                      }[args.shape]()
    data = problems.with_coupled_constraints(problems.with_arrow(base, s_r, s_c, seed=7), curv=args.curv, pairs=args.terms_per_row,
                                             seed=7)
qp = data.qp
sigma, rho, eta = 1e3, 1.0, 0.5
delta = float(np.sqrt(np.finfo(float).eps))
on = torch.device("cuda", 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(on)  # noqa: E731
xs = [t(qp.point(k)) for k in range(8)]
xk = t(qp.xhat)
gx, gs, Hv = (torch.empty(qp.n, dtype=torch.float64, device=on) for _ in range(3))
ys = torch.empty(qp.m, dtype=torch.float64, device=on)

if args.only == "separable":
    dev = DeviceArrowBandSepQuadNLP(problems.SepQuadNLP(qp, data.hvals, data.b), sigma=sigma, rho=rho, delta=delta, eta=eta)
else:
    dev = DeviceArrowBandCoupledQuadNLP(data, sigma=sigma, rho=rho, delta=delta, eta=eta)
info = dev.info()


def launches():
    """(objgrad, hprod Val(2), hprod Val(1)) at rho > 0, gx wanted, the factorisation and the sweeps not counted: the drivers'
    branches for this handle and side"""
    cols, form = info["border_cols"] > 0, os.environ.get("FPSQ_BAND_FORM", "0") == "1"
    coupled, split = args.only != "separable", args.only == "split" and cols
    og = 6 + (2 if cols else 0) + (1 if cols and form else 0) + (2 if coupled else 0) + (1 if split else 0)
    h2 = 4 + (1 if cols else 0) + (1 if coupled else 0) + (2 if split else 0)
    h1 = 5 + (2 if cols else 0) + (1 if coupled else 0) + (2 if split else 0)
    return og, h2, h1


what = (f"{qp.name}: n={qp.n} m={qp.m} nnz={qp.nnz} terms={data.nterms}; border rows {info['border_rows']}, long columns "
        f"{info['border_cols']}, blocks {info['nblocks']}, half bandwidth {info['bandwidth_blocks']}, chains {info['chains']}; "
        f"launches objgrad / Val(2) / Val(1): {' / '.join(str(v) for v in launches())}")


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
    print(json.dumps({**med, "what": what}))
else:
    print(f"({args.only}) {what}; {args.evals} evaluations after {args.warmup}, {args.repeats} repeats")
    for k, v in res.items():
        f, c, s = split[k]
        print(f"{k}: median {med[k]:.4f} ms, repeats {[round(a, 4) for a in v]} (spread {max(v) - min(v):.4f}); the library's "
              f"device events of its last call: form {f:.3f} Cholesky {c:.3f} evaluation {s:.3f} ms")
dev.close()
