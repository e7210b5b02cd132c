"""Developer/report tool: what the elementwise function terms cost on the device-resident nonlinear model of the banded
back-end.  The FUNCTION model (fpsq_band_nlp_create_fn with codes other than 0) against the SEPARABLE model on the same handle,
pattern, a and h (fpsq_band_nlp_create_arrow), everything in HBM:

  objgrad     one fpsq_band_nlp_objgrad (fn: k_bn_vals_fn + k_bn_tvals_fn in the place of k_bn_vals + k_bn_tvals, one 4-byte
              readback before the factorisation, the FN form of the prologue)
  hprod 2     fpsq_band_nlp_hprod Val(2)  (the same launches)
  hprod 1     fpsq_band_nlp_hprod Val(1)  (the same launches, g / tg in the place of h / th)

   python tools/band_fn_nlp.py --shape pendulum --only fn      # one side, in this process (also the run for a kernel trace)
   python tools/band_fn_nlp.py --shape pendulum --pairs 5      # both sides in fresh child processes, interleaved
   python tools/band_fn_nlp.py --accuracy                      # the error table of tests/test_gpu_band_fn_nlp.py, every case
   python tools/band_fn_nlp.py --shape pendulum --only fn --objective-terms   # the same model WITHOUT and WITH function terms in
                                                               # the objective (fpsq_band_nlp_set_objective_terms), alternating on
                                                               # ONE handle: what k_bn_objfn and the effective vectors cost
   python tools/band_fn_nlp.py --shape aug2dc --only separable --pairs 5 --other-lib <another libfpsq.so>
                                                               # one side on this build and on another (FPSQ_LIB_PATH), interleaved
                                                               # fresh processes: an unchanged path against the build before
ONE SIDE PER PROCESS, as tools/band_nlp.py explains (a second band handle in a process factorises slower).  Shapes:
aug2dc = aug2dc_like(N=100) with 2 mean rows and 16 parameter columns (the arrow shape of profiles/band_coupled_arrow_nlp.md),
headline = pde_control_like(n=1e6, m=1e5) with 3 mean rows and 5 parameter columns,
pendulum = pendulum_like(N=1e5) (its separable side reads the sine entries as 1/2 x^2), small (rehearsal).  On the first two the
codes are uniform over the table and the curvature is 0.1 (tests/sepfunc_ref.py).  Launches per evaluation besides the
factorisation and the sweeps are those of fpsq_band_nlp_create_arrow on the handle (include/fpsq.h); count them in a kernel
trace of `--only fn --evals 1 --warmup 0 --repeats 1`.  Prints per evaluation the median of the repeats and their spread
(device events around evaluations that each end in a synchronise); --pairs prints the median over the pairs and the
differences."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="pendulum", choices=["aug2dc", "headline", "pendulum", "small"])
ap.add_argument("--evals", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--only", default="fn", choices=["fn", "separable"], help="the side this process runs")
ap.add_argument("--pairs", type=int, default=0)
ap.add_argument("--accuracy", action="store_true")
ap.add_argument("--json", action="store_true", help="(child of --pairs) print one JSON line")
ap.add_argument("--objective-terms", action="store_true",
                help="time the side of --only without and with function terms in the objective, alternating on one handle")
ap.add_argument("--other-lib", default=None, help="(with --pairs) the side of --only on this build against another build")
args = ap.parse_args()

if args.pairs:   # this process never opens the GPU: every measurement is a fresh child
    rows = []
    sides = (("other", args.only, args.other_lib), ("this", args.only, None)) if args.other_lib else \
        (("separable", "separable", None), ("fn", "fn", None))
    for p in range(args.pairs):
        row = {}
        for label, only, lib in sides:
            env = dict(os.environ)
            env.pop("FPSQ_LIB_PATH", None)
            if lib:
                env["FPSQ_LIB_PATH"] = os.path.abspath(lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", args.shape, "--json", "--evals",
                                  str(args.evals), "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--only", only],
                                 check=True, capture_output=True, text=True, timeout=900, env=env).stdout
            row.update({f"{label} {k}": v for k, v in json.loads(out.strip().splitlines()[-1]).items()})
        rows.append(row)
        print(f"pair {p}: " + ", ".join(f"{k} {v:.4f}" for k, v in row.items()), flush=True)
    med = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
    spread = {k: max(r[k] for r in rows) - min(r[k] for r in rows) for k in rows[0]}
    for k in rows[0]:
        print(f"{k}: median {med[k]:.4f} ms (spread {spread[k]:.4f})")
    a, b = sides[1][0], sides[0][0]
    for k in ("objgrad", "hprod 2", "hprod 1"):
        print(f"{a} {k} - {b} {k} = {med[a + ' ' + k] - med[b + ' ' + k]:+.4f} ms "
              f"(x {med[a + ' ' + k] / med[b + ' ' + k]:.3f}; the {b} side's spread {spread[b + ' ' + k]:.4f})")
    sys.exit(0)

import torch  # noqa: E402

import fps_amd  # noqa: E402,F401
from fps_amd import _lib, problems  # noqa: E402

if os.environ.get("FPSQ_LIB_PATH"):   # another build may predate entries this tree declares: bind the ones it has
    import ctypes

    _have = ctypes.CDLL(_lib.LIB_PATH)
    _lib.SYMBOLS = [s for s in _lib.SYMBOLS if hasattr(_have, s[0])]
from fps_amd.device_qp import DeviceArrowBandSepFuncNLP, DeviceArrowBandSepQuadNLP, DeviceBandSepFuncNLP  # noqa: E402

if args.accuracy:
    import lane_group_cases as L
    import sepfunc_ref as F
    import test_gpu_band_arrow_nlp as T

    SE = float(np.sqrt(np.finfo(float).eps))

    def table(label, dev, ref):
        qp = dev.qp
        v = np.random.default_rng(0).standard_normal(qp.n)
        rel = lambda a, b: float(np.max(np.abs(a - b)) / np.max(np.abs(b)))  # noqa: E731
        c, gx, ys, gs, H2, H1 = (np.empty(k) for k in (qp.m, qp.n, qp.m, qp.n, qp.n, qp.n))
        for rho, eta in ((0.0, 0.0), (1.0, 0.5)):
            dev.rho = ref.pen.rho = rho
            dev.eta = ref.pen.eta = eta
            dev.cons(qp.x, c)
            fx, rc = dev.objgrad(qp.x, gx=gx, ys=ys, gs=gs, xk=qp.xhat)
            dev.hprod(v, H2, 2), dev.hprod(v, H1, 1)
            e = ref.objgrad(qp.x)
            errs = {"fx": abs(fx - e["fx"]) / abs(e["fx"]), "gx": rel(gx, e["gx"]), "ys": rel(ys, e["ys"]), "gs": rel(gs, e["gs"]),
                    "c": rel(c, e["c"]), "Hv2": rel(H2, ref.hprod(qp.x, v, 2)), "Hv1": rel(H1, ref.hprod(qp.x, v, 1))}
            print(f"{label} rho={rho} eta={eta} rc={rc}: " + " ".join(f"{k}={v_:.1e}" for k, v_ in errs.items()), flush=True)
        dev.close()

    for name in L.NAMES:
        for delta in (0.0, SE):
            table(f"{name} delta={delta:.1e}", DeviceBandSepFuncNLP(F.fn_data(name), sigma=L.SIGMA, delta=delta),
                  F.exact_fn(name, delta))
    for name in T.CASES:
        qp0 = T.CASES[name][0]()[0]
        data, delta, (border, cols) = F.fn_data_of(qp0), T.CASES[name][1], T.CASES[name][2]
        table(f"{name} delta={delta:.1e}", DeviceArrowBandSepFuncNLP(data, border=border, cols=cols, sigma=L.SIGMA, delta=delta),
              F.SepFuncRef(data, L.SIGMA, 0.0, delta, 0.0, qp0.xhat, kept=True))
    sys.exit(0)

if args.shape == "pendulum":
    data = problems.pendulum_like(N=100_000)
else:
    from sepfunc_ref import fn_data_of

    base = {"headline": lambda: problems.pde_control_like(n=1_000_000, m=100_000),
            "aug2dc": lambda: problems.aug2dc_like(N=100),
            "small": lambda: problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3)}[args.shape]()
    data = fn_data_of(problems.with_arrow(base, *((2, 16) if args.shape == "aug2dc" else (3, 5))))
qp = data.qp
sigma, rho, eta = 1e3, 1.0, 0.5
delta = float(np.sqrt(np.finfo(float).eps))
on = torch.device("cuda", 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(on)  # noqa: E731
xs = [t(qp.point(k)) for k in range(8)]
xk = t(qp.xhat)
gx, gs, Hv = (torch.empty(qp.n, dtype=torch.float64, device=on) for _ in range(3))
ys = torch.empty(qp.m, dtype=torch.float64, device=on)

if args.only == "fn":
    dev = DeviceArrowBandSepFuncNLP(data, sigma=sigma, rho=rho, delta=delta, eta=eta)
else:
    dev = DeviceArrowBandSepQuadNLP(problems.SepQuadNLP(qp, data.hvals, data.b), sigma=sigma, rho=rho, delta=delta, eta=eta)


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


if args.objective_terms:
    # the draw of tests/objfn_cases.py: codes uniform over the table, |w| in [0.5, 1.5), a quarter of the weights 0
    from objfn_cases import terms

    w, codes = terms(qp.n)
    if args.shape == "pendulum":   # (theta of a rotating pendulum grows without bound: its energy terms, not a draw with exp)
        energy = problems.pendulum_energy_like(N=100_000)
        w, codes = energy.obj_w, energy.obj_codes
    else:                          # exp stays in double range at every point that is evaluated
        big = np.max(np.abs(np.stack([qp.point(k) for k in range(8)])), axis=0) > 30.0
        codes[big & (codes == problems.FN_EXP)] = problems.FN_SIN
    w, codes = t(w), t(codes)
    both = {f"{k} {side}": [] for k in fns for side in ("plain", "terms")}
    for r in range(args.repeats):
        for side in ("plain", "terms"):
            dev.set_objective_terms(w if side == "terms" else None, codes if side == "terms" else None)
            objgrad(xs[0])
            for k, fn in fns.items():
                both[f"{k} {side}"].append(timed(fn))
    print(f"{qp.name} ({args.only}): n={qp.n} m={qp.m} nnz={qp.nnz}; {args.evals} evaluations after {args.warmup}, "
          f"{args.repeats} repeats, without and with objective terms alternating on one handle")
    for k in fns:
        a, b = both[f"{k} plain"], both[f"{k} terms"]
        print(f"{k}: plain median {np.median(a):.4f} ms (spread {max(a) - min(a):.4f}), with terms {np.median(b):.4f} ms "
              f"(spread {max(b) - min(b):.4f}), difference {np.median(b) - np.median(a):+.4f} ms")
    dev.close()
    sys.exit(0)

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
    print(f"{qp.name} ({args.only}): n={qp.n} m={qp.m} nnz={qp.nnz}; blocks {i['nblocks']}, half bandwidth "
          f"{i['bandwidth_blocks']}, chains {i['chains']}, border rows {i['border_rows']}, long columns {i['border_cols']}; "
          f"{args.evals} evaluations after {args.warmup}, {args.repeats} repeats")
    for k, v in res.items():
        f, c, s = split[k]
        print(f"{k}: median {med[k]:.4f} ms, repeats {[round(a, 4) for a in v]} (spread {max(v) - min(v):.4f}); the library's "
              f"device events of its last call: form {f:.3f} Cholesky {c:.3f} evaluation {s:.3f} ms")
dev.close()
