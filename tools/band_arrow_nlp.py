"""Developer/report tool: the nonlinear model on an arrow band (fpsq_band_nlp_create_arrow, DeviceArrowBandSepQuadNLP) next to
its comparison points, everything in HBM.  Sides (ONE band handle per process: see the measurement note of profiles/band_nlp.md):

  arrow-nlp   DeviceArrowBandSepQuadNLP on problems.with_arrow(shape, 3, 5): objgrad, hprod Val(2), hprod Val(1)
  arrow-lin   DeviceArrowBandEqQP on the same pattern: fpsq_band_factorize + fpsq_band_qp_objgrad, fpsq_band_qp_hprod -- the
              linear model; its difference to arrow-nlp is what the nonlinear parts cost (runs on an older build too)
  wide-nlp    DeviceBandSepQuadNLP on the same problem as a wide band (a plain handle): what a user had before (runs on an
              older build too; only where the full band fits the device)

   python tools/band_arrow_nlp.py --shape aug2dc --only arrow-nlp      # one side, in this process: also the run for rocprofv3
   python tools/band_arrow_nlp.py --shape aug2dc --pairs 3 --sides arrow-lin,arrow-nlp,wide-nlp [--other-lib <parent libfpsq.so>]
        # the sides (arrow-lin and wide-nlp on the OTHER build too) in fresh child processes, alternating
   python tools/band_arrow_nlp.py --accuracy                            # the cases of tests/test_gpu_band_arrow_nlp.py at both deltas
   python tools/band_arrow_nlp.py --bits --other-lib <parent libfpsq.so> # the existing banded entries: bitwise against another build
Shapes: headline = pde_control_like(n=1e6, m=1e5), mid = pde_control_like(n=2e5, m=2e4), aug2dc = aug2dc_like(N=100), small
(rehearsal); each with 3 "mean" rows and 5 "param" columns added.  Prints the median of the repeats and their spread per
evaluation (device events around evaluations that each end in a synchronise) and the library's own split of its last
factorisation (form / Cholesky / border) and evaluation."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIDES = ("arrow-lin", "arrow-nlp", "wide-nlp")

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="aug2dc", choices=["headline", "mid", "aug2dc", "small"])
ap.add_argument("--evals", type=int, default=30)
ap.add_argument("--warmup", type=int, default=5)
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--curv", type=float, default=0.3)
ap.add_argument("--only", default="arrow-nlp", choices=SIDES, help="the side this process runs")
ap.add_argument("--sides", default="arrow-lin,arrow-nlp,wide-nlp")
ap.add_argument("--pairs", type=int, default=0)
ap.add_argument("--other-lib", default=None)
ap.add_argument("--accuracy", action="store_true")
ap.add_argument("--bits", action="store_true")
ap.add_argument("--json", action="store_true", help="(child of --pairs) print one JSON line")
ap.add_argument("--dump", default=None, help="(child of --bits) save every output of one evaluation to this .npz")
args = ap.parse_args()


def child(extra, lib):
    env = dict(os.environ)
    env.pop("FPSQ_LIB_PATH", None)
    if lib:
        env["FPSQ_LIB_PATH"] = lib
    return subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", args.shape, "--evals", str(args.evals),
                           "--warmup", str(args.warmup), "--repeats", str(args.repeats), "--curv", str(args.curv)] + extra,
                          env=env, check=True, capture_output=True, text=True, timeout=1100).stdout


if args.pairs:   # this process never opens the GPU: every measurement is a fresh child
    assert args.other_lib is None or os.path.exists(args.other_lib)
    sides = [("this", None, s) for s in args.sides.split(",")]
    if args.other_lib:
        sides = [("other", args.other_lib, s) for _, _, s in sides if s != "arrow-nlp"] + sides
    rows = []
    for p in range(args.pairs):
        row = {}
        for tag, lib, only in sides:
            out = child(["--json", "--only", only], lib)
            row.update({f"{tag} {k}": v for k, v in json.loads(out.strip().splitlines()[-1]).items()})
        rows.append(row)
        print(f"pair {p}: " + ", ".join(f"{k} {v:.4f}" for k, v in row.items()), flush=True)
    for k in rows[0]:
        v = [r[k] for r in rows]
        print(f"{k}: median {float(np.median(v)):.4f} ms (spread {max(v) - min(v):.4f})")
    sys.exit(0)

if args.bits:    # one linear arrow case and one plain nlp case, this build against the other: every output bitwise
    assert args.other_lib and os.path.exists(args.other_lib)
    with tempfile.TemporaryDirectory() as tmp:
        for only in ("arrow-lin", "wide-nlp"):
            files = []
            for tag, lib in (("this", None), ("other", args.other_lib)):
                files.append(os.path.join(tmp, f"{only}-{tag}.npz"))
                child(["--only", only, "--dump", files[-1]], lib)
            a, b = np.load(files[0]), np.load(files[1])
            same = {k: bool(np.array_equal(a[k], b[k])) for k in a.files}
            print(f"{args.shape} {only}: " + ("every output bitwise equal " if all(same.values()) else "DIFFERENT ") + str(same))
    sys.exit(0)

import torch  # noqa: E402

import fps_amd  # noqa: E402,F401
from fps_amd import _lib, problems  # noqa: E402

sigma = 1e3
SE = float(np.sqrt(np.finfo(float).eps))

if args.accuracy:   # the table of profiles/band_arrow_nlp.md: every case of the GPU tests at delta = 0 and sqrt(eps)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_band_arrow_nlp as T
    from fps_amd.device_qp import DeviceArrowBandSepQuadNLP
    from sepquad_ref import SepQuadRef

    keys = ("gx", "ys", "gs", "c", "fx", "Hv2", "Hv1", "gx[L]", "gs[L]", "Hv2[L]", "Hv1[L]", "ys[border]")
    print("| case | delta | " + " | ".join(keys) + " | Hv1-Hv2 | pivot ratio |")
    for case in T.CASES:
        qp, data, rows, cols = T._problem(case)
        border, ncols = T.CASES[case][2]
        for delta in (0.0, SE):
            ref = SepQuadRef(data, sigma, 0.0, delta, 0.0, qp.xhat)
            dev = DeviceArrowBandSepQuadNLP(data, border=border, cols=ncols, sigma=sigma, delta=delta)
            worst, split = {}, 0.0
            for rho, eta in T.PAIRS:
                ref.pen.rho, ref.pen.eta = rho, eta
                e = ref.objgrad(qp.x)
                e["Hv2"], e["Hv1"] = ref.hprod(qp.x, T._v(qp), 2), ref.hprod(qp.x, T._v(qp), 1)
                got = T._evaluate(dev, rho, eta)
                for k, v in T._errors(got, e, rows, cols).items():
                    worst[k] = max(worst.get(k, 0.0), v)
                split = T._rel(got["Hv1"], got["Hv2"])
            ratio = dev.info()["border_pivot_ratio"]
            dev.close()
            print(f"| {case} | {delta:.1e} | " + " | ".join(f"{worst[k]:.1e}" if k in worst else "-" for k in keys) +
                  f" | {split:.1e} | {ratio:.3g} |", flush=True)
    sys.exit(0)

if args.only != "arrow-nlp":   # another build of the library may predate an entry; these sides need none of the new ones
    _probe = C.CDLL(_lib.LIB_PATH)
    _lib.SYMBOLS = [s for s in _lib.SYMBOLS if hasattr(_probe, s[0])]

from fps_amd import device_qp  # noqa: E402

base = {"headline": lambda: problems.pde_control_like(n=1_000_000, m=100_000),
        "mid": lambda: problems.pde_control_like(n=200_000, m=20_000),
        "aug2dc": lambda: problems.aug2dc_like(N=100),
        "small": lambda: problems.pde_control_like(n=3000, m=640, per_row=12, window=256, seed=5)}[args.shape]()
qp = problems.with_arrow(base, 3, 5, seed=7)
rho, eta, delta = 1.0, 0.5, SE
on = torch.device("cuda", 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(on)  # noqa: E731
xs = [t(qp.point(k)) for k in range(8)]
xk = t(qp.xhat)
gx, gs, Hv = (torch.empty(qp.n, dtype=torch.float64, device=on) for _ in range(3))
ys = torch.empty(qp.m, dtype=torch.float64, device=on)
vals_dev = t(qp.vals)
fx_box = [0.0]

if args.only == "arrow-lin":
    dev = device_qp.DeviceArrowBandEqQP(qp, sigma=sigma, rho=rho, delta=delta, eta=eta)
    dev.objgrad(xs[0], gx=gx)   # factorises, registers the stream
    llib, lh, lq = dev._lib, dev._h, dev._q

    def objgrad(x):
        fx = C.c_double()
        assert llib.fpsq_band_factorize(lh, vals_dev.data_ptr(), delta, None) == 0
        assert llib.fpsq_band_qp_objgrad(lh, lq, x.data_ptr(), sigma, rho, eta, xk.data_ptr(), C.byref(fx), gx.data_ptr(),
                                         ys.data_ptr(), gs.data_ptr()) == 0
        fx_box[0] = fx.value

    fns = {"lin fact+objgrad": objgrad, "lin hprod": lambda v: dev.hprod(v, Hv, 2)}
else:
    data = problems.with_quadratic_constraints(qp, curv=args.curv, seed=7)
    if args.only == "arrow-nlp":
        dev = device_qp.DeviceArrowBandSepQuadNLP(data, sigma=sigma, rho=rho, delta=delta, eta=eta)
    else:
        dev = device_qp.DeviceBandSepQuadNLP(data, sigma=sigma, rho=rho, delta=delta, eta=eta)

    def objgrad(x):
        fx, rc = dev.objgrad(x, gx=gx, ys=ys, gs=gs, xk=xk)
        assert rc == 0
        fx_box[0] = fx

    objgrad(xs[0])
    fns = {"nlp objgrad": objgrad, "nlp hprod 2": lambda v: dev.hprod(v, Hv, 2), "nlp hprod 1": lambda v: dev.hprod(v, Hv, 1)}

if args.dump:   # one evaluation of every entry of this side, every output
    out = {}
    for k, fn in fns.items():
        fn(xs[1])
        if "objgrad" in k:
            out.update({"fx": np.float64(fx_box[0]), "gx": gx.cpu().numpy(), "ys": ys.cpu().numpy(), "gs": gs.cpu().numpy()})
        else:
            out[k] = Hv.cpu().numpy()
    np.savez(args.dump, **out)
    dev.close()
    sys.exit(0)


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
        i = dev.info()
        split[k] = (i["last_form_ms"], i["last_chol_ms"], i["last_border_ms"], i["last_solve_ms"])
tag = args.only.split("-")[0]
med = {f"{tag} {k}": float(np.median(v)) for k, v in res.items()}
if args.json:
    print(json.dumps(med))
else:
    i = dev.info()
    print(f"{qp.name} as {args.only}: n={qp.n} m={qp.m} nnz={qp.nnz}; blocks {i['nblocks']}, half bandwidth {i['bandwidth_blocks']}, "
          f"chains {i['chains']}, border rows {i['border_rows']}, long columns {i['border_cols']}; {args.evals} evaluations after "
          f"{args.warmup}, {args.repeats} repeats, entries alternating")
    for k, v in res.items():
        f, c, b, s = split[k]
        print(f"{k}: median {float(np.median(v)):.4f} ms, repeats {[round(a, 4) for a in v]} (spread {max(v) - min(v):.4f}); the "
              f"library's device events of its last call: form {f:.3f} Cholesky {c:.3f} border {b:.3f} evaluation {s:.3f} ms")
dev.close()
