"""Developer/report tool: what a sparse symmetric objective Hessian (fpsq_qp_create_csr) costs an evaluation on the ITERATIVE
handle, and that the diagonal model costs what it did (profiles/qp_sparse_hessian.md).

  python tools/qp_sparse_hessian.py --shape headline
      one process, ONE handle, three models on it -- diagonal, half_width 1, half_width 8 (problems.with_sparse_hessian) --
      alternating; objgrad and hprod ms per evaluation (host wall time over device-resident arguments: what a caller sees),
      the kernel launches per evaluation, the algorithmic bytes of the extra launches (from shapes), outputs of a
      stored-zeros Hessian compared with the diagonal model
  python tools/qp_sparse_hessian.py --shape headline --pairs 3 --other-lib /path/to/parent/libfpsq.so
      the diagonal model alone in fresh child processes, alternating between this tree's library and another build
      (FPSQ_LIB_PATH), in interleaved pairs
  python tools/qp_sparse_hessian.py --shape headline --only 8
      one model alone (0 = diagonal): the run to put under rocprofv3 --kernel-trace --stats
Shapes: headline = pde_control_like(n=1e6, m=1e5), small (rehearsal)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="headline", choices=["headline", "small"])
ap.add_argument("--evals", type=int, default=200)
ap.add_argument("--warmup", type=int, default=20)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--only", type=int, default=None, help="half_width of the one model to run (0: diagonal)")
ap.add_argument("--pairs", type=int, default=0)
ap.add_argument("--other-lib", default=None)
ap.add_argument("--seed", type=int, default=4321)
ap.add_argument("--json", action="store_true", help="(child of --pairs) print one JSON line")
args = ap.parse_args()

if args.pairs:   # this process never opens the GPU: every measurement is a fresh child
    assert args.other_lib and os.path.exists(args.other_lib)
    rows = []
    for p in range(args.pairs):
        pair = {}
        for tag, lib in (("other", args.other_lib), ("this", None)):
            env = dict(os.environ)
            env.pop("FPSQ_LIB_PATH", None)
            if lib:
                env["FPSQ_LIB_PATH"] = lib
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", args.shape, "--only", "0", "--json",
                                  "--evals", str(args.evals), "--warmup", str(args.warmup), "--repeats", str(args.repeats)],
                                 env=env, check=True, capture_output=True, text=True, timeout=600).stdout
            pair[tag] = json.loads(out.strip().splitlines()[-1])
        rows.append(pair)
        print(f"pair {p}: objgrad other {pair['other']['objgrad']:.4f} this {pair['this']['objgrad']:.4f} ms; "
              f"hprod other {pair['other']['hprod']:.4f} this {pair['this']['hprod']:.4f} ms", flush=True)
    for k in ("objgrad", "hprod"):
        o, t = [r["other"][k] for r in rows], [r["this"][k] for r in rows]
        print(f"{k}: other median {np.median(o):.4f} (spread {max(o) - min(o):.4f}), this median {np.median(t):.4f} "
              f"(spread {max(t) - min(t):.4f}), this - other = {np.median(t) - np.median(o):+.4f} ms")
    sys.exit(0)

import torch  # noqa: E402

import fps_amd  # noqa: E402,F401
from fps_amd import _lib, problems  # noqa: E402
from fps_amd.device_qp import DeviceEqQP  # noqa: E402

if args.only == 0:   # another build of the library may predate fpsq_qp_create_csr; the diagonal model needs none of it
    _probe = C.CDLL(_lib.LIB_PATH)
    _lib.SYMBOLS = [s for s in _lib.SYMBOLS if hasattr(_probe, s[0])]

qp = {"headline": lambda: problems.pde_control_like(n=1_000_000, m=100_000),
      "small": lambda: problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3)}[args.shape]()
sigma, rho, eta = 1e3, 1.0, 0.5
delta = float(np.sqrt(np.finfo(float).eps))
on = torch.device("cuda", 0)
t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(on)  # noqa: E731

dev = DeviceEqQP(qp, sigma=sigma, rho=rho, delta=delta, eta=eta)
lib, h = dev._lib, dev._h
xs = [t(qp.point(k)) for k in range(8)]
xk = t(qp.xhat)
gx, gs, Hv = (torch.empty(qp.n, dtype=torch.float64, device=on) for _ in range(3))
ys = torch.empty(qp.m, dtype=torch.float64, device=on)
dev._order(xs[0])   # torch's stream is the producer: device-resident arguments, stream-ordered return
st = (_lib.Stats * 4)()


def model(hw, zeros=False):
    """(a model on the SAME handle, nnz of R)"""
    if hw == 0:
        return dev._q, 0
    sq = problems.with_sparse_hessian(qp, hw, args.seed)
    vals = sq.hess_vals
    if zeros:   # the diagonal model's Q with every off-diagonal entry stored as 0.0
        Q = sq.hess_csr().copy()
        Q.data[:] = 0.0
        Q.setdiag(qp.qdiag)
        vals = Q.data.copy()
    q = C.c_void_p()
    rc = lib.fpsq_qp_create_csr(h, sq.hess_rowptr.ctypes.data, sq.hess_colind.ctypes.data, vals.ctypes.data,
                                qp.d.ctypes.data, qp.b.ctypes.data, C.byref(q))
    assert rc == 0, lib.fpsq_last_error(h)
    return q, int(vals.size) - qp.n


def objgrad(q, x):
    fx = C.c_double()
    rc = lib.fpsq_qp_objgrad(h, q, x.data_ptr(), sigma, rho, eta, xk.data_ptr(), C.byref(fx), gx.data_ptr(), ys.data_ptr(),
                             gs.data_ptr(), st)
    assert rc >= 0, lib.fpsq_last_error(h)
    return fx.value


def hprod(q, x):
    assert lib.fpsq_qp_hprod(h, q, x.data_ptr(), sigma, rho, eta, 2, Hv.data_ptr(), st) >= 0, lib.fpsq_last_error(h)


def timed(fn, q):
    for k in range(args.warmup):
        fn(q, xs[k % len(xs)])
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(args.evals):
        fn(q, xs[k % len(xs)])
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / args.evals


hws = [0, 1, 8] if args.only is None else [args.only]
models = {hw: model(hw) for hw in hws}
if args.only is None:   # stored zeros against the diagonal model
    qz, _ = model(2, zeros=True)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    f0 = objgrad(dev._q, xs[1])
    hprod(dev._q, xs[1])
    torch.cuda.synchronize()
    keep = [v.clone() for v in (gx, ys, gs, Hv)]
    f1 = objgrad(qz, xs[1])
    hprod(qz, xs[1])
    torch.cuda.synchronize()
    print("stored zeros against the diagonal model (relative, max norm):",
          {"phi": f"{abs(f1 - f0) / abs(f0):.1e}", **{k: f"{rel(a, b):.1e}" for k, a, b in zip(("gx", "ys", "gs", "Hv"), (gx, ys, gs, Hv), keep)}})
    lib.fpsq_qp_destroy(qz)
res = {hw: {"objgrad": [], "hprod": []} for hw in hws}
launches = {hw: {} for hw in hws}
for r in range(args.repeats):
    for hw in hws:
        for name, fn in (("objgrad", objgrad), ("hprod", hprod)):
            res[hw][name].append(timed(fn, models[hw][0]))
            i = dev.info()
            launches[hw][name] = (i["last_kernel_launches"], i["last_loop_iterations"])
med = {hw: {k: float(np.median(v)) for k, v in res[hw].items()} for hw in hws}
if args.json:
    print(json.dumps(med[hws[0]]))
else:
    print(f"{qp.name}: n={qp.n} m={qp.m} nnz={qp.nnz}; {args.evals} evaluations after {args.warmup}, {args.repeats} repeats, "
          f"models alternating; host wall time per evaluation, device-resident arguments")
    for hw in hws:
        nnzr = models[hw][1]
        for k in ("objgrad", "hprod"):
            v = res[hw][k]
            extra = "" if hw == 0 or 0 not in med else f", + {med[hw][k] - med[0][k]:.4f} ms over the diagonal model"
            print(f"half_width {hw} (nnz(R) = {nnzr}) {k}: median {med[hw][k]:.4f} ms, repeats {[round(a, 4) for a in v]} "
                  f"(spread {max(v) - min(v):.4f}){extra}; last call: {launches[hw][k][0]} launches, {launches[hw][k][1]} loop iterations")
        if hw:
            r_bytes = nnzr * 12 + (qp.n + 1) * 4   # values, columns, row offsets of R
            front = r_bytes + qp.n * 8 * 2 + qp.n * 8 * 2      # + the gathered x and x again per row, d read, d_eff written
            hsv = r_bytes + qp.n * 8 * 2 + qp.n * 8 * 2        # + the gathered v and v again per row, q read, Hsv written
            sub_g = r_bytes + qp.n * 8 + qp.n * 8 * 2          # + the gathered p2, the tail's gx read, gx written
            sub_h = r_bytes + qp.n * 8 * 2 + qp.n * 8 * 2      # + the gathered v and p1, the tail's Hv read, Hv written
            print(f"   bytes from shapes: k_qp_csr front {front}, hsv {hsv}, subtract behind objgrad {sub_g}, behind hprod {sub_h}")
for hw in hws:
    if hw:
        lib.fpsq_qp_destroy(models[hw][0])
dev.close()
