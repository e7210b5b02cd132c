"""Developer tool: the BITS of the device-resident nonlinear model of the banded back-end (fpsq_band_nlp_*), one build of
libfpsq.so against another.  The tests hold this model to 1e-9 against CPU restatements, which cannot see a changed rounding; a
refactor of its kernels or drivers has to leave every bit where it was.

   python tools/band_nlp_bits.py                                   # this build: one line of digests per evaluation
   python tools/band_nlp_bits.py --other-lib <another libfpsq.so>  # both builds, a fresh process each (FPSQ_LIB_PATH), compared

Per case the process evaluates cons, one objgrad with every output ((rho, eta) = (1, 0.5), delta = sqrt(eps), x = qp.x,
xk = qp.xhat), hprod Val(2) and hprod Val(1) (v: default_rng(0)), and prints sha256 digests of the bytes of every output vector
and the bits of fx.  A line belongs to one evaluation, so a differing line names the launches to look at.  Models and cases:
  separable   DeviceBandSepQuadNLP        every case of tests/lane_group_cases.py (every lane-group width on both sides)
  arrow       DeviceArrowBandSepQuadNLP   the shapes of tests/test_gpu_band_arrow_nlp.py
  coupled     DeviceBandCoupledQuadNLP    every case of tests/coupled_cases.py, its `stride` included
  coupled-lg  DeviceBandCoupledQuadNLP    with_coupled_constraints(pairs=2, seed=7) on every case of tests/lane_group_cases.py: the
                                          kernels with the flag CP at all seven widths (one-entry rows get no terms, so every
                                          shape is admissible)
  coupled-arrow  DeviceArrowBandCoupledQuadNLP  every case of tests/coupled_arrow_cases.py.  NOT among the defaults: a build from
                                          before fpsq_band_nlp_create_coupled_arrow lacks the entry (name it in --models to compare
                                          two builds that have it)
  fn          DeviceBandSepFuncNLP        the function model (tests/sepfunc_ref.py fn_data) on every case of
                                          tests/lane_group_cases.py, and DeviceArrowBandSepFuncNLP on the arrow shapes.  NOT among
                                          the defaults: a build from before fpsq_band_nlp_create_fn lacks the entry
  objfn       DeviceBandSepFuncNLP        the function model with function terms in the OBJECTIVE (tests/objfn_cases.py
                                          objfn_data: fpsq_band_nlp_set_objective_terms) on every case of tests/lane_group_cases.py,
                                          and DeviceArrowBandSepQuadNLP / DeviceArrowBandCoupledQuadNLP with the same draw on the
                                          643-row arrow shape.  NOT among the defaults: a build from before the entry lacks it
                                          (the entry is bound only when the build under FPSQ_LIB_PATH has it)
Accuracy is the tests' business."""
import argparse
import hashlib
import os
import struct
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
MODELS = ("separable", "arrow", "coupled", "coupled-lg")

ap = argparse.ArgumentParser()
ap.add_argument("--models", default=",".join(MODELS))
ap.add_argument("--other-lib", default=None)
args = ap.parse_args()

if args.other_lib:   # this process never opens the GPU: each build evaluates in a fresh child
    assert os.path.exists(args.other_lib)
    lines = []
    for lib in (None, args.other_lib):
        env = dict(os.environ)
        env.pop("FPSQ_LIB_PATH", None)
        if lib:
            env["FPSQ_LIB_PATH"] = lib
        got = []
        with subprocess.Popen([sys.executable, os.path.abspath(__file__), "--models", args.models], env=env, text=True,
                              stdout=subprocess.PIPE) as proc:
            for ln in proc.stdout:   # (echoed as they come: a long run shows where it is)
                print(("other " if lib else "this  ") + ln, end="", flush=True)
                got.append(ln.rstrip("\n"))
        if proc.returncode != 0:     # nothing more on the GPU after a failure
            raise SystemExit(f"the evaluations on {lib or 'this build'} ended with {proc.returncode}")
        lines.append([ln for ln in got if ln.startswith("bits ")])
    this, other = lines
    assert len(this) == len(other) and this, (len(this), len(other))
    differ = [(a, b) for a, b in zip(this, other) if a != b]
    for a, b in differ:
        print(f"DIFFERENT\n  this : {a}\n  other: {b}")
    print(f"{len(this)} lines compared, {len(this) - len(differ)} equal, {len(differ)} different")
    sys.exit(1 if differ else 0)

import fps_amd  # noqa: E402,F401
from fps_amd import _lib, problems  # noqa: E402
from fps_amd import device_qp  # noqa: E402
from fps_amd.device_qp import (DeviceArrowBandCoupledQuadNLP, DeviceArrowBandSepQuadNLP, DeviceBandCoupledQuadNLP,  # noqa: E402
                               DeviceBandSepQuadNLP)
import coupled_cases as cc  # noqa: E402
import lane_group_cases as L  # noqa: E402

if os.environ.get("FPSQ_LIB_PATH"):   # another build may predate entries this tree declares: bind the ones it has
    import ctypes

    _have = ctypes.CDLL(_lib.LIB_PATH)
    _lib.SYMBOLS = [s for s in _lib.SYMBOLS if hasattr(_have, s[0])]

SE = float(np.sqrt(np.finfo(float).eps))
SIGMA, RHO, ETA = 1e3, 1.0, 0.5


def digest(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def evaluate(model, case, dev):
    qp = dev.qp
    x, xk = np.ascontiguousarray(qp.x), np.ascontiguousarray(qp.xhat)
    v = np.random.default_rng(0).standard_normal(qp.n)
    c, gx, ys, gs = np.zeros(qp.m), np.zeros(qp.n), np.zeros(qp.m), np.zeros(qp.n)
    Hv2, Hv1 = np.zeros(qp.n), np.zeros(qp.n)
    tag = f"bits {model} {case}"
    rc = dev.cons(x, c)
    print(f"{tag} cons rc={rc} c={digest(c)}")
    fx, rc = dev.objgrad(x, gx, ys, gs, xk)
    print(f"{tag} objgrad rc={rc} fx={struct.pack('<d', fx).hex()} gx={digest(gx)} ys={digest(ys)} gs={digest(gs)}")
    rc = dev.hprod(v, Hv2, 2)
    print(f"{tag} hprod2 rc={rc} Hv={digest(Hv2)}")
    rc = dev.hprod(v, Hv1, 1)
    print(f"{tag} hprod1 rc={rc} Hv={digest(Hv1)}", flush=True)
    dev.close()


kw = dict(sigma=SIGMA, rho=RHO, delta=SE, eta=ETA)
print(f"library: {_lib.LIB_PATH}")
for model in args.models.split(","):
    if model == "separable":
        for name in L.NAMES:
            evaluate(model, name, DeviceBandSepQuadNLP(L.nlp_data(name), **kw))
    elif model == "arrow":
        import test_gpu_band_arrow_nlp as T

        for name in T.CASES:
            border, cols = T.CASES[name][2]
            evaluate(model, name, DeviceArrowBandSepQuadNLP(T._problem(name)[1], border=border, cols=cols, **kw))
    elif model == "coupled":
        for name in list(cc.CASES) + ["stride"]:
            evaluate(model, name, DeviceBandCoupledQuadNLP(cc.data(name), **kw))
    elif model == "coupled-lg":
        for name in L.NAMES:
            data = problems.with_coupled_constraints(L.qp(name), curv=L.CURV, pairs=2, seed=7)
            evaluate(model, name, DeviceBandCoupledQuadNLP(data, **kw))
    elif model == "coupled-arrow":
        import coupled_arrow_cases as ca

        for name in ca.NAMES:
            border, cols = ca.limits(name)
            evaluate(model, name, DeviceArrowBandCoupledQuadNLP(ca.problem(name)[0], border=border, cols=cols, **kw))
    elif model == "fn":
        import sepfunc_ref as F
        import test_gpu_band_arrow_nlp as T

        for name in L.NAMES:
            evaluate(model, name, device_qp.DeviceBandSepFuncNLP(F.fn_data(name), **kw))
        for name in T.CASES:
            border, cols = T.CASES[name][2]
            data = F.fn_data_of(T.CASES[name][0]()[0])
            evaluate(model, name, device_qp.DeviceArrowBandSepFuncNLP(data, border=border, cols=cols, **kw))
    elif model == "objfn":
        import coupled_arrow_cases as ca
        import objfn_cases as oc
        import test_gpu_band_arrow_nlp as T

        for name in L.NAMES:
            evaluate(model, name, device_qp.DeviceBandSepFuncNLP(oc.objfn_data(name), **kw))
        border, cols = T.CASES[T.CASE_643][2]
        evaluate(model, "arrow-" + T.CASE_643, DeviceArrowBandSepQuadNLP(oc.with_terms(T._problem(T.CASE_643)[1]), border=border,
                                                                        cols=cols, **kw))
        evaluate(model, "coupled-arrow-" + T.CASE_643, DeviceArrowBandCoupledQuadNLP(oc.with_terms(ca.problem(T.CASE_643)[0]),
                                                                                border=border, cols=cols, **kw))
    else:
        raise SystemExit(f"unknown model {model}")
