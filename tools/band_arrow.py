"""Developer/report tool: what s long ROWS together with s long COLUMNS cost on the banded direct back-end (include/fpsq.h
"ARROW BAND").  For one shape it builds the plain handle on the shape itself (the band part alone) and, for every s, two arrow
handles on the shape plus s "mean" rows and s all-row columns that reach them (problems.with_arrow): one with the FUSED
correction (the default) and one with the NESTED one (FPSQ_ARROW_FUSED=0, read at create), all in one process, and times on
device-resident vectors, the three handles ALTERNATING repeat by repeat:

  the factorisation   form / Cholesky / last_border_ms (fpsq_band_info), median of --factorizations runs;
  objgrad             ms per fpsq_band_qp_objgrad;
  hprod_block(k = 8)  ms per fpsq_band_qp_hprod_block.

   python tools/band_arrow.py --shape headline --out profiles/band_arrow_headline.md
   python tools/band_arrow.py --shape aug2dc --out profiles/band_arrow_aug2dc.md
Shapes: headline = pde_control_like(n=1e6, m=1e5), aug2dc = aug2dc_like(N=100), small (rehearsal).  Results are checked by the
library's tests; here the two forms' objgrad are compared with each other.  The Cholesky column of every handle but the first of
the process reads about twice the first one's, whatever the kind of handle (profiles/band_long_columns.md).  Prints a markdown
section and, with --out, writes it to that file."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fps_amd  # noqa: E402,F401
from fps_amd import problems  # noqa: E402
from fps_amd.device_qp import DeviceArrowBandEqQP, DeviceBandEqQP  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="headline", choices=["headline", "aug2dc", "small"])
ap.add_argument("--ss", default="1,4,16")
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--factorizations", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

base = {"headline": lambda: problems.pde_control_like(n=1_000_000, m=100_000),
        "aug2dc": lambda: problems.aug2dc_like(N=100),
        "small": lambda: problems.pde_control_like(n=20000, m=2000, per_row=40, window=1024, seed=3)}[args.shape]()
sigma, rho, eta = 1e3, 1.0, 0.5
delta = float(np.sqrt(np.finfo(float).eps))
on = torch.device("cuda", 0)
K = 8
lines = []


def say(text=""):
    print(text, flush=True)
    lines.append(text)


class Handle:
    def __init__(self, qp, form):
        """form: None (the plain handle), "fused" or "nested" (an arrow handle)"""
        if form is None:
            self.dev = DeviceBandEqQP(qp, sigma=sigma, rho=rho, delta=delta, eta=eta)
        else:
            os.environ["FPSQ_ARROW_FUSED"] = "1" if form == "fused" else "0"
            try:
                self.dev = DeviceArrowBandEqQP(qp, sigma=sigma, rho=rho, delta=delta, eta=eta)
            finally:
                del os.environ["FPSQ_ARROW_FUSED"]
        self.qp = qp
        self.x = torch.from_numpy(qp.x).to(on)
        self.xk = torch.from_numpy(qp.xhat).to(on)
        self.gx = torch.empty(qp.n, dtype=torch.float64, device=on)
        self.V = torch.from_numpy(np.random.default_rng(0).standard_normal((K, qp.n))).to(on)
        self.HV = torch.empty_like(self.V)
        self.fact = []
        for _ in range(args.factorizations):
            self.dev._stale = True
            assert self.dev._factor() == 0
            i = self.dev.info()
            self.fact.append((i["last_form_ms"], i["last_chol_ms"], i["last_border_ms"]))
        self.info = self.dev.info()

    def objgrad(self):
        return self.dev.objgrad(self.x, gx=self.gx, xk=self.xk)[0]

    def hprod_block(self):
        assert self.dev.hprod_block(self.V, self.HV) == 0

    def fact_ms(self):
        return [float(np.median([f[j] for f in self.fact])) for j in range(3)]


def timed(fn):
    for _ in range(args.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(args.calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / args.calls


def alternating(handles, what):
    """median and the repeats of ms per call for every handle, the handles taking turns repeat by repeat"""
    tt = [[] for _ in handles]
    for _ in range(args.repeats):
        for j, h in enumerate(handles):
            tt[j].append(timed(getattr(h, what)))
    return [(float(np.median(t)), t) for t in tt]


def fmt(med, reps):
    return f"{med:.4f} ({', '.join(f'{v:.4f}' for v in reps)})"


t0 = time.time()
plain = Handle(base, None)
i = plain.info
fp = plain.fact_ms()
say(f"## {base.name}: n={base.n} m={base.m} nnz={base.nnz}")
say()
say(f"Plain handle (the band part alone): {i['nblocks']} blocks, half bandwidth {i['bandwidth_blocks']}, chains {i['chains']}, "
    f"factor {i['factor_bytes'] / 1e9:.3f} GB, form {fp[0]:.2f} ms, Cholesky {fp[1]:.2f} ms; created and factorised "
    f"{args.factorizations} times in {time.time() - t0:.1f} s.  {args.calls} calls after {args.warmup} warm-up calls, "
    f"{args.repeats} repeats, the three handles alternating repeat by repeat; median (repeats), ms.")
say()
say("| s_r = s_c | taken rows / columns | blocks / half bandwidth / chains | create s fused / nested | form ms | border ms fused / "
    "nested | pivot ratio | objgrad plain | objgrad fused | objgrad nested | fused / nested | fused / plain | hprod_block(8) plain | "
    "hprod_block(8) fused | hprod_block(8) nested | fused / nested | fused / plain |")
say("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
notes = []
for s in [int(v) for v in args.ss.split(",")]:
    qp = problems.with_arrow(base, s, s, seed=7)
    t0 = time.time()
    f = Handle(qp, "fused")
    t1 = time.time()
    print(f"(s = {s}: fused handle ready after {t1 - t0:.1f} s)", flush=True)
    g = Handle(qp, "nested")
    t2 = time.time()
    print(f"(s = {s}: nested handle ready after {t2 - t1:.1f} s)", flush=True)
    fi = f.info
    assert (fi["border_rows"], fi["border_cols"]) == (s, s), fi
    assert (g.info["border_rows"], g.info["border_cols"]) == (s, s), g.info
    ff, fg = f.fact_ms(), g.fact_ms()
    o = alternating([plain, f, g], "objgrad")
    h = alternating([plain, f, g], "hprod_block")
    say(f"| {s} | {fi['border_rows']} / {fi['border_cols']} | {fi['nblocks']} / {fi['bandwidth_blocks']} / {fi['chains']} | "
        f"{t1 - t0:.1f} / {t2 - t1:.1f} | {ff[0]:.2f} | {ff[2]:.2f} / {fg[2]:.2f} | {fi['border_pivot_ratio']:.3g} | {fmt(*o[0])} | "
        f"{fmt(*o[1])} | {fmt(*o[2])} | {o[1][0] / o[2][0]:.3f} | {o[1][0] / o[0][0]:.3f} | {fmt(*h[0])} | {fmt(*h[1])} | {fmt(*h[2])} | "
        f"{h[1][0] / h[2][0]:.3f} | {h[1][0] / h[0][0]:.3f} |")
    fx_f, fx_g = f.objgrad(), g.objgrad()
    err = float((f.gx - g.gx).abs().max() / g.gx.abs().max())
    notes.append(f"s = {s}: fused against nested, gx max rel {err:.1e}, |phi - phi| / |phi| {abs(fx_f - fx_g) / abs(fx_g):.1e}; "
                 f"nested spread of objgrad {min(o[2][1]):.4f} .. {max(o[2][1]):.4f}, of hprod_block(8) {min(h[2][1]):.4f} .. "
                 f"{max(h[2][1]):.4f}")
    f.dev.close()
    g.dev.close()
say()
for note in notes:
    say("- " + note)
plain.dev.close()
if args.out:
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
