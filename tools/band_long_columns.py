"""Developer/report tool: what s long COLUMNS cost on the banded direct back-end (include/fpsq.h "LONG COLUMNS").  For one
shape it builds the plain handle on the shape itself and, for every s, the handle with max_cols = 16 on the shape plus s
all-row columns (problems.with_long_columns, kind "param"), all in one process, and times on device-resident vectors, plain
and with long columns ALTERNATING:

  the factorisation   form / Cholesky / last_border_ms (fpsq_band_info), median of --factorizations runs;
  objgrad             ms per fpsq_band_qp_objgrad;
  hprod_block(k = 8)  ms per fpsq_band_qp_hprod_block.

   python tools/band_long_columns.py --shape headline --out profiles/band_long_columns_headline.md
   python tools/band_long_columns.py --shape aug2dc --wide --out profiles/band_long_columns_aug2dc.md
   python tools/band_long_columns.py --shape headline --plain-only     # the handle without added columns alone
Shapes: headline = pde_control_like(n=1e6, m=1e5), aug2dc = aug2dc_like(N=100), small (rehearsal).  --wide also creates the
handle max_cols = 0 gives for the problem with long columns (the wide band of the existing entries) and times it, or records
the text it is refused with; without it only the symbolic phase's figures for that handle are printed (its factor may fit the
device and still take minutes to form).  Results are checked by the library's tests; here the objgrad with long columns is
compared with the wide-band one when --wide ran.  The Cholesky column of every handle but the first of the process reads about
twice the first one's, whatever the kind of handle (profiles/band_long_columns.md).  Prints a markdown section and, with --out,
writes it to that file."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fps_amd  # noqa: E402,F401
from fps_amd import _lib, problems  # noqa: E402
from fps_amd.device_qp import DeviceBandEqQP  # noqa: E402
from fps_amd.qdsolver import FpsqError  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="headline", choices=["headline", "aug2dc", "small"])
ap.add_argument("--ss", default="1,4,16")
ap.add_argument("--calls", type=int, default=100)
ap.add_argument("--warmup", type=int, default=10)
ap.add_argument("--repeats", type=int, default=5)
ap.add_argument("--factorizations", type=int, default=3)
ap.add_argument("--wide", action="store_true")
ap.add_argument("--plain-only", action="store_true")
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
    def __init__(self, qp, cols):
        if cols is None:                       # the existing class and entry: also on a build without the bordered entries
            self.dev = DeviceBandEqQP(qp, sigma=sigma, rho=rho, delta=delta, eta=eta)
        else:
            from fps_amd.device_qp import DeviceBorderedBandEqQP

            self.dev = DeviceBorderedBandEqQP(qp, border=0, cols=cols, sigma=sigma, rho=rho, delta=delta, eta=eta)
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
            self.fact.append((i["last_form_ms"], i["last_chol_ms"], i.get("last_border_ms", 0.0)))
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
say(f"## {base.name}: n={base.n} m={base.m} nnz={base.nnz}")
say()
say(f"Plain handle (no added columns): {i['nblocks']} blocks, half bandwidth {i['bandwidth_blocks']}, chains {i['chains']}, factor "
    f"{i['factor_bytes'] / 1e9:.3f} GB; created and factorised {args.factorizations} times in {time.time() - t0:.1f} s.  "
    f"{args.calls} calls after {args.warmup} warm-up calls, {args.repeats} repeats, handles alternating repeat by repeat; "
    f"median (repeats), ms.")
say()
if args.plain_only:
    f = plain.fact_ms()
    o, h = alternating([plain], "objgrad")[0], alternating([plain], "hprod_block")[0]
    say(f"plain alone: form {f[0]:.2f} ms, Cholesky {f[1]:.2f} ms; objgrad {fmt(*o)}; hprod_block(k=8) {fmt(*h)}")
else:
    say("| s | long columns | blocks / half bandwidth / chains | create s | form ms | Cholesky ms | border ms | pivot ratio | "
        "objgrad plain | objgrad long columns | ratio | hprod_block(8) plain | hprod_block(8) long columns | ratio |")
    say("|---|---|---|---|---|---|---|---|---|---|---|---|---|---|")
    fp = plain.fact_ms()
    say(f"| 0 (plain) | 0 | {i['nblocks']} / {i['bandwidth_blocks']} / {i['chains']} | | {fp[0]:.2f} | {fp[1]:.2f} | | | | | | | | |")
    notes = []
    for s in [int(v) for v in args.ss.split(",")]:
        qp = problems.with_long_columns(base, s, kind="param", seed=7)
        t0 = time.time()
        b = Handle(qp, 16)
        dt = time.time() - t0
        bi = b.info
        assert bi["border_cols"] == s, bi
        fb = b.fact_ms()
        o = alternating([plain, b], "objgrad")
        h = alternating([plain, b], "hprod_block")
        say(f"| {s} | {bi['border_cols']} | {bi['nblocks']} / {bi['bandwidth_blocks']} / {bi['chains']} | {dt:.1f} | {fb[0]:.2f} | "
            f"{fb[1]:.2f} | {fb[2]:.2f} | {bi['border_pivot_ratio']:.3g} | {fmt(*o[0])} | {fmt(*o[1])} | {o[1][0] / o[0][0]:.3f} | "
            f"{fmt(*h[0])} | {fmt(*h[1])} | {h[1][0] / h[0][0]:.3f} |")
        # what max_cols = 0 does with the same problem: the symbolic phase's figures, and with --wide the handle itself
        rp = np.ascontiguousarray(qp.rowptr, dtype=np.int32)
        ci = np.ascontiguousarray(qp.colind, dtype=np.int32)
        wi = _lib.BandInfo()
        _lib.load().fpsq_band_analyze(qp.n, qp.m, rp.ctypes.data, ci.ctypes.data, None, C.byref(wi))
        note = (f"s = {s}, max_cols = 0 (the existing entries): {wi.nblocks} blocks, half bandwidth {wi.bandwidth_blocks}, "
                f"factor {wi.factor_bytes / 1e9:.2f} GB by the symbolic phase")
        if args.wide:
            try:
                t0 = time.time()
                w = Handle(qp, 0)
                fw = w.fact_ms()
                ow, hw = alternating([w], "objgrad")[0], alternating([w], "hprod_block")[0]
                fx_w, fx_b = w.objgrad(), b.objgrad()
                err = float((w.gx - b.gx).abs().max() / w.gx.abs().max())
                note += (f"; created and factorised in {time.time() - t0:.1f} s: form {fw[0]:.2f} ms, Cholesky {fw[1]:.2f} ms, objgrad "
                         f"{fmt(*ow)}, hprod_block(8) {fmt(*hw)}; long columns against it: gx max rel {err:.1e}, "
                         f"|phi - phi| / |phi| {abs(fx_w - fx_b) / abs(fx_w):.1e}")
                w.dev.close()
            except FpsqError as e:
                note += f"; REFUSED: \"{e}\""
        else:
            note += "; the handle itself NOT MEASURED (--wide)"
        notes.append(note)
        b.dev.close()
    say()
    for note in notes:
        say("- " + note)
plain.dev.close()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
