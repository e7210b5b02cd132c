"""Developer aid: ms per call of the two entry points that hand out p1 = g - A'q1 and v = -A'q2 behind the recurrences
(fpsq_solve_two_mixed, fpsq_ys_gs) at the headline size, all vectors resident on the device.  A/B runs select the build with
FPSQ_LIB_PATH (one process per build):
    python tools/seam_time.py [calls]
Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fps_amd  # noqa: E402,F401
from fps_amd import _lib, problems  # noqa: E402

calls = int(sys.argv[1]) if len(sys.argv) > 1 else 60
qp = problems.pde_control_hashed()
lib = _lib.load()
o = _lib.Options()
lib.fpsq_default_options(qp.n, qp.m, C.byref(o))
h = C.c_void_p()
assert lib.fpsq_create(C.byref(h), qp.n, qp.m, C.byref(o)) == 0, lib.fpsq_last_error(None)
assert lib.fpsq_set_jacobian_structure_csr(h, qp.rowptr.ctypes.data, qp.colind.ctypes.data) == 0, lib.fpsq_last_error(h)
assert lib.fpsq_set_jacobian_values(h, qp.vals.ctypes.data) == 0, lib.fpsq_last_error(h)
dev = torch.device("cuda:0")
g = torch.from_numpy(qp.qdiag * qp.x + qp.d).to(dev)
c = torch.from_numpy(qp.scipy_csr() @ qp.x - qp.b).to(dev)
on, om = [torch.empty(qp.n, dtype=torch.float64, device=dev) for _ in range(2)], [torch.empty(qp.m, dtype=torch.float64, device=dev) for _ in range(2)]
torch.cuda.synchronize()
st = (_lib.Stats * 2)()


def mixed():
    return lib.fpsq_solve_two_mixed(h, g.data_ptr(), c.data_ptr(), on[0].data_ptr(), om[0].data_ptr(), on[1].data_ptr(), om[1].data_ptr(), st)


def ys_gs():
    return lib.fpsq_ys_gs(h, g.data_ptr(), c.data_ptr(), 1e3, on[0].data_ptr(), om[0].data_ptr(), on[1].data_ptr(), om[1].data_ptr(), st)


res = {"lib": os.path.basename(_lib.LIB_PATH), "calls": calls}
for name, fn in (("solve_two_mixed", mixed), ("ys_gs", ys_gs)):
    for _ in range(5):
        assert fn() >= 0, lib.fpsq_last_error(h)
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    torch.cuda.synchronize()
    res[name + "_ms"] = round((time.perf_counter() - t0) / calls * 1e3, 4)
    res[name + "_iters"] = [st[0].niter, st[1].niter]
i = _lib.Info()
lib.fpsq_get_info(h, C.byref(i))
res["launches"] = i.last_kernel_launches
res["counters"] = [i.fuse_fallbacks, i.wait_timeouts, i.p2p_timeouts]
lib.fpsq_destroy(h)
print(json.dumps(res))
