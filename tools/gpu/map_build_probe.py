"""Probe of the map build (lvk_map_build) for a kernel trace and for wall times against the numpy judge it replaces.

    python tools/gpu/map_build_probe.py kernels     six calls each at 65,536 and at 1,048,576 points, de-duplication off and on; run it behind
                                                    `rocprofv3 --kernel-trace --stats --` for the kernel times of DESIGN.md 5.0i
    python tools/gpu/map_build_probe.py wall        per size and mode: the wall time of the stage entry on device-resident arrays (its launches
                                                    and one wait, uploads left out; six calls behind a warm-up), and of the numpy judge's
                                                    sort-and-cull (tests/map_build_ref.build) on the same input, once; both answers must agree
The input has a realistic density: three quarters of the points uniform in a cube sized for about three points per r_dup cell, a quarter
near copies of them (moved by less than r_dup / 4, one descriptor bit inverted); the score is the covariance's trace.  Prints one JSON line."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import larvio_amd                                             # noqa: E402
from larvio_amd import ops                                    # noqa: E402
from larvio_amd._lib import lib, _p, MAP_BUILD_INFO           # noqa: E402

R_DUP = 0.05
SIZES = (65536, 1 << 20)


def staged(n, seed=1):
    rng = np.random.default_rng(seed)
    m = n - n // 4
    side = R_DUP * (n / 3.0) ** (1.0 / 3.0)
    X = rng.uniform(0.0, side, (m, 3)) - 0.5 * side
    d = rng.integers(0, 256, (m, 32), dtype=np.uint8)
    src = rng.integers(0, m, n // 4)
    Xc = X[src] + rng.uniform(-1.0, 1.0, (n // 4, 3)) * (R_DUP / 8.0)
    dc = d[src].copy(); bit = rng.integers(0, 256, n // 4)
    dc[np.arange(n // 4), bit // 8] ^= (1 << (bit % 8)).astype(np.uint8)
    p = rng.permutation(n)
    A = rng.normal(0.0, 1.0, (n, 3, 3))
    cov = 1e-3 * (A @ A.transpose(0, 2, 1)) + 1e-6 * np.eye(3)
    return np.concatenate([X, Xc])[p], cov, np.concatenate([d, dc])[p]


class Call:
    """lvk_map_build on device-resident inputs and outputs"""

    def __init__(self, ctx, X, cov, desc):
        self.ctx, self.n = ctx, len(X)
        self.d_in = [ctx.to_device(a) for a in (X, cov.reshape(-1, 9), desc)]
        self.d_out = [ctx.alloc(s * self.n) for s in (4, 24, 72, 32, 1)] + [ctx.alloc(MAP_BUILD_INFO.itemsize)]

    def run(self, r_dup):
        o = ops.map_build_options(r_dup=r_dup)
        self.ctx.check(lib().lvk_map_build(self.ctx.h, _p(self.d_in[0]), _p(self.d_in[1]), _p(self.d_in[2]), None, self.n, C.byref(o), *[_p(b) for b in self.d_out]))
        self.ctx.sync()

    def info(self):
        return self.ctx.to_host(self.d_out[5], MAP_BUILD_INFO, (1,))[0]


def kernels():
    ctx = larvio_amd.Context(0)
    out = {}
    for n in SIZES:
        call = Call(ctx, *staged(n))
        for r_dup in (0.0, R_DUP):
            for _ in range(6):
                call.run(r_dup)
            out[f"n_kept_{n}_{'dedup' if r_dup else 'sort'}"] = int(call.info()["n_kept"])
    ctx.close()
    return out


def wall():
    from tests import map_build_ref as R
    ctx = larvio_amd.Context(0)
    out = dict(r_dup=R_DUP)
    for n in SIZES:
        X, cov, desc = staged(n)
        call = Call(ctx, X, cov, desc)
        for r_dup in (0.0, R_DUP):
            tag = f"{n}_{'dedup' if r_dup else 'sort'}"
            call.run(r_dup)
            times = []
            for _ in range(6):
                t0 = time.perf_counter(); call.run(r_dup); times.append(time.perf_counter() - t0)
            info = call.info()
            t0 = time.perf_counter(); ref = R.build(X, cov, desc, None, r_dup=r_dup); t_ref = time.perf_counter() - t0
            order = ctx.to_host(call.d_out[0], np.int32, (int(info["n_kept"]),))
            assert info.tobytes() == ref["info"].tobytes() and order.tobytes() == ref["order"].tobytes(), tag
            out[tag] = dict(device_ms=[round(1e3 * t, 3) for t in times], judge_ms=round(1e3 * t_ref, 1), n_kept=int(info["n_kept"]), n_duplicate=int(info["n_duplicate"]))
    ctx.close()
    return out


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "kernels"
    print(json.dumps({"mode": mode, **(kernels() if mode == "kernels" else wall())}))
