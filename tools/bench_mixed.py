#!/usr/bin/env python3
"""fp64 against the opt-in mixed-precision cycle (somar_solver_set_precision mode 1) on BASELINE C2: 512^3, one box, Neumann
on all faces, pre/post/bottom 2/2/2, bench.py's residual (std::mt19937_64(12345), J-weighted mean removed), on the stretched
and on the Cartesian (all-ones) metric.  Per variant and mode: the depth-0 sweep (HIP-event time per k_gsrb_fused launch),
one V-cycle from zero, and full solves from zero to eps 1e-6 and 1e-10 (time, V-cycles, final / initial residual).  Prints
one JSON line.  Not the driver's bench (bench.py).

    python tools/bench_mixed.py [--n 512] [--cycles 20] [--min-cells 0] [--quick]
    --quick: one variant, a few cycles, no solves (for a rocprofv3 --kernel-trace --stats run of the fp32 kernels)
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# algorithmic B/cell of one red+black sweep: phi in / out, rhs, Jg x 3, Jinv; a uniform (Cartesian) metric streams no coefficients
SWEEP_BYTES = {("stretched", 0): 64.0, ("stretched", 1): 32.0, ("cartesian", 0): 24.0, ("cartesian", 1): 12.0}


def build(F, synthetic, n, variant, eps, imax):
    import numpy as np
    L = (1.0, 1.0, 1.0)
    dx = tuple(L[d] / n for d in range(3))
    s = F.AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, imax, eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define((0, 0, 0), (n - 1,) * 3, (False, False, False), dx, [((0, 0, 0), (n - 1,) * 3)])
    if variant == "stretched":
        jg, jinv = synthetic.stretched_diagonal_metric((0, 0, 0), (n - 1,) * 3, dx, L)
    else:
        jg = [np.ones((n + (d == 0), n + (d == 1), n + (d == 2)), order="F") for d in range(3)]
        jinv = np.ones((n, n, n), order="F")
    s.setMetricOrtho(0, jg[0], jg[1], jg[2], jinv)
    del jg, jinv
    s.finalize()
    return s


def upload_residual(s, F, field, which):
    import numpy as np
    s.upload(which, 0, np.asfortranarray(field), (0, 0, 0))
    s.removeMean(which)


def cycle_numbers(s, F, cycles):
    """(ms per depth-0 sweep, ms per V-cycle from zero)"""
    for _ in range(2):
        s.vcycleFromZero(F.F_CORR, F.F_RES)   # warm-up: graphs, first touch of the buffers
    s.profileEnable(True)
    s.vcycleFromZero(F.F_CORR, F.F_RES)
    n0, ms0 = s.profileGet(0)
    s.profileEnable(False)
    for _ in range(3):
        s.vcycleFromZero(F.F_CORR, F.F_RES)
    s.sync()
    t0 = time.perf_counter()
    for _ in range(cycles):
        s.vcycleFromZero(F.F_CORR, F.F_RES)
    s.sync()
    return ms0 / max(n0, 1), 1e3 * (time.perf_counter() - t0) / cycles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--min-cells", type=int, default=0)
    ap.add_argument("--quick", action="store_true")
    args = ap.parse_args()
    from somar_amd import api as F
    from somar_amd import synthetic
    n = args.n
    field = F.host_random_field((n, n, n), 12345)
    out = {"workload": "C2 %d^3, one box, Neumann, 2/2/2, bench.py residual: fp64 vs mixed (fp32 cycle on the large depths)" % n,
           "min_cells": args.min_cells}
    variants = ("stretched",) if args.quick else ("stretched", "cartesian")
    for variant in variants:
        rec = {}
        s = build(F, synthetic, n, variant, 1e-6, 100)
        upload_residual(s, F, field, F.F_RES)
        for mode in (0, 1):
            s.setPrecision(mode, args.min_cells)
            sweep, cyc = cycle_numbers(s, F, 3 if args.quick else args.cycles)
            rec[("fp64", "mixed")[mode]] = {"fp32_depths": s.precision()[1], "depth0_sweep_ms": sweep,
                                            "depth0_sweep_TBs": SWEEP_BYTES[(variant, mode)] * n ** 3 / (sweep * 1e-3) / 1e12,
                                            "vcycle_ms": cyc}
        s.undefine()
        if not args.quick:
            for eps in (1e-6, 1e-10):
                s = build(F, synthetic, n, variant, eps, 100)
                upload_residual(s, F, field, F.F_RHS)
                for mode in (0, 1):
                    s.setPrecision(mode, args.min_cells)
                    s.solveResident(zeroPhi=True)             # warm-up: graphs, first touch
                    s.sync()
                    t0 = time.perf_counter()
                    st = s.solveResident(zeroPhi=True)
                    s.sync()
                    rec[("fp64", "mixed")[mode]]["solve_eps%g" % eps] = {
                        "ms": 1e3 * (time.perf_counter() - t0), "iters": st["iters"], "exit_status": st["exitStatus"],
                        "final_over_initial": st["final_rnorm"] / st["initial_rnorm"]}
                s.undefine()
        m, d = rec["mixed"], rec["fp64"]
        rec["mixed_over_fp64"] = {"depth0_sweep": m["depth0_sweep_ms"] / d["depth0_sweep_ms"],
                                  "vcycle": m["vcycle_ms"] / d["vcycle_ms"]}
        for key in [k for k in m if k.startswith("solve_")]:
            rec["mixed_over_fp64"][key] = m[key]["ms"] / d[key]["ms"]
        out[variant] = rec
    print(json.dumps(out))


if __name__ == "__main__":
    main()
