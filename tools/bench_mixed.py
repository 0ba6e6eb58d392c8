#!/usr/bin/env python3
"""fp64 against the opt-in mixed-precision cycle (somar_solver_set_precision mode 1) on BASELINE C2: 512^3, one box, Neumann
on all faces, pre/post/bottom 2/2/2, bench.py's residual (std::mt19937_64(12345), J-weighted mean removed), on the stretched
and on the Cartesian (all-ones) metric.  Per variant and mode: the depth-0 sweep (HIP-event time per k_gsrb_fused launch),
one V-cycle from zero, and full solves from zero to eps 1e-6 and 1e-10 (time, V-cycles, final / initial residual).  Prints
one JSON line.  Not the driver's bench (bench.py).

    python tools/bench_mixed.py [--n 512] [--cycles 20] [--min-cells 0] [--quick]
    --quick: one variant, a few cycles, no solves (for a rocprofv3 --kernel-trace --stats run of the fp32 kernels)
    --ranks N (2 or 4): the same problem in bench.py's slab layout, one box per rank, N fresh child processes sharing ONE GPU
        over the host-staged shared-memory transport.  Per mode: fp32 depths, V-cycles to eps 1e-6 and 1e-10, payload bytes each
        rank sends per V-cycle (exchangeBytes: fp64, fp32), and a V-cycle time that is NOT a multi-GPU number (the wire is a
        host round trip and the ranks queue on one device).  A rehearsal of the sharded mixed cycle, as tools/rehearse_ranks.sh
        is of bench.py's N > 1 path.
"""
import argparse
import json
import os
import subprocess
import sys
import time
import uuid

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


SHM_LABEL = "ranks share one GPU over host-staged shm: not a multi-GPU number"


def build_sharded(F, synthetic, n, world, rank, comm, eps, imax):
    """bench.py's C2 layout: one slab per rank, stretched metric"""
    L = (1.0, 1.0, 1.0)
    dx = tuple(L[d] / n for d in range(3))
    boxes = synthetic.slab_partition(n, world)
    s = F.AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, imax, eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define((0, 0, 0), (n - 1,) * 3, (False, False, False), dx, boxes, owner=list(range(world)), comm=comm)
    for q in range(s.num_local_patches):
        lo, hi, _ = s.patch_box(q)
        jg, jinv = synthetic.stretched_diagonal_metric(lo, hi, dx, L)
        s.setMetricOrtho(q, jg[0], jg[1], jg[2], jinv)
    s.finalize()
    return s


def rank_main(args):
    """one rank of a --ranks run (a child process): prints its JSON line"""
    import numpy as np
    from somar_amd import api as F
    from somar_amd import synthetic
    n, world, rank = args.n, args.ranks, args.rank
    comm = F.comm_create_shm(args.shm_name, rank, world, 256 << 20)
    F.comm_selftest(comm)
    field = F.host_random_field((n, n, n), 12345)

    def upload(s, which):
        for q in range(s.num_local_patches):
            lo, hi, _ = s.patch_box(q)
            s.upload(which, q, np.asfortranarray(field[lo[0]:hi[0] + 1, lo[1]:hi[1] + 1, lo[2]:hi[2] + 1]), (0, 0, 0))
        s.removeMean(which)

    rec = {"rank": rank}
    s = build_sharded(F, synthetic, n, world, rank, comm, 1e-6, 100)
    upload(s, F.F_RES)
    for mode in (0, 1):
        s.setPrecision(mode, args.min_cells)
        for _ in range(2):
            s.vcycleFromZero(F.F_CORR, F.F_RES)
        b0 = s.exchangeBytes()
        s.vcycleFromZero(F.F_CORR, F.F_RES)
        b1 = s.exchangeBytes()
        s.sync()
        t0 = time.perf_counter()
        for _ in range(args.cycles):
            s.vcycleFromZero(F.F_CORR, F.F_RES)
        s.sync()
        rec[("fp64", "mixed")[mode]] = {"fp32_depths": s.precision()[1],
                                        "exchange_bytes_per_vcycle": {"fp64": b1[0] - b0[0], "fp32": b1[1] - b0[1]},
                                        "vcycle_ms": 1e3 * (time.perf_counter() - t0) / args.cycles,
                                        "vcycle_ms_label": SHM_LABEL,
                                        "overlapped_sweeps": s.counters()["overlapped_sweeps"]}
    s.undefine()
    for eps in (1e-6, 1e-10):
        s = build_sharded(F, synthetic, n, world, rank, comm, eps, 100)
        upload(s, F.F_RHS)
        for mode in (0, 1):
            s.setPrecision(mode, args.min_cells)
            st = s.solveResident(zeroPhi=True)
            rec[("fp64", "mixed")[mode]]["solve_eps%g" % eps] = {
                "iters": st["iters"], "exit_status": st["exitStatus"],
                "final_over_initial": st["final_rnorm"] / st["initial_rnorm"]}
        s.undefine()
    F.comm_destroy(comm)
    print(json.dumps(rec), flush=True)


def ranks_main(args):
    """the parent of a --ranks run: N fresh children, their JSON lines gathered into one"""
    name = "/somar_mixed_%s" % uuid.uuid4().hex[:12]
    cmd = [sys.executable, os.path.abspath(__file__), "--n", str(args.n), "--cycles", str(args.cycles), "--min-cells",
           str(args.min_cells), "--ranks", str(args.ranks), "--shm-name", name]
    procs = [subprocess.Popen(cmd + ["--rank", str(r)], stdout=subprocess.PIPE, text=True) for r in range(args.ranks)]
    recs, failed = [], False
    try:
        for p in procs:
            try:
                out, _ = p.communicate(timeout=args.timeout)
            except subprocess.TimeoutExpired:
                failed = True
                break
            lines = [ln for ln in out.splitlines() if ln.startswith("{")]
            if p.returncode != 0 or not lines:
                failed = True
                break
            recs.append(json.loads(lines[-1]))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
                p.wait()
    if failed:
        sys.exit("a rank failed or timed out (its peers were ended)")
    out = {"workload": "C2 %d^3, %d slabs on %d ranks (one GPU, shm transport), Neumann, 2/2/2, bench.py residual: fp64 vs "
                       "mixed" % (args.n, args.ranks, args.ranks), "min_cells": args.min_cells, "ranks": args.ranks,
           "note": SHM_LABEL, "per_rank": sorted(recs, key=lambda r: r["rank"])}
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--cycles", type=int, default=20)
    ap.add_argument("--min-cells", type=int, default=0)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--ranks", type=int, default=0, choices=(0, 2, 4))
    ap.add_argument("--rank", type=int, default=-1, help=argparse.SUPPRESS)        # (set by the parent of a --ranks run)
    ap.add_argument("--shm-name", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--timeout", type=float, default=900.0, help="seconds a --ranks run may take")
    args = ap.parse_args()
    if args.ranks:
        if args.rank >= 0:
            rank_main(args)
        else:
            ranks_main(args)
        return
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
