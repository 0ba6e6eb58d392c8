#!/usr/bin/env python3
"""Several components on one operator (somar_solver_set_components) against the same number of single-field calls on the same
handle, on the C2 geometry as a Helmholtz operator: 512^3, one box, stretched diagonal metric, Neumann on all faces,
alpha = 1, beta = -0.01, pre/post/bottom 2/2/2, one std::mt19937_64 residual per component.  The single-field calls are the
existing, unchanged path: they are the yardstick.  Per component count (2, 3, 4): the time of one 2/2/2 V-cycle from zero of
every component, batched (vcycleMulti) and sequential (vcycleFromZero, ncomp times), in interleaved rounds -- the spread of the
sequential rounds is what a difference has to beat -- and one complete solve to eps 1e-8, batched (solveMulti) and sequential.
Prints one JSON line.  Not the driver's bench (bench.py).

    python tools/bench_multi.py [--n 512] [--cycles 10] [--rounds 5] [--min-cells 0] [--quick]
    --min-cells: somar_solver_set_components' argument (0: the library's threshold)
    --quick: a few V-cycles of each kind and one solve, for a rocprofv3 --kernel-trace --stats run: the N-field kernels
        (k_gsrb_fused_nf, k_resid_march_nf) next to the single-field ones (k_gsrb_fused, k_resid_march) in one table
    --ops: 3 and 4 components that DIFFER in operator (somar_comp_set_op: free-slip walls on three, an all-Neumann scalar with
        another beta) on one handle against the same components on separate one-component handles: V-cycles and backward-Euler
        heat steps in interleaved rounds, the device memory of both arrangements; with --quick a few of each, for a kernel
        trace that shows k_gsrb_fused_nf / k_resid_march_nf on one operator per field (last template argument FieldOps<NF>)
        next to the separate handles' single-field launches
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ALPHA, BETA = 1.0, -0.01


def build(F, synthetic, n, eps, imax):
    L = (1.0, 1.0, 1.0)
    dx = tuple(L[d] / n for d in range(3))
    s = F.AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, imax, eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define((0, 0, 0), (n - 1,) * 3, (False, False, False), dx, [((0, 0, 0), (n - 1,) * 3)], alpha=ALPHA, beta=BETA)
    jg, jinv = synthetic.stretched_diagonal_metric((0, 0, 0), (n - 1,) * 3, dx, L)
    s.setMetricOrtho(0, jg[0], jg[1], jg[2], jinv)
    del jg, jinv
    s.finalize()
    return s


# --ops: components that differ in operator (somar_comp_set_op) on one handle against the same components on SEPARATE
# one-component handles, which is what they needed before: free-slip walls on three velocity components (the normal one
# Dirichlet, with wall values of its own) plus an all-Neumann scalar with another beta
# The create-time pair is (1, diffusivity), as a heat solver's: the heat steps scale it with dt, and for the V-cycles
# setAlphaAndBeta(1, BETA) turns it into the Helmholtz operators (1, -0.01) on the velocities and (1, -0.003) on the scalar.
D_, N_ = 1, 0
OPS = [([D_, D_, N_, N_, N_, N_], [0.25, -0.5, 0, 0, 0, 0], 1.0, 1.0),
       ([N_, N_, D_, D_, N_, N_], [0, 0, 0.75, 0.1, 0, 0], 1.0, 1.0),
       ([N_, N_, N_, N_, D_, D_], [0, 0, 0, 0, -0.3, 0.6], 1.0, 1.0),
       ([N_] * 6, [0.0] * 6, 1.0, 0.3)]


def build_op(F, synthetic, n, eps, imax, op):
    bc, values, alpha, beta = op
    L = (1.0, 1.0, 1.0)
    dx = tuple(L[d] / n for d in range(3))
    s = F.AMRPressureSolver()
    p = s._p
    s.setAMRMGParameters(p.imin, imax, eps, -1, p.num_smooth_precond, 2, 2, 2, p.precond_mode, 1, p.num_mg, p.hang,
                         p.norm_thresh, 0)
    s.define((0, 0, 0), (n - 1,) * 3, (False, False, False), dx, [((0, 0, 0), (n - 1,) * 3)], alpha=alpha, beta=beta, bc_type=bc)
    s.setBCValues(values)
    jg, jinv = synthetic.stretched_diagonal_metric((0, 0, 0), (n - 1,) * 3, dx, L)
    s.setMetricOrtho(0, jg[0], jg[1], jg[2], jinv)
    del jg, jinv
    s.finalize()
    return s


def run_ops(args, F, synthetic, np):
    n = args.n
    fields = [np.asfortranarray(F.host_random_field((n, n, n), 12345 + c)) for c in range(4)]
    out = {"workload": "C2 %d^3 as a Helmholtz operator, one box, stretched metric, 2/2/2: ncomp components with DIFFERENT "
                       "operators on one handle vs the same components on separate one-component handles" % n,
           "min_cells": args.min_cells, "ncomp": {}}
    reps = 2 if args.quick else args.cycles
    rounds = 1 if args.quick else args.rounds
    for nc in (3, 4):
        base = F.device_bytes_live()
        sep = [build_op(F, synthetic, n, 1e-8, 100, OPS[c]) for c in range(nc)]
        for c in range(nc):
            sep[c].upload(F.F_RES, 0, fields[c], (0, 0, 0))
        mem_sep = F.device_bytes_live() - base
        one = build_op(F, synthetic, n, 1e-8, 100, OPS[0])
        one.setComponents(nc, args.min_cells)
        for c in range(1, nc):
            one.setCompOp(c, *OPS[c])
        for c in range(nc):
            one.uploadComp(c, F.F_RES, 0, fields[c], (0, 0, 0))
        for s in sep + [one]:
            s.setAlphaAndBeta(1.0, BETA)
        mem_one = F.device_bytes_live() - base - mem_sep
        rec = {"batched_depths": one.getComponents()[1], "device_bytes_separate_handles": mem_sep, "device_bytes_one_handle": mem_one}

        def seq():
            for s in sep:
                s.vcycleFromZero(F.F_CORR, F.F_RES)

        def multi():
            one.vcycleMulti(True)

        def sync_all(fn, k):   # every handle has a stream of its own
            for s in sep + [one]:
                s.sync()
            t0 = time.perf_counter()
            for _ in range(k):
                fn()
            for s in sep + [one]:
                s.sync()
            return 1e3 * (time.perf_counter() - t0) / k

        for fn in (seq, multi):
            fn()
            fn()
        ts, tm = [], []
        for _ in range(rounds):
            ts.append(sync_all(seq, reps))
            for s in sep:
                s.sync()
            tm.append(sync_all(multi, reps))
        rec["vcycles_ms_separate"] = spread(ts)
        rec["vcycles_ms_one_handle"] = spread(tm)
        rec["one_handle_over_separate"] = statistics.median(tm) / statistics.median(ts)
        rec["separate_spread"] = (max(ts) - min(ts)) / statistics.median(ts)
        rec["n_field_launches"], rec["op_launches"] = one.getComponents()[2], one.opLaunches()
        # one backward-Euler heat step of every component, dt = 0.01 (the first pair is the warm-up)
        hs, hm = [], []
        try:
            heat_rounds(F, fields, nc, sep, one, rounds, sync_all, hs, hm, args.quick)
            rec["heat_step_ms_separate"] = spread(hs)
            rec["heat_step_ms_one_handle"] = spread(hm)
            rec["heat_one_handle_over_separate"] = statistics.median(hm) / statistics.median(hs)
        except F.SomarError as e:   # a solve that does not converge raises: recorded, and the rest is still measured
            rec["heat_step_error"] = str(e)
        out["ncomp"][str(nc)] = rec
        for s in sep + [one]:
            s.undefine()
    print(json.dumps(out))


def heat_rounds(F, fields, nc, sep, one, rounds, sync_all, hs, hm, tolerant):
    def quiet(fn):   # --quick (a kernel trace): a solve that reports failure has still run its launches
        try:
            fn()
        except F.SomarError:
            if not tolerant:
                raise

    for r in range(rounds + 1):
        for c in range(nc):
            sep[c].upload(F.F_HEAT_OLD, 0, fields[c], (0, 0, 0))
            sep[c].upload(F.F_HEAT_SRC, 0, fields[(c + 1) % 4], (0, 0, 0))
            one.uploadComp(c, F.F_HEAT_OLD, 0, fields[c], (0, 0, 0))
            one.uploadComp(c, F.F_HEAT_SRC, 0, fields[(c + 1) % 4], (0, 0, 0))
        a = sync_all(lambda: [quiet(lambda s=s: s.heatStep(0, 0.01, zeroPhi=True)) for s in sep], 1)
        b = sync_all(lambda: quiet(lambda: one.heatStepMulti(0, 0.01, zeroPhi=True)), 1)
        if r > 0:
            hs.append(a)
            hm.append(b)


def timed(s, fn, reps):
    s.sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    s.sync()
    return 1e3 * (time.perf_counter() - t0) / reps


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--cycles", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--min-cells", type=int, default=0)
    ap.add_argument("--quick", action="store_true")
    ap.add_argument("--ops", action="store_true")
    args = ap.parse_args()
    import numpy as np
    from somar_amd import api as F
    from somar_amd import synthetic
    if args.ops:
        run_ops(args, F, synthetic, np)
        return
    n = args.n
    fields = [np.asfortranarray(F.host_random_field((n, n, n), 12345 + c)) for c in range(4)]
    out = {"workload": "C2 %d^3 as a Helmholtz operator (alpha 1, beta -0.01), one box, stretched metric, Neumann, 2/2/2: "
                       "ncomp components batched vs ncomp single-field calls" % n, "min_cells": args.min_cells, "ncomp": {}}
    s = build(F, synthetic, n, 1e-8, 100)
    s.upload(F.F_RES, 0, fields[0], (0, 0, 0))
    base = F.device_bytes_live()
    for nc in (2, 3, 4):
        s.setComponents(nc, args.min_cells)
        for c in range(nc):
            s.uploadComp(c, F.F_RES, 0, fields[c], (0, 0, 0))
        rec = {"batched_depths": s.getComponents()[1], "device_bytes_per_extra_component": (F.device_bytes_live() - base) // (nc - 1)}

        def seq():
            for _ in range(nc):
                s.vcycleFromZero(F.F_CORR, F.F_RES)

        def multi():
            s.vcycleMulti(True)

        for fn in (seq, multi):   # warm-up: graphs, first touch of the buffers
            fn()
            fn()
        reps = 2 if args.quick else args.cycles
        ts, tm = [], []
        for _ in range(1 if args.quick else args.rounds):
            ts.append(timed(s, seq, reps))
            tm.append(timed(s, multi, reps))
        rec["vcycles_ms_sequential"] = spread(ts)
        rec["vcycles_ms_batched"] = spread(tm)
        rec["batched_over_sequential"] = statistics.median(tm) / statistics.median(ts)
        rec["sequential_spread"] = (max(ts) - min(ts)) / statistics.median(ts)
        out["ncomp"][str(nc)] = rec
    for nc in (3,):
        s.setComponents(nc, args.min_cells)
        rec = {}
        for label in ("sequential", "batched"):
            for rep in range(1 if args.quick else 2):   # the first is the warm-up
                for c in range(nc):
                    s.uploadComp(c, F.F_RHS, 0, fields[c], (0, 0, 0))
                if label == "batched":
                    s.sync()
                    t0 = time.perf_counter()
                    st = s.solveMulti(zeroPhi=True)
                    s.sync()
                    ms = 1e3 * (time.perf_counter() - t0)
                else:
                    st, ms = [], 0.0   # the uploads between the single-field solves are not timed
                    for c in range(nc):
                        s.upload(F.F_RHS, 0, fields[c], (0, 0, 0))
                        s.sync()
                        t0 = time.perf_counter()
                        st.append(dict(s.solveResident(zeroPhi=True)))
                        s.sync()
                        ms += 1e3 * (time.perf_counter() - t0)
            rec[label] = {"ms": ms, "iters": [x["iters"] for x in st],
                          "final_over_initial": [x["final_rnorm"] / x["initial_rnorm"] for x in st]}
        rec["batched_over_sequential"] = rec["batched"]["ms"] / rec["sequential"]["ms"]
        out["solve_3_components_eps1e-8"] = rec
    s.undefine()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
