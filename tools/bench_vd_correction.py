#!/usr/bin/env python3
"""Times one volume-discrepancy correction (somar_amr_vd_correction) on a hierarchy of tools/bench_amr.py, 1 GPU.

    python tools/bench_vd_correction.py --config c3 [--scale 1] [--reps 3]
    python tools/bench_vd_correction.py --config c3 --solve-only      # somar_amr_solve alone, same right-hand side

lambda = 1 + R / mult with R = -L_composite[hash-random phi] (covered cells zeroed), so the right-hand side
(lambda - 1) * mult is compatible.  After one warm-up call, HIP events (on the caller's stream, around blocking calls) time
  * the whole call,
  * its solve stage: the right-hand side, the zeroing and somar_amr_solve, issued as pieces,
  * its gradient stage: somar_amr_comp_gradient_mac,
and the levels' launch counters (somar_solver_counters) are compared between the solve inside the call and a plain
somar_amr_solve of the same right-hand side: they must be equal.  --solve-only needs nothing of the correction's interface: it
forms the same right-hand side with the same two rounded operations in torch and times somar_amr_solve alone.
Prints one JSON line."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c3")
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--box", type=int, default=128)
    ap.add_argument("--mult", type=float, default=0.3 / 0.07, help="lambda_mult = etaLambda / dt")
    ap.add_argument("--solve-only", action="store_true")
    args = ap.parse_args()
    import torch
    from bench_amr import build_hierarchy
    from somar_amd import api as F
    gpu, levels, cells, _, _, _ = build_hierarchy(args.config, args.scale, args.box)
    nlev = len(levels)
    lmax = nlev - 1
    g0 = (0, 0, 0)
    for l, v in enumerate(gpu.levels):
        v.fillHash(F.F_PHI, 12345 + l)
        v.setVal(F.F_RHS, 0.0)
    for ilev in range(nlev):
        gpu.residualLevel(lmax, 0, ilev)
    for l in range(lmax):
        gpu.zeroCovered(l, F.F_RES)
    lam = []
    for v in gpu.levels:
        t = [torch.empty(n, dtype=torch.float64, device="cuda") for n in v._dev_numel(ghost=g0)]
        v.downloadDev(F.F_RES, t, g0)
        lam.append([1.0 + x / args.mult for x in t])

    def counters():
        return [v.counters() for v in gpu.levels]

    def delta(a, b):
        return [{k: q[k] - p[k] for k in p} for p, q in zip(a, b)]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), out

    def plain_solve():
        """somar_amr_solve on (lambda - 1.0) * mult, formed here"""
        for l, v in enumerate(gpu.levels):
            v.uploadDev(F.F_RHS, [(x - 1.0) * args.mult for x in lam[l]], g0)
            v.setVal(F.F_PHI, 0.0)
        c0 = counters()
        ms, st = timed(lambda: dict(gpu.solveAMR(lmax, 0, zeroPhi=False)))
        return ms, st, delta(c0, counters())

    out = {"config": args.config, "scale": args.scale, "levels": nlev, "cells_per_level": cells, "lambda_mult": args.mult}
    plain_solve()   # warm-up
    runs = [plain_solve() for _ in range(args.reps)]
    out["amr_solve_ms"] = [round(r[0], 3) for r in runs]
    out["amr_solve_iters"] = runs[-1][1]["iters"]
    if not args.solve_only:
        def put_lambda():
            for l, v in enumerate(gpu.levels):
                v.uploadDev(F.F_RHS, lam[l], g0)

        put_lambda()
        gpu.vdCorrection(lmax, 0, args.mult)   # warm-up: builds the face tables
        whole, stage_solve, stage_grad = [], [], []
        for _ in range(args.reps):
            put_lambda()
            ms, st = timed(lambda: dict(gpu.vdCorrection(lmax, 0, args.mult)))
            whole.append(round(ms, 3))
            assert st["iters"] == runs[-1][1]["iters"] and st["history"] == runs[-1][1]["history"]
            # the same call as pieces
            put_lambda()
            c0 = counters()

            def solve_stage():
                for l in range(nlev):
                    gpu.vdRhs(l, args.mult)
                for v in gpu.levels:
                    v.setVal(F.F_PHI, 0.0)
                return dict(gpu.solveAMR(lmax, 0, zeroPhi=False))

            ms, st = timed(solve_stage)
            stage_solve.append(round(ms, 3))
            inside = delta(c0, counters())
            assert st["history"] == runs[-1][1]["history"]
            assert inside == runs[-1][2], (inside, runs[-1][2])
            ms, _ = timed(lambda: gpu.compGradientMAC(lmax, 0))
            stage_grad.append(round(ms, 3))
        out.update({"vd_correction_ms": whole, "vd_solve_stage_ms": stage_solve, "vd_gradient_stage_ms": stage_grad,
                    "solve_launch_counters_equal": True, "solve_launch_counters": runs[-1][2]})
    print(json.dumps(out))
    gpu.undefine()


if __name__ == "__main__":
    main()
