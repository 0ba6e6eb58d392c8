#!/usr/bin/env python3
"""Metric refresh against re-definition, 1 GPU.

    python tools/bench_metric_refresh.py --config c4 [--scale 1] [--reps 3] [--refresh-only N]

Builds the hierarchy of tools/bench_amr.py (c4: Cartesian, the metric written by setMetricUniform; c5: the terrain-
following non-diagonal metric written by setMetricMap(BATHYMETRIC)), then alternates, --reps times:
  redefine: destroy + create + metric producers + finalize (what an adapter pays today for a new metric)
  refresh:  metricUpdate() begin + the same producers + end, on the hierarchy as it stands
and prints one JSON line with the wall times (each step ends with a device synchronisation); the refresh is also split into
its producers (begin + the set_metric_* calls, host-side map inputs included) and its end (the recomputation).
SOMAR_TIMING=1 adds the library's per-stage breakdown of finalize and of the refresh on stderr.  --refresh-only N runs N
refreshes and nothing else after the build (for a kernel trace of the refresh alone)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def produce(gpu, config):
    """the producers bench_amr.build_hierarchy runs, on every level (device-side producers only)"""
    from somar_amd import api as F
    from somar_amd import synthetic
    if config != "c5":
        for v in gpu.levels:
            v.setMetricUniform(1.0, 1.0, 1.0, 1.0)
        return
    H = synthetic.c5_hierarchy(produce.scale, 64, 1)
    dxl = list(H["dx0"])
    for l, v in enumerate(gpu.levels):
        if l > 0:
            dxl = [a / b for a, b in zip(dxl, H["ratios"][l - 1])]
        if not v.num_local_patches:
            continue
        bx = [v.patch_box(q) for q in range(v.num_local_patches)]
        nlo = [min(b[0][d] for b in bx) - 1 for d in range(2)]
        nhi = [max(b[1][d] for b in bx) + 2 for d in range(2)]
        v.setMetricMap(F.MAP_BATHYMETRIC, H["L"], synthetic.terrain_nodal_depth(nlo, nhi, dxl, H["L"]), nlo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="c4", choices=["c3", "c4", "c5"])
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--refresh-only", type=int, default=0)
    a = ap.parse_args()
    import bench_amr
    produce.scale = a.scale
    box = 64 if a.config == "c5" else 128
    gpu, levels, cells, _, _, _ = bench_amr.build_hierarchy(a.config, a.scale, box)
    if a.refresh_only:
        for _ in range(a.refresh_only):
            with gpu.metricUpdate():
                produce(gpu, a.config)
        gpu.levels[0].sync()
        gpu.undefine()
        return
    from somar_amd import api as F
    redefine, refresh, producers, ends = [], [], [], []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        gpu.undefine()
        gpu, levels, cells, _, _, _ = bench_amr.build_hierarchy(a.config, a.scale, box)
        gpu.levels[0].sync()
        redefine.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        F._ck(F.lib().somar_amr_metric_update_begin(gpu._amr))
        produce(gpu, a.config)
        gpu.levels[0].sync()
        t1 = time.perf_counter()
        F._ck(F.lib().somar_amr_metric_update_end(gpu._amr))
        gpu.levels[0].sync()
        t2 = time.perf_counter()
        refresh.append(t2 - t0)
        producers.append(t1 - t0)
        ends.append(t2 - t1)
    gpu.undefine()
    r = lambda v: [round(x, 4) for x in v]   # noqa: E731
    print(json.dumps({"config": a.config, "scale": a.scale, "cells": cells, "redefine_s": r(redefine), "refresh_s": r(refresh),
                      "refresh_producers_s": r(producers), "refresh_end_s": r(ends),
                      "ratio_best": round(min(redefine) / min(refresh), 1)}))


if __name__ == "__main__":
    main()
