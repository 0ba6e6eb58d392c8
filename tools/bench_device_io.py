#!/usr/bin/env python3
"""Field I/O of a device-resident caller (somar_field_upload_dev / _download_dev) against a bare device-to-device copy, a
per-patch hipMemcpy3DAsync loop, and the host path, 1 GPU.

    python tools/bench_device_io.py [--shape c2|c3|both] [--scale 1] [--reps 10]

Shapes: c2 = one 512^3 box (bench.py's flagship); c3 = the refined level of BASELINE C3 cut into 64-wide boxes
(512 x 1024 x 64 cells, 128 boxes; tools/bench_amr.py --config c3 --box 64).  --scale divides every extent.
Per shape and ghost width (0 and 1), for SOMAR_F_PHI:
  (a) uploadDev / downloadDev: one box-I/O launch for all patches (csrc/box_io.hip), the binding's tensor checks, the
      library's pointer checks and the drain included; and the C entry points alone on a pointer table built once
  (b) one hipMemcpyAsync device-to-device of the same number of bytes (the caller's arrays back to back)
  (d) a per-patch hipMemcpy3DAsync device-to-device loop into a buffer shaped like the level's (2-cell frame, even pitch)
  (c) the host path: somar_field_upload / _download per patch from pageable numpy arrays
GB/s counts 16 B per cell of the caller's arrays and direction (8 read + 8 written).  Times are host clocks around calls that
end in a drained stream; median of --reps after two warm-up calls (the host path: of 3 after one).
Prints one JSON line per shape and ghost width."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np  # noqa: E402

FRAME = 2


class Pos(C.Structure):
    _fields_ = [("x", C.c_size_t), ("y", C.c_size_t), ("z", C.c_size_t)]


class PitchedPtr(C.Structure):
    _fields_ = [("ptr", C.c_void_p), ("pitch", C.c_size_t), ("xsize", C.c_size_t), ("ysize", C.c_size_t)]


class Extent(C.Structure):
    _fields_ = [("width", C.c_size_t), ("height", C.c_size_t), ("depth", C.c_size_t)]


class Memcpy3DParms(C.Structure):   # hipMemcpy3DParms, hip/driver_types.h
    _fields_ = [("srcArray", C.c_void_p), ("srcPos", Pos), ("srcPtr", PitchedPtr), ("dstArray", C.c_void_p), ("dstPos", Pos),
                ("dstPtr", PitchedPtr), ("extent", Extent), ("kind", C.c_int)]


D2D = 3   # hipMemcpyDeviceToDevice


def hip_runtime():
    """the HIP runtime this process already runs on (torch's copy; a second one would find no device)"""
    for line in open("/proc/self/maps"):
        path = line.split()[-1]
        if os.path.basename(path).startswith("libamdhip64.so"):
            hip = C.CDLL(path)
            hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
            hip.hipMemcpy3DAsync.argtypes = [C.POINTER(Memcpy3DParms), C.c_void_p]
            return hip
    raise SystemExit("no libamdhip64 loaded in this process")


def median_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t), min(t)


def build(shape, scale):
    """-> (owner to undefine, the level's solver view)"""
    from somar_amd import api as F
    if shape == "c2":
        n = 512 // scale
        s = F.AMRPressureSolver()
        s.define((0, 0, 0), (n - 1, n - 1, n - 1), (False, True, False), (1.0 / n,) * 3, [((0, 0, 0), (n - 1, n - 1, n - 1))])
        s.setMetricUniform(1.0, 1.0, 1.0, 1.0)
        s.finalize()
        return s, s
    import bench_amr
    gpu = bench_amr.build_hierarchy("c3", scale, box=64)[0]
    return gpu, gpu.levels[1]


def measure(torch, hip, v, ghost, reps):
    from somar_amd import api as F
    npatch = v.num_local_patches
    boxes = [v.patch_box(p)[:2] for p in range(npatch)]
    valid = [tuple(h - l + 1 for l, h in zip(lo, hi)) for lo, hi in boxes]
    shapes = [tuple(n + 2 * g for n, g in zip(nv, ghost)) for nv in valid]
    numel = [int(np.prod(s)) for s in shapes]
    total = sum(numel)
    flat = torch.rand(total, dtype=torch.float64, device="cuda")
    off = np.concatenate([[0], np.cumsum(numel)])
    tens = [flat[off[p]:off[p + 1]] for p in range(npatch)]
    out = {"patches": npatch, "cells": total, "ghost": list(ghost), "box_i": valid[0][0]}

    def sync():
        torch.cuda.synchronize()

    # (a) the library: it synchronises torch's stream, launches once and drains its own
    up = median_ms(lambda: v.uploadDev(F.F_PHI, tens, ghost), reps, 2)
    dn = median_ms(lambda: v.downloadDev(F.F_PHI, tens, ghost), reps, 2)
    # ... and the library call alone, on a table built once (what a C caller pays: pointer checks, launch, drain)
    tab = (C.c_void_p * npatch)(*[t.data_ptr() for t in tens])
    g3 = F._ia(ghost)
    lib_up = median_ms(lambda: F._ck(F.lib().somar_field_upload_dev(v._h, F.F_PHI, tab, g3)), reps, 2)
    lib_dn = median_ms(lambda: F._ck(F.lib().somar_field_download_dev(v._h, F.F_PHI, tab, g3)), reps, 2)
    # (b) one bare device-to-device copy of the same bytes
    other = torch.empty_like(flat)

    def bare():
        assert hip.hipMemcpyAsync(other.data_ptr(), flat.data_ptr(), total * 8, D2D, None) == 0
        sync()
    cp = median_ms(bare, reps, 2)
    # (d) per patch, one 3-D copy into a framed buffer shaped like the level's arrays
    frames = [(-(-(n[0] + 2 * FRAME) // 2) * 2, n[1] + 2 * FRAME, n[2] + 2 * FRAME) for n in valid]
    fnum = [int(np.prod(f)) for f in frames]
    foff = np.concatenate([[0], np.cumsum(fnum)])
    framed = torch.zeros(int(foff[-1]), dtype=torch.float64, device="cuda")
    parms = []
    for p in range(npatch):
        q = Memcpy3DParms()
        q.srcPtr = PitchedPtr(tens[p].data_ptr(), shapes[p][0] * 8, shapes[p][0], shapes[p][1])
        q.dstPtr = PitchedPtr(framed.data_ptr() + int(foff[p]) * 8, frames[p][0] * 8, frames[p][0], frames[p][1])
        q.dstPos = Pos((FRAME - ghost[0]) * 8, FRAME - ghost[1], FRAME - ghost[2])
        q.extent = Extent(shapes[p][0] * 8, shapes[p][1], shapes[p][2])
        q.kind = D2D
        parms.append(q)

    def loop3d():
        for q in parms:
            assert hip.hipMemcpy3DAsync(C.byref(q), None) == 0
        sync()
    lp = median_ms(loop3d, reps, 2)
    # (c) the host path
    host = [np.asfortranarray(np.random.default_rng(p).random(shapes[p])) for p in range(npatch)]

    def host_up():
        for p in range(npatch):
            v.upload(F.F_PHI, p, host[p], ghost)

    def host_dn():
        for p in range(npatch):
            F._ck(F.lib().somar_field_download(v._h, F.F_PHI, p, F._dp(host[p]), F._ia(ghost)))
    hu = median_ms(host_up, 3, 1)
    hd = median_ms(host_dn, 3, 1)
    # what was timed moves the right data: the device path's download equals the host path's
    v.uploadDev(F.F_PHI, tens, ghost)
    host_dn()
    for p in (0, npatch - 1):
        assert np.array_equal(host[p].ravel(order="F"), tens[p].cpu().numpy())

    gb = total * 16 / 1e9
    for name, (med, lo) in (("a_upload_dev", up), ("a_download_dev", dn), ("a_upload_dev_c_abi", lib_up),
                            ("a_download_dev_c_abi", lib_dn), ("b_memcpy_d2d", cp), ("d_memcpy3d_loop", lp),
                            ("c_host_upload", hu), ("c_host_download", hd)):
        out[name] = {"ms": round(med, 4), "ms_min": round(lo, 4), "GBps": round(gb / (med * 1e-3), 1)}
    a = (up[0] + dn[0]) / 2
    out["a_over_b"] = round(a / cp[0], 3)
    out["c_over_a"] = round((hu[0] + hd[0]) / 2 / a, 1)
    out["d_over_a"] = round(lp[0] / a, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="both", choices=["c2", "c3", "both"])
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_io needs a GPU")
    from somar_amd import api as F
    F.lib()
    hip = hip_runtime()
    for shape in (["c2", "c3"] if args.shape == "both" else [args.shape]):
        owner, v = build(shape, args.scale)
        for ghost in ((0, 0, 0), (1, 1, 1)):
            r = measure(torch, hip, v, ghost, args.reps)
            r.update({"shape": shape, "scale": args.scale, "reps": args.reps})
            print(json.dumps(r), flush=True)
        owner.undefine()
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
