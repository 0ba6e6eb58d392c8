// somar_amd/csrc/metric_refresh.hip -- batched setup kernels of a metric refresh (PressureSolver::refresh_metric):
//   k_coarsen_metric: every coarse metric array of one MG depth in ONE launch (fill_MGfields, MappedAMRPoissonOpFactory.cpp:
//                     1164-1234), instead of one k_avg_face launch per patch x direction x component plus k_avg_harmonic
//   k_minmax_all:     (min, max) of every array the uniform-metric / zero-plane detection looks at, every depth, ONE launch
#include "kernels.h"

namespace somar {

// One workgroup = 4 wavefronts = 4 consecutive coarse j-rows of one k-plane of one work item.  A wavefront covers 64 coarse
// entries of its row at a time.  Where a coarse entry averages a run of r0 > 1 fine entries along i (every face direction
// but 0, and the harmonic cell average), the wavefront first loads the 64 * r0 fine entries it needs as contiguous runs into
// LDS, then every lane adds its own r0 values from there.  The summation order is k_avg_face's / k_avg_harmonic's
// (ii2, ii1, ii0 nesting, then the refScale product), so the results are the same bits.
constexpr int CM_WAVES = 4;
constexpr int CM_MAXR = 4;   // LDS runs for r0 <= CM_MAXR; a larger r0 reads strided (no MG depth here coarsens by more)

__global__ __launch_bounds__(256) void k_coarsen_metric(const CoarsenItem* __restrict__ items,
                                                        const PatchDesc* __restrict__ cpatches,
                                                        const PatchDesc* __restrict__ fpatches, int r0, int r1, int r2)
{
    __shared__ double buf[CM_WAVES][64 * CM_MAXR];
    const CoarsenItem it = items[blockIdx.x];
    const PatchDesc cp = cpatches[it.patch];
    const PatchDesc fp = fpatches[it.patch];
    const int dir = it.dir;   // -1: harmonic cell average
    const int ni = cp.n[0] + (dir == 0), nj = cp.n[1] + (dir == 1), nk = cp.n[2] + (dir == 2);
    const int b0 = dir == 0 ? 1 : r0, b1 = dir == 1 ? 1 : r1, b2 = dir == 2 ? 1 : r2;
    const int rr[3] = {r0, r1, r2};
    const double refScale = dir < 0 ? 1.0 / (double)(r0 * r1 * r2) : (double)rr[dir] / (double)(r0 * r1 * r2);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const bool staged = b0 > 1 && b0 <= CM_MAXR;
    const int njg = (nj + CM_WAVES - 1) / CM_WAVES;
    const long long groups = (long long)njg * nk;
    // every loop bound below is uniform over the workgroup (the barriers inside are reached by all four wavefronts)
    for (long long g = blockIdx.y; g < groups; g += gridDim.y) {
        const int lk = (int)(g / njg);
        const int lj = (int)(g - (long long)lk * njg) * CM_WAVES + w;
        const bool row = lj < nj;
        for (int seg = 0; seg < ni; seg += 64) {
            const int li = seg + lane;
            const int nseg = ni - seg < 64 ? ni - seg : 64;
            double s = 0.0;
            for (int ii2 = 0; ii2 < b2; ++ii2)
                for (int ii1 = 0; ii1 < b1; ++ii1) {
                    const double* frow = it.fine + fp.off + (long long)fp.pj * (lj * r1 + ii1) + fp.pk * (long long)(lk * r2 + ii2);
                    if (staged) {
                        const int nf = nseg * b0;   // fine entries seg * r0 .. seg * r0 + nf - 1, contiguous
                        if (row)
                            for (int q = lane; q < nf; q += 64) buf[w][q] = frow[seg * r0 + q];
                        __syncthreads();
                        if (row && lane < nseg)
                            for (int ii0 = 0; ii0 < b0; ++ii0) {
                                const double v = buf[w][lane * b0 + ii0];
                                s = dir < 0 ? s + 1.0 / v : s + v;
                            }
                        __syncthreads();
                    } else if (row && lane < nseg) {
                        for (int ii0 = 0; ii0 < b0; ++ii0) {
                            const double v = frow[li * r0 + ii0];
                            s = dir < 0 ? s + 1.0 / v : s + v;
                        }
                    }
                }
            if (row && lane < nseg)
                it.crse[cp.off + li + (long long)cp.pj * lj + cp.pk * (long long)lk] = dir < 0 ? 1.0 / (s * refScale) : refScale * s;
        }
    }
}

void launch_coarsen_metric(hipStream_t st, const LevelDev& C, const LevelDev& F, const CoarsenItem* items, int nitems,
                           int gy, const int r[3])
{
    if (nitems == 0) return;
    hipLaunchKernelGGL(k_coarsen_metric, dim3(nitems, gy), dim3(64 * CM_WAVES), 0, st, items, C.patches, F.patches, r[0], r[1],
                       r[2]);
}

// min / max of a table of (array, patch table, patch, dir) items, MM_CH chunks of k-planes per item: out[2 * (item * MM_CH +
// chunk)] = min, [... + 1] = max over the valid cells (dir < 0) or the valid dir-faces, +-inf for an empty chunk.  Runs at
// finalize and at every metric refresh (PressureSolver::detect_metric_flags).
__global__ __launch_bounds__(256) void k_minmax_all(const MinMaxItem* __restrict__ items, double* __restrict__ out)
{
    const MinMaxItem it = items[blockIdx.x];
    const PatchDesc p = it.patches[it.patch];
    const int dir = it.dir;
    const int n0 = p.n[0] + (dir == 0), n1 = p.n[1] + (dir == 1), n2 = p.n[2] + (dir == 2);
    const int per = (n2 + MM_CH - 1) / MM_CH;
    const int k0 = per * blockIdx.y, k1 = k0 + per < n2 ? k0 + per : n2;
    double lo = HUGE_VAL, hi = -HUGE_VAL;
    for (int k = k0; k < k1; ++k)
        for (int j = threadIdx.y; j < n1; j += 4) {
            const double* row = it.a + p.off + (long long)p.pj * j + p.pk * k;
            for (int i = threadIdx.x; i < n0; i += 64) {
                const double v = row[i];
                lo = v < lo ? v : lo;
                hi = v > hi ? v : hi;
            }
        }
    __shared__ double slo[256], shi[256];
    const int t = threadIdx.x + 64 * threadIdx.y;
    slo[t] = lo;
    shi[t] = hi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            slo[t] = slo[t + s] < slo[t] ? slo[t + s] : slo[t];
            shi[t] = shi[t + s] > shi[t] ? shi[t + s] : shi[t];
        }
        __syncthreads();
    }
    if (t == 0) {
        const long long o = 2 * ((long long)blockIdx.x * MM_CH + blockIdx.y);
        out[o] = slo[0];
        out[o + 1] = shi[0];
    }
}

void launch_minmax_all(hipStream_t st, const MinMaxItem* items, int nitems, double* out)
{
    if (nitems) hipLaunchKernelGGL(k_minmax_all, dim3(nitems, MM_CH), dim3(64, 4), 0, st, items, out);
}

}  // namespace somar
