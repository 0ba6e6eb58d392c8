// somar_amd/csrc/box_io.hip -- copies between caller arrays in DEVICE memory (Fortran order, one array per local patch) and
// the level's patch layout: every local patch, and every component of a multi-component array, in ONE launch, either way.
//
// An item (BoxIoItem, one per patch and component) owns the tiles [tile0, next item's tile0): BIO_THREADS consecutive (i, j)
// pairs of the region's flattened i-j plane, times BIO_KC k-planes.  Flattening i and j puts consecutive lanes on consecutive
// i of one row and carries on into the next row, so a 12-wide box fills its wavefronts as a 512-wide one does; a wavefront
// touches at most two contiguous runs per array when the region is at least 32 wide, one when the array has no ghosts.
// 8 bytes per lane: the caller's rows start at any multiple of 8 bytes, so nothing wider is aligned.  A lane keeps its BIO_KC
// loads in flight before the first store.  No LDS, no barrier, no atomic; a workgroup reads its item and tile and nothing else.
#include "kernels.h"

namespace somar {

namespace {

struct BoxIoFields { double* f[3]; };

template <bool TO_LEVEL>
__global__ __launch_bounds__(BIO_THREADS) void k_box_io(const BoxIoItem* __restrict__ items, double* const* __restrict__ ptrs,
                                                        int nitems, const PatchDesc* __restrict__ patches, BoxIoFields F)
{
    const int t = blockIdx.x;
    // the last item whose first tile is <= t (items without tiles are not in the table, so tile0 is strictly increasing)
    int lo = 0, hi = nitems - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].tile0 <= t) lo = mid;
        else hi = mid - 1;
    }
    const BoxIoItem it = items[lo];
    double* const caller = ptrs[it.slot];
    if (!caller) return;   // a NULL entry skips its patch
    const PatchDesc p = patches[it.patch];
    const int lt = t - it.tile0;
    const int tk = lt / it.tiles_ij, tij = lt - tk * it.tiles_ij;
    const unsigned idx = (unsigned)tij * BIO_THREADS + threadIdx.x;
    if (idx >= (unsigned)it.n[0] * (unsigned)it.n[1]) return;
    const int j = (int)(idx / (unsigned)it.n[0]), i = (int)(idx - (unsigned)j * (unsigned)it.n[0]);
    const int k0 = tk * BIO_KC;
    const int nk = min(BIO_KC, it.n[2] - k0);
    const long long co = it.coff + (long long)(it.rlo[0] - it.clo[0] + i) + (long long)it.cpj * (it.rlo[1] - it.clo[1] + j) +
                         it.cpk * (long long)(it.rlo[2] - it.clo[2] + k0);
    const long long lo_ = p.off + (long long)(it.rlo[0] - p.lo[0] + i) + (long long)p.pj * (it.rlo[1] - p.lo[1] + j) +
                          p.pk * (long long)(it.rlo[2] - p.lo[2] + k0);
    double* const field = F.f[it.comp];
    const double* src = TO_LEVEL ? caller + co : field + lo_;
    double* dst = TO_LEVEL ? field + lo_ : caller + co;
    const long long spk = TO_LEVEL ? it.cpk : p.pk, dpk = TO_LEVEL ? p.pk : it.cpk;
    double v[BIO_KC];
#pragma unroll
    for (int q = 0; q < BIO_KC; ++q)
        if (q < nk) v[q] = src[q * spk];
#pragma unroll
    for (int q = 0; q < BIO_KC; ++q)
        if (q < nk) dst[q * dpk] = v[q];
}

}  // namespace

void launch_box_io(hipStream_t st, const LevelDev& L, const BoxIoItem* items, double* const* ptrs, int nitems, int ntiles,
                   double* const field[3], bool to_level)
{
    if (nitems <= 0 || ntiles <= 0) return;
    BoxIoFields F{{field[0], field[1], field[2]}};
    if (to_level) hipLaunchKernelGGL(k_box_io<true>, dim3(ntiles), dim3(BIO_THREADS), 0, st, items, ptrs, nitems, L.patches, F);
    else hipLaunchKernelGGL(k_box_io<false>, dim3(ntiles), dim3(BIO_THREADS), 0, st, items, ptrs, nitems, L.patches, F);
    SOMAR_HIP(hipGetLastError());
}

}  // namespace somar
