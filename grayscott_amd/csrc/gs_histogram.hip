// gs_histogram.hip -- histograms of planes on the device (include/gs_hip.h: gs_fields_histogram, gs_members_histogram).
//
// gs_plane_hist_k counts every cell of a plane into one of bins + 3 slots -- counts[0, bins), below, above, nan, by the rule
// of gs_hip.h -- in u32 words of LDS shared by the workgroup, and adds the slots that are not zero to the plane's u64
// counters in global memory once, at its end.  Counts are integers: no order matters, so neither the launch shape nor the
// slab layout shows in the result.
//
// Reading: as gs_row_summary_k does -- a wave owns a row at a time, its lanes read 16 B each, eight loads ahead of their use.
// Counting (gs_hist_count.h: slot_of and count, shared with gs_region_hist.hip): for each of the wave's loads of 64 cells the slot of the first lane is broadcast (readfirstlane), the lanes that
// hold the same slot are counted with one ballot, and only the OTHER lanes add 1 to their slot in LDS.  What the first
// lane's slot gained goes to a run kept in scalar registers -- (slot, count) -- which is written to LDS when another slot
// takes over.  On one-valued data (Species::new, and everything off the pattern: U exactly 1, V exactly 0) a wave so issues
// no LDS atomic per load at all, and where a pattern begins the background value of a wave still costs none; without this all
// 64 lanes would add to one word, and adds to one address are served one after the other.  All of it is wave-uniform control
// flow: the loop bounds are scalar, and a column outside the row counts into a spare slot that nobody reads.
//
// Built with hipcc's default float mode (f32 denormals kept) and -ffp-contract=off, as gs_summary.hip is: the rule's
// subtraction and multiplication are one f32 operation each, and a sub-normal cell or product is the value it is.
#include "gs_kernels.h"
#include "gs_hist_count.h"
#include "gs_plane_scan.h"

namespace {

constexpr int kHistUnroll = 8;        // blocks of 256 columns whose loads a wave issues before it counts them
constexpr int kHistSegment = 1 << 20; // columns of a row that make one unit of work (a multiple of 256 * kHistUnroll)
// A workgroup takes at most kHistUnitsPerGroup units (the launcher sizes the grid for it) of at most kHistSegment cells
// each between zeroing its LDS words and flushing them: 2^11 * 2^20 = 2^31 cells, so no u32 word can wrap whatever the
// plane -- the spare slot included, which gains fewer than 2048 per unit.
constexpr int64_t kHistUnitsPerGroup = 2048;

struct GsHistArgs {
    float lo[4], hi[4], scale[4]; // per set.p[]
    GsPlaneSet set;
    int32_t bins;
    int64_t groups;      // workgroups per plane
    unsigned long long *out; // [planes][bins + 3], zeroed by the caller
};

// 1-D grid of planes x groups workgroups of 4 waves; dynamic LDS: (bins + 4) u32.
template <bool VEC>
__global__ __launch_bounds__(256) void gs_plane_hist_k(GsHistArgs a)
{
    extern __shared__ unsigned h[];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int bins = a.bins, slots = bins + 4;
    const int64_t y = (int64_t)blockIdx.x / a.groups, g = (int64_t)blockIdx.x % a.groups;
    int which;
    const float *plane = gs_plane_at(a.set, y, which);
    const float lo = a.lo[which], hi = a.hi[which], scale = a.scale[which];
    for (int i = (int)threadIdx.x; i < slots; i += 256) h[i] = 0u;
    __syncthreads();

    const int cols = a.set.cols;
    const int64_t segs = ((int64_t)cols + kHistSegment - 1) / kHistSegment, units = a.set.rows * segs;
    Run run{bins + 3, 0};
    for (int64_t u = g * 4 + wave; u < units; u += a.groups * 4) {
        // the unit: columns [0, c_end) of `row`, which begins at the segment's first column (a multiple of 2^20)
        const float *row = plane + (u / segs) * a.set.pitch + (u % segs) * kHistSegment;
        const int64_t left = (int64_t)cols - (u % segs) * kHistSegment;
        const int c_end = (int)(left < kHistSegment ? left : kHistSegment);
        for (int base = 0; base < c_end; base += 256 * kHistUnroll) { // (scalar: no lane leaves early)
            float4 x[kHistUnroll];
            const int c0 = base + 4 * lane;
#pragma unroll
            for (int k = 0; k < kHistUnroll; ++k) {
                const int c = c0 + 256 * k;
                if (VEC && c + 3 < c_end) {
                    x[k] = *reinterpret_cast<const float4 *>(row + c);
                } else { // (a column outside the row reads the row's last cell instead -- c_end > base >= 0 -- and is not counted)
                    const int last = c_end - 1;
                    x[k].x = row[c < last ? c : last];
                    x[k].y = row[c + 1 < last ? c + 1 : last];
                    x[k].z = row[c + 2 < last ? c + 2 : last];
                    x[k].w = row[c + 3 < last ? c + 3 : last];
                }
            }
#pragma unroll
            for (int k = 0; k < kHistUnroll; ++k) {
                const int c = c0 + 256 * k;
                if (base + 256 * k >= c_end) break; // (scalar) no lane of the wave has a column here
                count(h, run, slot_of(x[k].x, c < c_end, lo, hi, scale, bins), lane);
                count(h, run, slot_of(x[k].y, c + 1 < c_end, lo, hi, scale, bins), lane);
                count(h, run, slot_of(x[k].z, c + 2 < c_end, lo, hi, scale, bins), lane);
                count(h, run, slot_of(x[k].w, c + 3 < c_end, lo, hi, scale, bins), lane);
            }
        }
    }
    if (lane == 0) atomicAdd(&h[run.slot], (unsigned)run.n);
    __syncthreads();
    unsigned long long *out = a.out + y * (int64_t)(bins + 3);
    for (int i = (int)threadIdx.x; i < bins + 3; i += 256) {
        const unsigned n = h[i];
        if (n) atomicAdd(&out[i], (unsigned long long)n);
    }
}

} // namespace

hipError_t gs_launch_histogram(const float *const *planes, int np, int64_t repeat, int64_t stride, int64_t pitch, int64_t rows,
                               int32_t cols, const float *lo, const float *hi, const float *scale, int32_t bins,
                               int64_t max_groups, unsigned long long *out, hipStream_t s)
{
    if (np < 1 || np > 4 || repeat < 1 || bins < 1 || bins > 4096) return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    GsHistArgs a{};
    const bool vec = gs_plane_set(a.set, planes, np, repeat, stride, pitch, rows, cols);
    for (int i = 0; i < np; ++i) {
        a.lo[i] = lo[i];
        a.hi[i] = hi[i];
        a.scale[i] = scale[i];
    }
    a.bins = bins;
    a.out = out;
    const int64_t nplanes = (int64_t)np * repeat;
    const int64_t segs = ((int64_t)cols + kHistSegment - 1) / kHistSegment, units = rows * segs;
    if (!gs_scan_groups(units, kHistUnitsPerGroup, max_groups, nplanes, a.groups)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.groups * nplanes));
    const size_t lds = (size_t)(bins + 4) * sizeof(unsigned);
    if (vec)
        hipLaunchKernelGGL(gs_plane_hist_k<true>, grid, dim3(256), lds, s, a);
    else
        hipLaunchKernelGGL(gs_plane_hist_k<false>, grid, dim3(256), lds, s, a);
    return hipGetLastError();
}
