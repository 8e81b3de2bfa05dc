// gs_morphology.hip -- bit-quad counts of thresholded planes on the device (include/gs_hip.h: gs_fields_morphology,
// gs_members_morphology).
//
// gs_plane_quads_k classifies every 2 x 2 block of a plane's thresholded image, padded with one ring of unset cells, by the
// rule of gs_hip.h and adds the counts of the five classes with a set cell -- Q1, Q2, Q3, Q4, QD; Q0 is the host's complement
// -- to the plane's u64 counters, for up to four thresholds in one pass.  Counts are integers and additive over any partition
// of the quads: neither the launch shape nor the slab layout shows in the result.
//
// Work: a unit is a strip of 256 columns x a run of kQuadRows quad rows, and a wave owns a unit at a time.  It marches down
// the unit with the set bits of the row above in two registers, so that a row is read once -- only the row that two
// vertically adjacent units share is read twice, 1 / kQuadRows of the plane.  Its lanes read 16 B each, kQuadUnroll rows ahead
// of their use, as gs_row_summary_k reads columns.
// Bits: a lane packs the set bits of its four columns for every threshold into one word -- threshold k in byte k: bit 0 the
// column to the left of the lane (never set: it only exists as the padding column of the plane's first lane), bits 1..4 its
// own columns, bit 5 the column to its right, which is the right neighbour's bit 1 moved over by one DPP wave shift; the
// strip's last lane has no neighbour and keeps the bit of one extra cell that every lane reads from the same address.  A
// column >= cols is never set (the pitch padding holds whatever kernels left there), nor is the row above the plane when
// there is none, nor the row below it.  The class of the five quads of a lane follows from bit-sliced sums of the four
// corners over all thresholds at once; a lane that is not the plane's first has the right corners of its quad 0 masked away,
// which makes that quad Q0: not counted.  All control flow is wave-uniform: rows and columns outside the plane are loaded
// from a clamped address and masked.
// Counting: five u32 counters per threshold and lane, reduced over the wave and the workgroup (LDS) at the kernel's end.
//
// Built with hipcc's default float mode (f32 denormals kept), as gs_histogram.hip is: a sub-normal cell is compared as the
// value it is.
#include "gs_kernels.h"
#include "gs_plane_scan.h"

namespace {

constexpr int kQuadRows = 32;  // quad rows of a unit (a multiple of kQuadUnroll): one row in kQuadRows + 1 is read twice
constexpr int kQuadUnroll = 8; // rows whose loads a wave issues before it classifies them
// A wave takes at most kQuadUnitsPerWave units (the launcher sizes the grid for it) of kQuadRows quad rows with 5 quads per
// lane at most: a lane counter stays below 5 * 2^5 * 2^16 < 2^24, and the sum over the 256 lanes of a workgroup below 2^32,
// so no u32 on the way can wrap whatever the plane.
constexpr int64_t kQuadUnitsPerWave = 1 << 16;
constexpr int kQuadClasses = 5; // Q1, Q2, Q3, Q4, QD

struct GsQuadArgs {
    float t[4][4];         // per set.p[]: the thresholds and ...
    uint32_t flip[4];      // ... the sign flip of gs_is_set
    const float *above[4]; // per set.p[]: columns [0, cols) of the row above the plane's row 0, or null: unset (repeat == 1 only)
    GsPlaneSet set;        // (in this order a wave fetches its arguments in the fewest loads and waits: gs_plane_scan.h)
    int32_t bottom;        // 1: the quad row below the last row (its lower half is padding) is counted too
    int64_t groups;        // workgroups per plane
    unsigned long long *out; // [planes][nt][kQuadClasses], zeroed by the caller
};

// Lane l receives lane l + 1's `w`; lane 63, which has no such neighbour, keeps `last`.  Every lane active.
__device__ __forceinline__ unsigned from_right(unsigned w, unsigned last)
{
    return (unsigned)__builtin_amdgcn_update_dpp((int)last, (int)w, 0x130 /* wave_shl:1 */, 0xf, 0xf, false);
}

// The set bits of four cells at bits 1..4 of byte k for threshold k.
template <int NT>
__device__ __forceinline__ unsigned bits_of(float4 x, const float *t, uint32_t flip)
{
    unsigned w = 0u;
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        w |= (gs_is_set(x.x, flip, t[k]) ? 2u : 0u) << (8 * k);
        w |= (gs_is_set(x.y, flip, t[k]) ? 4u : 0u) << (8 * k);
        w |= (gs_is_set(x.z, flip, t[k]) ? 8u : 0u) << (8 * k);
        w |= (gs_is_set(x.w, flip, t[k]) ? 16u : 0u) << (8 * k);
    }
    return w;
}

// 1-D grid of planes x groups workgroups of 4 waves.
template <int NT, bool VEC>
__global__ __launch_bounds__(256) void gs_plane_quads_k(GsQuadArgs a)
{
    __shared__ unsigned total[NT * kQuadClasses];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t y = (int64_t)blockIdx.x / a.groups, g = (int64_t)blockIdx.x % a.groups;
    int which;
    const float *plane = gs_plane_at(a.set, y, which);
    const float *above = a.above[which];
    const uint32_t flip = a.flip[which];
    float t[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) t[k] = a.t[which][k];
    if (threadIdx.x < NT * kQuadClasses) total[threadIdx.x] = 0u;
    __syncthreads();

    const int cols = a.set.cols;
    const int64_t rows = a.set.rows, pitch = a.set.pitch;
    const int64_t quad_rows = rows + (a.bottom ? 1 : 0); // quad row q: the plane's rows q - 1 and q
    const int64_t strips = ((int64_t)cols + 255) / 256, chunks = (quad_rows + kQuadRows - 1) / kQuadRows;
    const int64_t units = strips * chunks;
    unsigned n[NT][kQuadClasses];
#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int c = 0; c < kQuadClasses; ++c) n[k][c] = 0u;

    // row r of the plane as the wave reads it: an address that exists, and whether its cells count (both wave-uniform)
    auto row_at = [&](int64_t r, unsigned &live) -> const float * {
        if (r < 0) {
            live = above ? ~0u : 0u;
            return above ? above : plane;
        }
        live = r < rows ? ~0u : 0u;
        return plane + (r < rows ? r : rows - 1) * pitch;
    };

    for (int64_t u = g * 4 + wave; u < units; u += a.groups * 4) {
        const int64_t q0 = (u / strips) * kQuadRows;
        const int64_t q1 = q0 + kQuadRows < quad_rows ? q0 + kQuadRows : quad_rows;
        const int c0 = (int)(u % strips) * 256, c = c0 + 4 * lane;
        // own columns inside the row, in every byte; the extra cell at column c0 + 256 (wave-uniform)
        unsigned own = (c < cols ? 2u : 0u) | (c + 1 < cols ? 4u : 0u) | (c + 2 < cols ? 8u : 0u) | (c + 3 < cols ? 16u : 0u);
        own *= 0x01010101u;
        const unsigned extra_live = c0 + 256 < cols ? 0x02020202u : 0u;
        const int ce = c0 + 256 < cols ? c0 + 256 : cols - 1;
        const GsLaneColumns at = gs_lane_columns(c, cols);
        // the right corners of quad 0 count in the plane's first lane alone: there the column to the left is the padding
        const unsigned right = (c == 0) ? 0x1f1f1f1fu : 0x1e1e1e1eu;

        auto load = [&](const float *row, float4 &x, float &xe) {
            x = gs_load_columns<VEC>(row, at);
            xe = row[ce];
        };
        // the row's word: bits 1..4 the lane's columns, bit 5 the column to its right, of every threshold's byte
        auto word = [&](float4 x, float xe, unsigned live) -> unsigned {
            const unsigned w = bits_of<NT>(x, t, flip) & own;
            const unsigned e = bits_of<NT>(make_float4(xe, xe, xe, xe), t, flip) & extra_live;
            const unsigned nb = from_right(w, e);
            return (w | ((nb & 0x02020202u) << 4)) & live;
        };

        unsigned live0;
        float4 x0;
        float xe0;
        load(row_at(q0 - 1, live0), x0, xe0);
        const unsigned top = word(x0, xe0, live0);
        unsigned tl = top & 0x1f1f1f1fu, tr = (top >> 1) & right; // the corners of the row above, left and right

        for (int64_t q = q0; q < q1; q += kQuadUnroll) { // (scalar: no lane leaves early)
            float4 x[kQuadUnroll];
            float xe[kQuadUnroll];
            unsigned live[kQuadUnroll];
#pragma unroll
            for (int i = 0; i < kQuadUnroll; ++i) load(row_at(q + i, live[i]), x[i], xe[i]);
#pragma unroll
            for (int i = 0; i < kQuadUnroll; ++i) {
                if (q + i >= q1) break; // (scalar)
                const unsigned w = word(x[i], xe[i], live[i]);
                const unsigned bl = w & 0x1f1f1f1fu, br = (w >> 1) & right;
                // corners set, bit-sliced: b0 + 2 b1 + 4 q4
                const unsigned s1 = tl ^ tr, c1 = tl & tr, s2 = bl ^ br, c2 = bl & br;
                const unsigned b0 = s1 ^ s2, b1 = c1 ^ c2 ^ (s1 & s2), q4 = c1 & c2;
                const unsigned two = b1 & ~b0, side = tl ^ br; // of two set corners: tl != br <=> they share a side
                const unsigned m[kQuadClasses] = {b0 & ~b1, two & side, b0 & b1, q4, two & ~side};
#pragma unroll
                for (int k = 0; k < NT; ++k)
#pragma unroll
                    for (int cl = 0; cl < kQuadClasses; ++cl)
                        n[k][cl] += (unsigned)__popc(NT == 1 ? m[cl] : (m[cl] & (0x1fu << (8 * k))));
                tl = bl;
                tr = br;
            }
        }
    }

#pragma unroll
    for (int k = 0; k < NT; ++k)
#pragma unroll
        for (int cl = 0; cl < kQuadClasses; ++cl) {
            unsigned v = n[k][cl];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v += (unsigned)__shfl_xor((int)v, m);
            if (lane == 0 && v) atomicAdd(&total[k * kQuadClasses + cl], v);
        }
    __syncthreads();
    if (threadIdx.x < NT * kQuadClasses) {
        const unsigned v = total[threadIdx.x];
        if (v) atomicAdd(&a.out[y * (int64_t)(NT * kQuadClasses) + threadIdx.x], (unsigned long long)v);
    }
}

template <int NT>
void launch_quads(bool vec, dim3 grid, hipStream_t s, const GsQuadArgs &a)
{
    if (vec)
        hipLaunchKernelGGL((gs_plane_quads_k<NT, true>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((gs_plane_quads_k<NT, false>), grid, dim3(256), 0, s, a);
}

} // namespace

hipError_t gs_launch_quads(const float *const *planes, const float *const *above, int np, int64_t repeat, int64_t stride,
                           int64_t pitch, int64_t rows, int32_t cols, int bottom, const float *thresholds, const int32_t *sense,
                           int32_t nt, int64_t max_groups, unsigned long long *out, hipStream_t s)
{
    if (np < 1 || np > 4 || repeat < 1 || nt < 1 || nt > 4) return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    GsQuadArgs a{};
    for (int i = 0; i < np; ++i) a.above[i] = (above && repeat == 1) ? above[i] : nullptr;
    const bool vec = gs_plane_set(a.set, planes, np, repeat, stride, pitch, rows, cols, a.above);
    gs_set_rules(a.t, a.flip, thresholds, sense, np, nt);
    a.bottom = bottom ? 1 : 0;
    a.out = out;
    const int64_t nplanes = (int64_t)np * repeat;
    const int64_t quad_rows = rows + a.bottom;
    const int64_t units = (((int64_t)cols + 255) / 256) * ((quad_rows + kQuadRows - 1) / kQuadRows);
    if (!gs_scan_groups(units, 4 * kQuadUnitsPerWave, max_groups, nplanes, a.groups)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.groups * nplanes));
    switch (nt) {
    case 1: launch_quads<1>(vec, grid, s, a); break;
    case 2: launch_quads<2>(vec, grid, s, a); break;
    case 3: launch_quads<3>(vec, grid, s, a); break;
    default: launch_quads<4>(vec, grid, s, a); break;
    }
    return hipGetLastError();
}
