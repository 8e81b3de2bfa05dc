// gs_correlation.hip -- two-point pair counts of thresholded planes on the device (include/gs_hip.h: gs_fields_correlation,
// gs_members_correlation).
//
// gs_plane_pairs_k counts, for every lag d = 0 .. L (L <= 64) along the four unit steps (0, 1), (1, 0), (1, 1), (1, -1), the
// cell pairs {p, p + d e_k} of a plane's thresholded image that are both set, by the rule of gs_hip.h, and adds the counts to
// the plane's u64 counters, for up to four thresholds in one pass.  Pairs never wrap.  Counts are integers and additive over
// any partition of the pairs: neither the launch shape nor the slab layout shows in the result.
//
// Work: a unit is a strip of 256 columns x a run of kPairRows rows, and a wave owns a unit at a time.  A pair belongs to its
// LOWER row, so the wave first runs in over the L rows above its unit -- from the plane, from the rows staged above a slab's
// first row, or unset where there is nothing above -- forming masks and counting nothing, then marches down its rows.
// Masks: a lane reads one cell from each of six 64-column words of the row -- the 64 columns to the left of the strip, the
// strip's four words, the 64 columns to its right; the loads of kPairUnroll rows are issued before they are used -- so that
// one compare gives the wave the 64-bit mask of a word (a ballot: bit i = column 64 w + i), wave-uniform.  No load is wider
// than 4 B: nothing is assumed about the alignment of a plane.  A column outside [0, cols) is never set (loaded from a clamped
// address and masked), nor is a row above the plane when none was staged.
// Lane = lag: lane l counts lag d = l + 1.  It keeps the strip's four words of the row d rows above the current one, handed
// down one lane per row with a DPP wave shift (lane 0 takes the current row's), and counts with shift, and, popcount:
//   direction 0   cur[c] & cur[c + d]      direction 2   up[c] & cur[c + d]
//   direction 1   cur[c] & up[c]           direction 3   up[c] & cur[c - d]
// for the strip's columns c, the shifts carrying across the words into the halo words.  Lag 0, the set cells of the strip, is
// a wave-uniform popcount.  Lanes whose lag exceeds L count what nobody reads.  All control flow is wave-uniform.
// Counting: u32 per lane, direction and threshold; added over the workgroup in LDS ([NT][4][65] u32) and then once per
// workgroup to the u64 counters.
//
// Built with hipcc's default float mode (f32 denormals kept), as gs_morphology.hip is: a sub-normal cell is compared as the
// value it is.
#include "gs_kernels.h"
#include "gs_plane_scan.h"

namespace {

#ifndef GS_PAIR_ROWS
#define GS_PAIR_ROWS 512 // (a build may set another height to time it: tools/ab_build.py; the result does not depend on it)
#endif
constexpr int kPairRows = GS_PAIR_ROWS; // rows of a unit: the run-in adds L / kPairRows of its reads, 1/8 at L = 64
static_assert(kPairRows >= 64 && kPairRows <= 512, "the bound on a lane's counter below assumes at most 2^9 rows");
constexpr int kPairUnroll = 4;  // rows whose loads a wave issues before it forms their masks (8: SGPR spills with 3 and 4
                                // thresholds, 135 .. 186 VGPRs against 95 .. 145)
constexpr int kPairLags = 65;   // lags 0 .. 64
constexpr int kPairWords = 6;   // 64-column words of a row a wave looks at: left halo, the strip's four, right halo
// A wave takes at most kPairUnitsPerWave units (the launcher sizes the grid for it) of kPairRows rows, each adding at most
// 256 to a lane's counter: a lane counter stays below 2^9 * 2^8 * 2^12 = 2^29, and the sum over the 4 waves of a workgroup
// below 2^31, so no u32 on the way can wrap whatever the plane.
constexpr int64_t kPairUnitsPerWave = 1 << 12;

struct GsPairArgs {
    const float *p[4];     // the first `np` planes; plane y of the launch is p[y % np] + (y / np) * stride
    const float *above[4]; // per p[]: the `nabove` rows above the plane's row 0, `pitch` floats apart, the farthest first, or
                           // null: unset (repeat == 1 only)
    float t[4][4];         // per p[]: the thresholds and ...
    uint32_t flip[4];      // ... the sign flip of gs_is_set
    // (no GsPlaneSet: it splits the one load of the next four and costs a wave a wait, profiles/plane_scan_refactor.md)
    int32_t np;
    int32_t nabove;
    int32_t max_lag;       // L, 1 .. 64
    int32_t cols;
    int64_t stride;        // floats between one group of np planes and the next (ensembles: a member's cells)
    int64_t pitch, rows;   // of every plane
    int64_t groups;        // workgroups per plane
    unsigned long long *out; // [planes][nt][4][L + 1], zeroed by the caller
};

// Lane l receives lane l - 1's `w`; lane 0, which has no such neighbour, takes `first`.  Every lane active.
__device__ __forceinline__ uint64_t from_left(uint64_t w, uint64_t first)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)first, (int)(unsigned)w, 0x138 /* wave_shr:1 */,
                                                              0xf, 0xf, false);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp((int)(unsigned)(first >> 32), (int)(unsigned)(w >> 32),
                                                              0x138 /* wave_shr:1 */, 0xf, 0xf, false);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ unsigned popc64(uint64_t x) { return (unsigned)__popcll(x); }

// 1-D grid of planes x groups workgroups of 4 waves.
template <int NT>
__global__ __launch_bounds__(256) void gs_plane_pairs_k(GsPairArgs a)
{
    __shared__ unsigned total[NT * 4 * kPairLags];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t y = (int64_t)blockIdx.x / a.groups, g = (int64_t)blockIdx.x % a.groups;
    const int which = (int)(y % a.np);
    const float *plane = a.p[which] + (y / a.np) * a.stride;
    const float *above = a.above[which];
    const uint32_t flip = a.flip[which];
    float t[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) t[k] = a.t[which][k];
    for (int i = (int)threadIdx.x; i < NT * 4 * kPairLags; i += 256) total[i] = 0u;
    __syncthreads();

    const int cols = a.cols, L = a.max_lag;
    const int64_t rows = a.rows, pitch = a.pitch, nabove = above ? a.nabove : 0;
    const int64_t strips = ((int64_t)cols + 255) / 256, chunks = (rows + kPairRows - 1) / kPairRows;
    const int64_t units = strips * chunks;
    unsigned n[NT][4]; // lag lane + 1 along the four directions
    unsigned n0[NT];   // lag 0: set cells (wave-uniform)
#pragma unroll
    for (int k = 0; k < NT; ++k) {
        n0[k] = 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) n[k][e] = 0u;
    }

    // row r of the plane as the wave reads it: an address that exists (wave-uniform).  A row above the plane that was not
    // staged is read from row 0 and masked; a row below the plane is only ever loaded, never used.
    auto row_at = [&](int64_t r) -> const float * {
        if (r < 0) return r >= -nabove ? above + (r + nabove) * pitch : plane;
        return plane + (r < rows ? r : rows - 1) * pitch;
    };

    for (int64_t u = g * 4 + wave; u < units; u += a.groups * 4) {
        const int64_t q0 = (u / strips) * kPairRows;
        const int64_t q1 = q0 + kPairRows < rows ? q0 + kPairRows : rows;
        const int c0 = (int)(u % strips) * 256;
        // the lane's column in each word, clamped into the row, and the columns of each word that exist (wave-uniform)
        int at[kPairWords];
        uint64_t inside[kPairWords];
#pragma unroll
        for (int w = 0; w < kPairWords; ++w) {
            const int64_t c = (int64_t)c0 - 64 + 64 * w + lane;
            at[w] = (int)(c < 0 ? 0 : (c < cols ? c : cols - 1));
            inside[w] = __ballot(c >= 0 && c < cols);
        }
        uint64_t up[NT][4]; // the strip's words of the row lane + 1 rows above the current one
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int w = 0; w < 4; ++w) up[k][w] = 0ull;

        for (int64_t r = q0 - L; r < q1; r += kPairUnroll) { // (scalar: no lane leaves early)
            float x[kPairUnroll][kPairWords];
#pragma unroll
            for (int i = 0; i < kPairUnroll; ++i) {
                const float *row = row_at(r + i);
#pragma unroll
                for (int w = 0; w < kPairWords; ++w) x[i][w] = row[at[w]];
            }
#pragma unroll
            for (int i = 0; i < kPairUnroll; ++i) {
                if (r + i >= q1) break;            // (scalar)
                const bool counted = r + i >= q0;  // (scalar) a run-in row only fills the history
                const uint64_t live = r + i >= -nabove ? ~0ull : 0ull; // (scalar) nothing is set above what exists
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    uint64_t cur[kPairWords];
#pragma unroll
                    for (int w = 0; w < kPairWords; ++w)
                        cur[w] = __ballot(gs_is_set(x[i][w], flip, t[k])) & inside[w] & live;
                    if (counted) {
                        n0[k] += popc64(cur[1]) + popc64(cur[2]) + popc64(cur[3]) + popc64(cur[4]);
#pragma unroll
                        for (int w = 0; w < 4; ++w) {
                            // the current row d = lane + 1 columns to the right and to the left of this word's columns
                            const uint64_t right = ((cur[w + 1] >> 1) >> lane) | (cur[w + 2] << (63 - lane));
                            const uint64_t left = ((cur[w + 1] << 1) << lane) | (cur[w] >> (63 - lane));
                            n[k][0] += popc64(cur[w + 1] & right);
                            n[k][1] += popc64(cur[w + 1] & up[k][w]);
                            n[k][2] += popc64(up[k][w] & right);
                            n[k][3] += popc64(up[k][w] & left);
                        }
                    }
#pragma unroll
                    for (int w = 0; w < 4; ++w) up[k][w] = from_left(up[k][w], cur[w + 1]);
                }
            }
        }
    }

    if (lane < L) {
#pragma unroll
        for (int k = 0; k < NT; ++k)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (n[k][e]) atomicAdd(&total[(k * 4 + e) * kPairLags + lane + 1], n[k][e]);
                if (lane == 0 && n0[k]) atomicAdd(&total[(k * 4 + e) * kPairLags], n0[k]);
            }
    }
    __syncthreads();
    for (int i = (int)threadIdx.x; i < NT * 4 * (L + 1); i += 256) {
        const int ke = i / (L + 1), d = i % (L + 1);
        const unsigned v = total[ke * kPairLags + d];
        if (v) atomicAdd(&a.out[(y * (int64_t)(NT * 4) + ke) * (int64_t)(L + 1) + d], (unsigned long long)v);
    }
}

} // namespace

hipError_t gs_launch_pairs(const float *const *planes, const float *const *above, int32_t nabove, int np, int64_t repeat,
                           int64_t stride, int64_t pitch, int64_t rows, int32_t cols, const float *thresholds,
                           const int32_t *sense, int32_t nt, int32_t max_lag, int64_t max_groups, unsigned long long *out,
                           hipStream_t s)
{
    if (np < 1 || np > 4 || repeat < 1 || nt < 1 || nt > 4 || max_lag < 1 || max_lag > 64 || nabove < 0)
        return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    GsPairArgs a{};
    for (int i = 0; i < np; ++i) {
        a.p[i] = planes[i];
        a.above[i] = (above && repeat == 1 && nabove > 0) ? above[i] : nullptr;
    }
    gs_set_rules(a.t, a.flip, thresholds, sense, np, nt);
    a.np = np;
    a.nabove = nabove;
    a.max_lag = max_lag;
    a.cols = cols;
    a.stride = stride;
    a.pitch = pitch;
    a.rows = rows;
    a.out = out;
    const int64_t nplanes = (int64_t)np * repeat;
    const int64_t units = (((int64_t)cols + 255) / 256) * ((rows + kPairRows - 1) / kPairRows);
    if (!gs_scan_groups(units, 4 * kPairUnitsPerWave, max_groups, nplanes, a.groups)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.groups * nplanes));
    switch (nt) {
    case 1: hipLaunchKernelGGL((gs_plane_pairs_k<1>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((gs_plane_pairs_k<2>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((gs_plane_pairs_k<3>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((gs_plane_pairs_k<4>), grid, dim3(256), 0, s, a); break;
    }
    return hipGetLastError();
}
