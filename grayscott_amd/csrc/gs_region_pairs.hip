// gs_region_pairs.hip -- regional two-point pair counts on the device (include/gs_hip.h: gs_fields_region_correlation): the
// pair counts of every region of rh x rw cells of a plane, each bit for bit what gs_correlation.hip returns for a plane that
// holds that region's cells alone.  A region's border is a wall for pairs: a pair whose two cells lie in different regions
// is never formed.
//
// gs_region_pairs_k is gs_plane_pairs_k's second form (gs_correlation.hip has the technique: ballot masks of 64-column
// words, lane = lag, the row masks handed down one lane per row with a DPP wave shift, shift / and / popcount).  What differs:
// Work: a unit is one region x a strip of 64 SW columns counted from the region's FIRST column x a run of at most kPairRows
// of the region's rows, and a wave owns a unit at a time.
// Columns: the words of a row are masked to the region's columns [cb, ce): the halo words and everything outside the region
// are unset, so the shifts carry nothing across a vertical border.  Loads are 4 B per lane from addresses clamped into
// [cb, ce): nothing is assumed about alignment, nothing outside the region is read.
// Rows: the run-in above a unit starts at the region's first row when fewer than L of its rows lie above the unit -- the
// history of a lane starts unset -- and never reads the region above; the first (or only) unit of a region has no run-in.
// Forms: a region wider than 256 columns is cut into strips of four words with a halo word on either side (HALO); one of at
// most 256 columns is one strip of four words and one of at most 64 columns one strip of one word, both without halo words:
// what would lie in them is outside the region.  Several narrow regions are not packed into one strip.
// Counting: u32 per lane, direction and threshold, at most 256 kPairRows = 2^17 per unit; at the unit's end every non-zero
// counter is added to the region's u64 counters with one atomic (lanes 0 .. 3 add lag 0, which is wave-uniform, for the four
// directions).  All control flow is wave-uniform but those guards; no LDS, no kernel waits for another.
//
// Built with hipcc's default float mode (f32 denormals kept), as gs_correlation.hip is: a sub-normal cell is compared as the
// value it is.
#include "gs_kernels.h"
#include "gs_plane_scan.h"

namespace {

constexpr int kPairRows = 512; // rows of a unit, gs_correlation.hip's: a region higher than this is cut, the lower units run in

struct GsRegionPairArgs {
    const float *p[4];  // the slab's planes (no repeats)
    float t[4][4];      // per p[]: the thresholds and ...
    uint32_t flip[4];   // ... the sign flip of gs_is_set
    int32_t max_lag;    // L, 1 .. 64
    int32_t cols;
    int32_t rh, rw;     // the region shape (rh at most the plane's rows)
    int32_t strips;     // strips a region's rw columns are cut into ...
    int32_t chunks;     // ... and units its rh rows are cut into
    int64_t rr, rc;     // rows of the region grid in this slab, columns of the region grid
    int64_t pitch, rows; // of every plane
    int64_t groups;     // workgroups per plane
    unsigned long long *out; // [plane][rr][rc][nt][4][L + 1], zeroed by the caller
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

// 1-D grid of planes x groups workgroups of 4 waves.  SW: the strip's words; HALO: a word on either side of them is read.
template <int NT, int SW, bool HALO>
__global__ __launch_bounds__(256) void gs_region_pairs_k(GsRegionPairArgs a)
{
    constexpr int H = HALO ? 1 : 0, W = SW + 2 * H; // words a lane loads from; the strip's are H .. H + SW - 1
    constexpr int kUnroll = W >= 4 ? 4 : 8;        // rows whose loads a wave issues before it forms their masks
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t y = (int64_t)blockIdx.x / a.groups, g = (int64_t)blockIdx.x % a.groups;
    const float *plane = a.p[y];
    const uint32_t flip = a.flip[y];
    float t[NT];
#pragma unroll
    for (int k = 0; k < NT; ++k) t[k] = a.t[y][k];

    const int cols = a.cols, L = a.max_lag;
    const int64_t rows = a.rows, pitch = a.pitch;
    const int64_t per_band = a.rc * a.strips;             // units side by side: one run of rows of one row of the region grid
    const int64_t units = a.rr * a.chunks * per_band;

    for (int64_t u = g * 4 + wave; u < units; u += a.groups * 4) {
        const int64_t band = u / per_band, v = u % per_band;
        const int64_t i = band / a.chunks, j = v / a.strips;
        // the region's rows [r0, r1) and the unit's [q0, q1) (all wave-uniform)
        const int64_t r0 = i * a.rh, r1 = r0 + a.rh < rows ? r0 + a.rh : rows;
        const int64_t q0 = r0 + (band % a.chunks) * kPairRows;
        if (q0 >= r1) continue; // (scalar: a ragged region's last units are empty)
        const int64_t q1 = q0 + kPairRows < r1 ? q0 + kPairRows : r1;
        // the region's columns [cb, ce) and the strip's first one
        const int64_t cb = j * a.rw, ce = cb + a.rw < cols ? cb + a.rw : cols;
        const int64_t c0 = cb + (v % a.strips) * (64 * SW);
        if (c0 >= ce) continue; // (scalar: likewise)
        // the lane's column in each word, clamped into the region, and the columns of each word that are the region's
        int at[W];
        uint64_t inside[W];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const int64_t c = c0 + 64 * (w - H) + lane;
            at[w] = (int)(c < cb ? cb : (c < ce ? c : ce - 1));
            inside[w] = __ballot(c >= cb && c < ce);
        }
        unsigned n[NT][4]; // lag lane + 1 along the four directions
        unsigned n0[NT];   // lag 0: set cells (wave-uniform)
        uint64_t up[NT][SW]; // the strip's words of the row lane + 1 rows above the current one; unset above the region
#pragma unroll
        for (int k = 0; k < NT; ++k) {
            n0[k] = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) n[k][e] = 0u;
#pragma unroll
            for (int w = 0; w < SW; ++w) up[k][w] = 0ull;
        }

        // the run-in: the min(L, rows of this region above the unit) rows above it
        const int64_t rs = q0 - L > r0 ? q0 - L : r0;
        for (int64_t r = rs; r < q1; r += kUnroll) { // (scalar: no lane leaves early)
            float x[kUnroll][W];
#pragma unroll
            for (int m = 0; m < kUnroll; ++m) {
                // (a row past the unit is only ever loaded, never used: read from the unit's last row)
                const float *row = plane + (r + m < q1 ? r + m : q1 - 1) * pitch;
#pragma unroll
                for (int w = 0; w < W; ++w) x[m][w] = row[at[w]];
            }
#pragma unroll
            for (int m = 0; m < kUnroll; ++m) {
                if (r + m >= q1) break;           // (scalar)
                const bool counted = r + m >= q0; // (scalar) a run-in row only fills the history
#pragma unroll
                for (int k = 0; k < NT; ++k) {
                    uint64_t cur[SW + 2]; // the strip's words at 1 .. SW; without halo words nothing is set beside them
                    cur[0] = 0ull;
                    cur[SW + 1] = 0ull;
#pragma unroll
                    for (int w = 0; w < W; ++w) cur[w + 1 - H] = __ballot(gs_is_set(x[m][w], flip, t[k])) & inside[w];
                    if (counted) {
#pragma unroll
                        for (int w = 0; w < SW; ++w) {
                            n0[k] += popc64(cur[w + 1]);
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
                    for (int w = 0; w < SW; ++w) up[k][w] = from_left(up[k][w], cur[w + 1]);
                }
            }
        }

        unsigned long long *region = a.out + ((y * a.rr + i) * a.rc + j) * (int64_t)(NT * 4 * (L + 1));
#pragma unroll
        for (int k = 0; k < NT; ++k) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (lane < L && n[k][e]) atomicAdd(&region[(k * 4 + e) * (L + 1) + lane + 1], (unsigned long long)n[k][e]);
            if (lane < 4 && n0[k]) atomicAdd(&region[(k * 4 + lane) * (L + 1)], (unsigned long long)n0[k]);
        }
    }
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

template <int SW, bool HALO>
void launch(int nt, dim3 grid, hipStream_t s, const GsRegionPairArgs &a)
{
    switch (nt) {
    case 1: hipLaunchKernelGGL((gs_region_pairs_k<1, SW, HALO>), grid, dim3(256), 0, s, a); break;
    case 2: hipLaunchKernelGGL((gs_region_pairs_k<2, SW, HALO>), grid, dim3(256), 0, s, a); break;
    case 3: hipLaunchKernelGGL((gs_region_pairs_k<3, SW, HALO>), grid, dim3(256), 0, s, a); break;
    default: hipLaunchKernelGGL((gs_region_pairs_k<4, SW, HALO>), grid, dim3(256), 0, s, a); break;
    }
}

} // namespace

hipError_t gs_launch_region_pairs(const float *const *planes, int np, int64_t pitch, int64_t rows, int32_t cols, int32_t rh,
                                  int32_t rw, const float *thresholds, const int32_t *sense, int32_t nt, int32_t max_lag,
                                  int64_t max_groups, unsigned long long *out, hipStream_t s)
{
    if (np < 1 || np > 4 || nt < 1 || nt > 4 || max_lag < 1 || max_lag > 64 || rh < 1 || rw < 16 || rw % 4 != 0)
        return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    GsRegionPairArgs a{};
    for (int i = 0; i < np; ++i) a.p[i] = planes[i];
    gs_set_rules(a.t, a.flip, thresholds, sense, np, nt);
    a.max_lag = max_lag;
    a.cols = cols;
    a.rh = rh < rows ? rh : (int32_t)rows; // (one row of regions either way)
    a.rw = rw;
    const int32_t widest = rw < cols ? rw : cols; // the columns of the widest region: the narrowest form that holds them
    a.strips = widest > 256 ? (int32_t)ceil_div(widest, 256) : 1;
    a.chunks = (int32_t)ceil_div(a.rh, kPairRows);
    a.rr = ceil_div(rows, a.rh);
    a.rc = ceil_div(cols, a.rw);
    a.pitch = pitch;
    a.rows = rows;
    a.out = out;
    const int64_t units = a.rr * a.chunks * a.rc * a.strips;
    if (!gs_scan_groups(units, 0, max_groups, np, a.groups)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(a.groups * np));
    if (widest > 256)
        launch<4, true>(nt, grid, s, a);
    else if (widest > 64)
        launch<4, false>(nt, grid, s, a);
    else
        launch<1, false>(nt, grid, s, a);
    return hipGetLastError();
}
