// gs_region_hist.hip -- regional histograms on the device (include/gs_hip.h: gs_fields_region_histogram): the bins + 3
// counters of every region of rh x rw cells of a plane, each bit for bit what gs_histogram.hip returns for a plane that holds
// that region's cells alone.  The slot of a cell is gs_hist_count.h's slot_of, the one rule both kernels count by.
//
// gs_region_hist_k: a workgroup of 4 waves takes a TILE at a time -- one row of the region grid x a run of `nreg` adjacent
// regions (or, for a region wider than kTileCols, a chunk of kTileCols of its columns) x a chunk of at most kTileRows of
// that region row's rows (fewer, down to kTileRowsLeast, while the launch has fewer tiles than workgroups it may use: a
// 4096 x 4096 plane of 1024 x 1024 regions is 64 tiles of 256 rows) -- and counts it into u32 words of LDS: nreg x (bins + 3) words, region after region, and one spare
// word behind them.  At the tile's end the words that are not zero are added to the regions' u64 counters in global memory
// and zeroed for the next tile; a region wider or higher than a tile is flushed by several tiles into the same counters.
// nreg is the most regions whose words fit in 64 KiB (no opt-in for dynamic LDS, two workgroups on a CU) and whose columns
// fit in kTileCols: 3 regions at 4096 bins.
// Reading: a lane holds four columns, a 16-byte load, which lie in one region because rw is a multiple of 4.  The tile's
// rows are `qpr` such lanes wide, and the 256 lanes of a load take rpl = 256 / qpr whole rows of the tile, stacked: a narrow
// tile wastes 256 % qpr lanes, not the rest of a wave.  A lane's place in the stack -- row, column, region -- is the
// launch's, not the tile's: only the row pointer moves from load to load, eight loads ahead of their use.
// Counting: gs_hist_count.h's count() on the index of the lane's LDS word -- region and slot together, never the bin alone:
// on one-valued data the lanes of different regions hold the same bin.  A column outside the row, a lane outside the tile
// and a row past its end count into the spare word, which is never flushed.  Loop bounds are wave-uniform, addresses are
// clamped into the plane: no lane leaves early, no load depends on a lane's own condition.
//
// Built with hipcc's default float mode (f32 denormals kept) and -ffp-contract=off, as gs_histogram.hip is.
#include "gs_kernels.h"
#include "gs_hist_count.h"
#include "gs_plane_scan.h"

namespace {

constexpr int kRegHistUnroll = 8;  // loads of 256 lanes x 16 B a workgroup issues before it counts them
constexpr int kTileCols = 1024;    // most columns of a tile: 256 lanes x 4 columns, one load a row
constexpr int kLdsWords = 16384;   // 64 KiB of u32
// A tile is at most kTileRows x kTileCols = 2^18 cells, and every tile is counted between one zeroing of the LDS words and
// their flush: no u32 word can wrap whatever the plane -- the spare word included, which gains at most four per lane of each
// of the tile's at most kTileRows loads, 2^18 as well, and is zeroed with the others.
constexpr int kTileRows = 256;
constexpr int kTileRowsLeast = 32; // below, a tile's zeroing and flush of up to 16 Ki words outweigh its cells

struct GsRegionHistArgs {
    const float *p[4];            // the slab's planes (no repeats)
    float lo[4], hi[4], scale[4]; // per p[]
    int32_t bins;
    int32_t cols;
    int32_t rh, rw;      // the region shape (rh at most the plane's rows)
    int32_t nreg;        // regions side by side in a tile ...
    int32_t cw;          // ... columns each of them has in it: rw, or kTileCols of a wider region, ...
    int32_t cchunks;     // ... which is then cut into this many tiles (nreg == 1); else 1
    int32_t trows;       // rows of a tile: at most kTileRows
    int32_t rchunks;     // tiles of trows rows the rh rows of a region row are cut into
    int32_t rr, rc;      // rows of the region grid in this slab, columns of the region grid
    int32_t ctiles;      // tiles side by side in a row of the region grid
    int32_t tiles;       // rr * rchunks * ctiles: of one plane
    int32_t rows;        // of every plane
    int32_t groups;      // workgroups per plane
    int64_t pitch;       // of every plane
    unsigned long long *out; // [plane][rr][rc][bins + 3], zeroed by the caller
};

// 1-D grid of planes x groups workgroups of 4 waves; dynamic LDS: (nreg * (bins + 3) + 1) u32.
template <bool VEC>
__global__ __launch_bounds__(256) void gs_region_hist_k(GsRegionHistArgs a)
{
    extern __shared__ unsigned h[];
    const int tid = (int)threadIdx.x, lane = tid & 63;
    const int bins = a.bins, per = bins + 3, words = a.nreg * per, spare = words;
    const int y = (int)blockIdx.x / a.groups, g = (int)blockIdx.x % a.groups;
    const float *plane = a.p[y];
    const float lo = a.lo[y], hi = a.hi[y], scale = a.scale[y];
    for (int i = tid; i <= words; i += 256) h[i] = 0u;
    __syncthreads();

    // the lane's place in a load: row lrow of the rpl rows it stacks, columns 4 quad .. 4 quad + 3 of the tile
    const int qpr = a.nreg * (a.cw / 4), rpl = 256 / qpr;
    const int lrow = tid / qpr, quad = tid % qpr;
    const bool stacked = lrow < rpl;                      // (else: one of the 256 % qpr lanes left over)
    const int base = (4 * quad / a.cw) * per;             // the first word of the lane's region
    const int cols = a.cols, rows = a.rows;
    const int64_t pitch = a.pitch;
    Run run{spare, 0};

    // (rows, columns and tiles are 32-bit: the launcher refuses a plane whose sums below could leave that range)
    for (int u = g; u < a.tiles; u += a.groups) { // (u is the workgroup's: every branch on it is taken by all four waves)
        const int band = u / a.ctiles, ct = u % a.ctiles;
        const int i = band / a.rchunks;
        // the region row's rows [r0, r1) and the tile's [q0, q1)
        const int r0 = i * a.rh, r1 = a.rh < rows - r0 ? r0 + a.rh : rows;
        const int q0 = r0 + (band % a.rchunks) * a.trows;
        if (q0 >= r1) continue; // (a ragged region row's last tiles are empty)
        const int q1 = a.trows < r1 - q0 ? q0 + a.trows : r1;
        // the tile's first region and its columns [cb, ce): never beyond its regions, never beyond the row
        const int j0 = (ct / a.cchunks) * a.nreg;
        // (no sum here leaves 32 bits: j0 rw < cols, the chunk's offset is below rw, nreg cw is at most kTileCols)
        const int left = j0 * a.rw, room = cols - left, off = (ct % a.cchunks) * a.cw;
        const int span = a.nreg * a.rw < room ? a.nreg * a.rw : room; // the columns the tile's regions have in the row
        if (off >= span) continue; // (a ragged region's last chunks are empty)
        const int cb = left + off, ce = a.nreg * a.cw < span - off ? cb + a.nreg * a.cw : left + span;

        // the lane's columns: how many of its four lie in the tile, and where it reads -- inside the row whatever they are
        const int c = cb + 4 * quad;
        const int inside = !stacked || c >= ce ? 0 : (ce - c < 4 ? ce - c : 4);
        int at[4];
        if (VEC) { // (16 bytes at a multiple of 4 below cols end below the pitch, a multiple of 4: the padding is readable)
            at[0] = c < cols ? c : 0;
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) at[e] = c + e < cols ? c + e : cols - 1;
        }

        const int loads = (q1 - q0 + rpl - 1) / rpl;      // of 256 lanes each
        for (int m = 0; m < loads; m += kRegHistUnroll) {   // (scalar: no lane leaves early)
            float4 x[kRegHistUnroll];
#pragma unroll
            for (int k = 0; k < kRegHistUnroll; ++k) {
                // (a row past the tile is only ever loaded, never counted: read from the tile's last row)
                const int r = q0 + (m + k) * rpl + lrow;
                const float *row = plane + (r < q1 ? r : q1 - 1) * pitch;
                if (VEC)
                    x[k] = *reinterpret_cast<const float4 *>(row + at[0]);
                else
                    x[k] = make_float4(row[at[0]], row[at[1]], row[at[2]], row[at[3]]);
            }
#pragma unroll
            for (int k = 0; k < kRegHistUnroll; ++k) {
                if (m + k >= loads) break; // (scalar) no lane of the workgroup has a row here
                const int n = q0 + (m + k) * rpl + lrow < q1 ? inside : 0;
                count(h, run, n > 0 ? base + slot_of(x[k].x, true, lo, hi, scale, bins) : spare, lane);
                count(h, run, n > 1 ? base + slot_of(x[k].y, true, lo, hi, scale, bins) : spare, lane);
                count(h, run, n > 2 ? base + slot_of(x[k].z, true, lo, hi, scale, bins) : spare, lane);
                count(h, run, n > 3 ? base + slot_of(x[k].w, true, lo, hi, scale, bins) : spare, lane);
            }
        }
        if (lane == 0) atomicAdd(&h[run.slot], (unsigned)run.n);
        run = Run{spare, 0};
        __syncthreads();

        // the flush: word w is slot w % per of region j0 + w / per of this region row; the spare word is zeroed unread
        unsigned long long *first = a.out + (((int64_t)y * a.rr + i) * a.rc + j0) * per;
        const int64_t live = (int64_t)(a.rc - j0) * per; // (words of regions beyond the region grid stay zero: their columns are outside the row)
        for (int w = tid; w <= words; w += 256) {
            const unsigned n = h[w];
            if (n) {
                if (w < words && w < live) atomicAdd(&first[w], (unsigned long long)n);
                h[w] = 0u;
            }
        }
        __syncthreads();
    }
}

int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

} // namespace

hipError_t gs_launch_region_hist(const float *const *planes, int np, int64_t pitch, int64_t rows, int32_t cols, int32_t rh,
                                 int32_t rw, const float *lo, const float *hi, const float *scale, int32_t bins,
                                 int64_t max_groups, unsigned long long *out, hipStream_t s)
{
    if (np < 1 || np > 4 || bins < 1 || bins > 4096 || rh < 1 || rw < 16 || rw % 4 != 0) return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    // the kernel's rows and columns are 32-bit: the row numbers of a tile's last loads, clamped before they are used, reach up to
    // 8 x 256 rows beyond the plane's, and a tile's lanes kTileCols columns
    if (rows > INT32_MAX - 16 * kTileRows || cols > INT32_MAX - 2 * kTileCols) return hipErrorInvalidValue;
    GsRegionHistArgs a{};
    for (int i = 0; i < np; ++i) {
        a.p[i] = planes[i];
        a.lo[i] = lo[i];
        a.hi[i] = hi[i];
        a.scale[i] = scale[i];
    }
    a.bins = bins;
    a.cols = cols;
    a.rh = rh < rows ? rh : (int32_t)rows; // (one row of regions either way)
    a.rw = rw < cols ? rw : (cols + 3) / 4 * 4; // (one column of regions either way)
    const int64_t rr = ceil_div(rows, a.rh), rc = ceil_div(cols, a.rw);
    const int per = bins + 3;
    int64_t ctiles;
    if (a.rw > kTileCols) { // chunks of one region's columns
        a.nreg = 1;
        a.cw = kTileCols;
        a.cchunks = (int32_t)ceil_div(a.rw, kTileCols);
        ctiles = rc * a.cchunks;
    } else { // regions side by side: as many as fit in the tile's columns, in the LDS words and in the region grid
        int64_t nreg = kTileCols / a.rw;
        if (nreg > (kLdsWords - 1) / per) nreg = (kLdsWords - 1) / per;
        if (nreg > rc) nreg = rc;
        a.nreg = (int32_t)nreg;
        a.cw = a.rw;
        a.cchunks = 1;
        ctiles = ceil_div(rc, nreg);
    }
    // the tile's rows: halved while that leaves workgroups the launch may use without a tile
    a.trows = kTileRows;
    while (a.trows > kTileRowsLeast && rr * ceil_div(a.rh, a.trows) * ctiles * np < max_groups) a.trows /= 2;
    a.rchunks = (int32_t)ceil_div(a.rh, a.trows);
    a.pitch = pitch;
    a.rows = (int32_t)rows;
    a.out = out;
    // (a tile that is not empty holds at least 16 cells, and few are empty: no plane that fits a device has 2^31 of them)
    const int64_t tiles = rr * a.rchunks * ctiles;
    int64_t groups;
    // (gs_scan_groups counts waves that take a unit each: four "units" a tile make a workgroup a tile)
    if (rr > INT32_MAX || rc > INT32_MAX || tiles > INT32_MAX / 4 || !gs_scan_groups(tiles * 4, 0, max_groups, np, groups))
        return hipErrorInvalidValue;
    a.rr = (int32_t)rr;
    a.rc = (int32_t)rc;
    a.ctiles = (int32_t)ctiles;
    a.tiles = (int32_t)tiles;
    a.groups = (int32_t)groups;
    const dim3 grid((unsigned)(groups * np));
    const size_t lds = ((size_t)a.nreg * per + 1) * sizeof(unsigned);
    if (gs_reads_16_bytes(planes, np, 1, 0, pitch))
        hipLaunchKernelGGL(gs_region_hist_k<true>, grid, dim3(256), lds, s, a);
    else
        hipLaunchKernelGGL(gs_region_hist_k<false>, grid, dim3(256), lds, s, a);
    return hipGetLastError();
}
