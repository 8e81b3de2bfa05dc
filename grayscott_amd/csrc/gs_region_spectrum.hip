// gs_region_spectrum.hip -- tile-averaged power spectra of every region of rh x rw cells of a plane on the device
// (include/gs_hip.h: gs_fields_region_spectrum): a region's result is what gs_spectrum.hip leaves for a plane that holds the
// region's cells alone.  The per-tile work is gs_spectrum_tile.h's, the body gs_spectrum_tiles_k runs; here the tiles are
// anchored at every region's first row and column, and segments and bands are counted inside a region.
//
// A slab's region rows are `full` rows of rh cells and, below them, perhaps a ragged one; its region columns likewise.  A full
// region row has bmax = rh / T bands of tiles, the ragged one fewer (or none); a band of a full region column has smax =
// ceil((rw / T) / 16) segments, the ragged column's fewer (or none).  The bands of a plane are numbered down the slab -- band
// g = i bmax + b is band b of region row i, which holds for the ragged row too --, the segments of such a band across it --
// segment q = j smax + s is segment s of region column j --: a record per (plane, g, q) and not one more, in that order.
//
// gs_region_spectrum_tiles_k: one workgroup of 4 waves per record, the grid flattened into its first index (a slab has fewer
//                 than 2^31 records: the records' cap of gs_hip.h).  Tile t of the segment lies at
//                 plane + (i rh + b T) pitch + j rw + t T: rw is a multiple of 4, so where the whole-grid kernel may read 16
//                 bytes per lane this one may too.
// gs_region_spectrum_fold_k: a thread per (plane, region, word): for each band of the region in ascending order its segment
//                 records added in ascending order from +0.0, then the band sums added in ascending order from +0.0 (the
//                 counts as integers).  Every region's words are written, zeros for a region in which no tile fits.
// No workgroup waits for another and nothing is added atomically: a region lies inside one slab, so its result is complete.
//
// Built with hipcc's default float mode (f32 denormals kept) and -ffp-contract=off, as gs_spectrum.hip is.
#include "gs_spectrum_tile.h"
#include "gs_plane_scan.h"

namespace {

// How a slab's rows and columns fall into regions, bands and segments (the head comment).
struct GsRegionSpectrumShape {
    int32_t rh, rw;       // a region's cells
    int32_t rr, rc;       // region rows of the slab, region columns
    int32_t bmax, smax;   // bands of a full region row, segments of a band of a full region column
    int32_t last_bands;   // bands of the ragged region row (0: there is none, or no tile fits)
    int32_t last_tiles;   // tiles of a band of the ragged region column (0 likewise)
    int32_t full_rows, full_cols, full_tiles; // full region rows and columns, tiles of a band of a full region column
    uint32_t bands, segs; // bands of a plane, segments of such a band
};

struct GsRegionSpectrumArgs {
    GsPlaneSet set;
    GsRegionSpectrumShape g;
    int32_t window;  // != 0: the window is applied
    double *records; // [plane][band g][segment q][T (T/2 + 1) + 2]
};

GsRegionSpectrumShape shape_of(int64_t rows, int32_t cols, int32_t rh, int32_t rw, int32_t tile)
{
    GsRegionSpectrumShape g{};
    g.rh = rh;
    g.rw = rw;
    g.rr = (int32_t)((rows + rh - 1) / rh);
    g.rc = (cols + rw - 1) / rw;
    g.full_rows = (int32_t)(rows / rh);
    g.full_cols = cols / rw;
    g.full_tiles = rw / tile;
    g.bmax = rh / tile;
    g.smax = (g.full_tiles + kSpectrumSegment - 1) / kSpectrumSegment;
    g.last_bands = (int32_t)(rows % rh) / tile;
    g.last_tiles = cols % rw / tile;
    const int64_t bands = (int64_t)g.full_rows * g.bmax + g.last_bands;
    const int64_t segs = (int64_t)g.full_cols * g.smax + (g.last_tiles + kSpectrumSegment - 1) / kSpectrumSegment;
    g.bands = (uint32_t)bands; // (the callers have bounded bands * segs: gs_region_spectrum_records)
    g.segs = (uint32_t)segs;
    return g;
}

template <int T, bool VEC>
__global__ __launch_bounds__(256) void gs_region_spectrum_tiles_k(GsRegionSpectrumArgs a, GsSpectrumTables tab)
{
    using G = Geo<T>;
    extern __shared__ double gs_region_spectrum_lds[];
    const SpectrumLds<T> l = gs_spectrum_lds_parts<T>(gs_region_spectrum_lds, tab);

    // (32-bit divisions: a 64-bit one would bring its own multiply-adds)
    const GsRegionSpectrumShape &g = a.g;
    const unsigned unit = blockIdx.x, per_plane = g.bands * g.segs;
    const unsigned y = unit / per_plane, in_plane = unit - y * per_plane;
    const unsigned band = in_plane / g.segs, q = in_plane - band * g.segs;
    const unsigned i = band / (unsigned)g.bmax, b = band - i * (unsigned)g.bmax;
    const unsigned j = q / (unsigned)g.smax, s = q - j * (unsigned)g.smax;
    const int tiles = (int)j < g.full_cols ? g.full_tiles : g.last_tiles;
    const int j0 = (int)s * kSpectrumSegment, j1 = j0 + kSpectrumSegment < tiles ? j0 + kSpectrumSegment : tiles;
    const int64_t pitch = a.set.pitch;
    const float *first = a.set.p[y] + ((int64_t)i * g.rh + (int64_t)b * T) * pitch + (int64_t)j * g.rw;

    double acc[G::NB];
#pragma unroll
    for (int n = 0; n < G::NB; ++n) acc[n] = 0.0;
    unsigned long long used = 0, skipped = 0;
    for (int t = j0; t < j1; ++t) { // (uniform: every thread takes every barrier)
        if (gs_spectrum_tile<T, VEC>(first + t * T, pitch, a.window, l, acc)) ++skipped;
        else ++used;
    }
    gs_spectrum_write_record<T>(a.records + (int64_t)unit * (G::BINS + 2), acc, used, skipped);
}

// A thread per (plane, region, word), the grid flattened into its first index: (plane, region) = blockIdx.x / chunks, the
// chunk of 256 words the remainder.
__global__ __launch_bounds__(256) void gs_region_spectrum_fold_k(const double *records, GsRegionSpectrumShape g, int32_t bins,
                                                                  uint32_t chunks, double *out)
{
    const uint32_t at = blockIdx.x / chunks; // (plane * rr + i) * rc + j
    const int32_t w = (int32_t)(blockIdx.x - at * chunks) * 256 + (int32_t)threadIdx.x;
    const int32_t words = bins + 2;
    if (w >= words) return;
    const uint32_t row = at / (uint32_t)g.rc, j = at - row * (uint32_t)g.rc; // row: plane * rr + i
    const uint32_t y = row / (uint32_t)g.rr, i = row - y * (uint32_t)g.rr;
    const int32_t nb = (int32_t)i < g.full_rows ? g.bmax : g.last_bands;
    const int32_t tiles = (int32_t)j < g.full_cols ? g.full_tiles : g.last_tiles;
    const int32_t ns = (tiles + kSpectrumSegment - 1) / kSpectrumSegment;
    // (band b of the region is band i bmax + b of the plane, its segment s segment j smax + s of that band)
    const int64_t band0 = (int64_t)y * g.bands + (int64_t)i * g.bmax, seg0 = (int64_t)j * g.smax;
    if (w < bins) {
        double sum = 0.0;
        for (int32_t b = 0; b < nb; ++b) {
            const double *rec = records + ((band0 + b) * g.segs + seg0) * words + w;
            double band = 0.0;
            for (int32_t k = 0; k < ns; ++k) band = band + rec[(int64_t)k * words];
            sum = sum + band;
        }
        out[(int64_t)at * words + w] = sum;
    } else {
        unsigned long long sum = 0;
        for (int32_t b = 0; b < nb; ++b) {
            const unsigned long long *rec = reinterpret_cast<const unsigned long long *>(records) + ((band0 + b) * g.segs + seg0) * words + w;
            for (int32_t k = 0; k < ns; ++k) sum += rec[(int64_t)k * words];
        }
        reinterpret_cast<unsigned long long *>(out)[(int64_t)at * words + w] = sum;
    }
}

template <int T, bool VEC>
hipError_t launch_region_tiles(unsigned units, const GsRegionSpectrumArgs &a, const GsSpectrumTables &tab, hipStream_t s)
{
    constexpr size_t lds = Geo<T>::LDS;
    static_assert(lds <= 160 * 1024, "a workgroup's LDS");
    if (lds > 64 * 1024) { // the limit belongs to the function on the current device: set where it is launched
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&gs_region_spectrum_tiles_k<T, VEC>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((gs_region_spectrum_tiles_k<T, VEC>), dim3(units), dim3(256), lds, s, a, tab);
    return hipGetLastError();
}

template <bool VEC>
hipError_t launch_region_tiles_of(int32_t tile, unsigned units, const GsRegionSpectrumArgs &a, const GsSpectrumTables &tab,
                                  hipStream_t s)
{
    switch (tile) {
    case 16: return launch_region_tiles<16, VEC>(units, a, tab, s);
    case 32: return launch_region_tiles<32, VEC>(units, a, tab, s);
    case 64: return launch_region_tiles<64, VEC>(units, a, tab, s);
    default: return launch_region_tiles<128, VEC>(units, a, tab, s);
    }
}

bool tile_ok(int32_t tile)
{
    return tile == 16 || tile == 32 || tile == 64 || tile == 128;
}

} // namespace

uint64_t gs_region_spectrum_records(uint64_t rows, uint64_t cols, int32_t rh, int32_t rw, int32_t tile)
{
    if (rh < 1 || rw < 1 || !tile_ok(tile)) return 0;
    const uint64_t q = (uint64_t)rh, w = (uint64_t)rw, T = (uint64_t)tile, S = (uint64_t)kSpectrumSegment;
    const uint64_t bands = rows / q * (q / T) + rows % q / T;
    const uint64_t segs = cols / w * ((w / T + S - 1) / S) + (cols % w / T + S - 1) / S;
    return bands * segs; // (rows, cols < 2^32 and at least T cells per band and 1 per segment: no wrap)
}

hipError_t gs_launch_region_spectrum(const float *const *planes, int np, int64_t pitch, int64_t rows, int32_t cols, int32_t rh,
                                     int32_t rw, int32_t tile, int32_t window, const float *h, const float *w, void *records,
                                     void *out, hipStream_t s)
{
    if (np < 1 || np > 4 || rh < 1 || rw < 4 || rw % 4 != 0 || !tile_ok(tile)) return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    const int32_t bins = tile * (tile / 2 + 1), words = bins + 2;
    const uint32_t chunks = (uint32_t)((words + 255) / 256);
    const uint64_t per_plane = gs_region_spectrum_records((uint64_t)rows, (uint64_t)cols, rh, rw, tile);
    const uint64_t regions = (uint64_t)((rows + rh - 1) / rh) * (uint64_t)((cols + rw - 1) / rw);
    // (a grid's first index; the caps of gs_hip.h keep both far below)
    if (per_plane * (uint64_t)np > (uint64_t)INT32_MAX || regions * (uint64_t)np * chunks > (uint64_t)INT32_MAX)
        return hipErrorInvalidValue;
    GsRegionSpectrumArgs a{};
    const bool vec = gs_plane_set(a.set, planes, np, 1, 0, pitch, rows, cols);
    a.g = shape_of(rows, cols, rh, rw, tile);
    a.window = window;
    a.records = static_cast<double *>(records);
    const unsigned units = (unsigned)(per_plane * (uint64_t)np);
    if (units > 0) {
        const GsSpectrumTables tab = gs_spectrum_tables_of(tile, h, w);
        const hipError_t e = vec ? launch_region_tiles_of<true>(tile, units, a, tab, s) : launch_region_tiles_of<false>(tile, units, a, tab, s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(gs_region_spectrum_fold_k, dim3((unsigned)(regions * (uint64_t)np * chunks)), dim3(256), 0, s, a.records, a.g,
                       bins, chunks, static_cast<double *>(out));
    return hipGetLastError();
}
