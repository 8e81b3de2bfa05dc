// gs_spectrum.hip -- tile-averaged power spectra of planes on the device (include/gs_hip.h: gs_fields_spectrum,
// gs_members_spectrum): the f32 radix-2 transform of every whole T x T tile of a plane, T = 16, 32, 64 or 128, its power
// added in f64 over segments of up to 16 tiles of a band of T rows, and the segments' records added per band.
//
// gs_spectrum_tiles_k: one workgroup of 4 waves per (plane, band, segment); the work per tile -- load, mean, row and column
// transforms, the power added to f64 accumulators in registers -- is gs_spectrum_tile.h's, shared with the regional kernel
// (gs_region_spectrum.hip).
// The record of a segment: T (T/2 + 1) f64 sums, then the tiles used and skipped as u64.
// gs_spectrum_fold_k: a thread per (plane, band, word) adds the band's records in ascending segment order from +0.0; a band
// that is not whole (the rows below the last whole band of a slab) and a band of no tiles are written as zeros.
//
// Every f32 operation is rounded on its own (-ffp-contract=off).  The tables -- the window h[T] and the twiddles W[T/2] -- are
// formed by the host and travel by value with the launch.  T = 128 needs 71 KiB of LDS: the kernel's dynamic LDS limit is
// raised at its launch.
//
// Built with hipcc's default float mode (f32 denormals kept), as the other observables' units are.
#include "gs_spectrum_tile.h"
#include "gs_plane_scan.h"

namespace {

struct GsSpectrumArgs {
    GsPlaneSet set;
    int64_t bands;   // whole bands of a plane
    int64_t tiles;   // whole tiles of a band
    int64_t segs;    // segments of a band
    int32_t window;  // != 0: the window is applied
    double *records; // [plane][band][segment][T (T/2 + 1) + 2]
};

// Grid (segments of a band, bands, planes) of workgroups of 256 threads; Geo<T>::LDS bytes of dynamic LDS.
template <int T, bool VEC>
__global__ __launch_bounds__(256) void gs_spectrum_tiles_k(GsSpectrumArgs a, GsSpectrumTables tab)
{
    using G = Geo<T>;
    extern __shared__ double gs_spectrum_lds[];
    const SpectrumLds<T> l = gs_spectrum_lds_parts<T>(gs_spectrum_lds, tab);

    // (the grid's three indices and one 32-bit division: a 64-bit one would bring its own multiply-adds)
    const int64_t seg = (int64_t)blockIdx.x, band = (int64_t)blockIdx.y, y = (int64_t)blockIdx.z;
    const int64_t unit = (y * a.bands + band) * a.segs + seg;
    const unsigned np = (unsigned)a.set.np, group = blockIdx.z / np;
    const float *plane = a.set.p[blockIdx.z - group * np] + (int64_t)group * a.set.stride;
    const int64_t pitch = a.set.pitch;
    const int64_t j0 = seg * kSpectrumSegment, j1 = j0 + kSpectrumSegment < a.tiles ? j0 + kSpectrumSegment : a.tiles;

    double acc[G::NB];
#pragma unroll
    for (int n = 0; n < G::NB; ++n) acc[n] = 0.0;
    unsigned long long used = 0, skipped = 0;

    for (int64_t j = j0; j < j1; ++j) { // (uniform: every thread takes every barrier)
        if (gs_spectrum_tile<T, VEC>(plane + band * T * pitch + j * T, pitch, a.window, l, acc)) ++skipped;
        else ++used;
    }
    gs_spectrum_write_record<T>(a.records + unit * (int64_t)(G::BINS + 2), acc, used, skipped);
}

// A thread per (plane, band of the result, word) -- grid (chunks of 256 words, bands, planes) --: the band's segment records
// added in ascending order from +0.0 (the counts as integers).  `whole` bands of a plane have records, `bands` >= whole are
// written.
__global__ __launch_bounds__(256) void gs_spectrum_fold_k(const double *records, int64_t whole, int64_t bands, int64_t segs, int32_t bins,
                                                           double *out)
{
    const int32_t w = (int32_t)blockIdx.x * 256 + (int32_t)threadIdx.x;
    const int32_t words = bins + 2;
    if (w >= words) return;
    const int64_t y = (int64_t)blockIdx.z, band = (int64_t)blockIdx.y, at = y * bands + band;
    const double *rec = records + ((y * whole + band) * segs) * words + w;
    if (w < bins) {
        double sum = 0.0;
        if (band < whole)
            for (int64_t k = 0; k < segs; ++k) sum = sum + rec[k * words];
        out[at * words + w] = sum;
    } else {
        unsigned long long sum = 0;
        if (band < whole)
            for (int64_t k = 0; k < segs; ++k) sum += reinterpret_cast<const unsigned long long *>(rec)[k * words];
        reinterpret_cast<unsigned long long *>(out)[at * words + w] = sum;
    }
}

template <int T, bool VEC>
hipError_t launch_tiles(dim3 grid, const GsSpectrumArgs &a, const GsSpectrumTables &tab, hipStream_t s)
{
    constexpr size_t lds = Geo<T>::LDS;
    static_assert(lds <= 160 * 1024, "a workgroup's LDS");
    // what gs_spectrum_lds_parts takes apart: the row sums, the slots, the staging rows, the twiddles, the window, the mean
    constexpr int BINS = Geo<T>::BINS, RB = Geo<T>::RB, SP = Geo<T>::SP, HB = Geo<T>::HB;
    static_assert(lds == (size_t)T * 8 + (size_t)BINS * 8 + (size_t)RB * SP * 8 + (size_t)HB * 8 + (size_t)T * 4 + 8, "the LDS layout");
    if (lds > 64 * 1024) { // the limit belongs to the function on the current device: set where it is launched
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(&gs_spectrum_tiles_k<T, VEC>),
                                                 hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((gs_spectrum_tiles_k<T, VEC>), grid, dim3(256), lds, s, a, tab);
    return hipGetLastError();
}

template <bool VEC>
hipError_t launch_tiles_of(int32_t tile, dim3 grid, const GsSpectrumArgs &a, const GsSpectrumTables &tab, hipStream_t s)
{
    switch (tile) {
    case 16: return launch_tiles<16, VEC>(grid, a, tab, s);
    case 32: return launch_tiles<32, VEC>(grid, a, tab, s);
    case 64: return launch_tiles<64, VEC>(grid, a, tab, s);
    default: return launch_tiles<128, VEC>(grid, a, tab, s);
    }
}

int64_t segments_of(int32_t cols, int32_t tile)
{
    return (cols / tile + kSpectrumSegment - 1) / kSpectrumSegment;
}

} // namespace

size_t gs_spectrum_record_bytes(int64_t planes, int64_t rows, int32_t cols, int32_t tile)
{
    return (size_t)(planes * (rows / tile) * segments_of(cols, tile)) * gs_spectrum_result_bytes(tile);
}

hipError_t gs_launch_spectrum(const float *const *planes, int np, int64_t repeat, int64_t stride, int64_t pitch, int64_t rows,
                              int32_t cols, int32_t tile, int32_t window, const float *h, const float *w, void *records,
                              void *out, hipStream_t s)
{
    if (np < 1 || np > 4 || repeat < 1 || (tile != 16 && tile != 32 && tile != 64 && tile != 128)) return hipErrorInvalidValue;
    if (rows <= 0) return hipSuccess;
    const int64_t bands = rows / tile, out_bands = (rows + tile - 1) / tile, segs = segments_of(cols, tile);
    const int32_t bins = tile * (tile / 2 + 1), words = bins + 2;
    if (out_bands > 65535 || segs > INT32_MAX) return hipErrorInvalidValue; // (a grid's second index)
    const GsSpectrumTables tab = gs_spectrum_tables_of(tile, h, w);
    // a grid's third index ends at 65535: the repeats in runs of at most 65532 / np, each a launch of its own
    const int64_t run = 65532 / np;
    for (int64_t first = 0; first < repeat; first += run) {
        const int64_t count = repeat - first < run ? repeat - first : run;
        const float *from[4];
        for (int i = 0; i < np; ++i) from[i] = planes[i] + first * stride;
        GsSpectrumArgs a{};
        const bool vec = gs_plane_set(a.set, from, np, count, stride, pitch, rows, cols);
        a.bands = bands;
        a.tiles = cols / tile;
        a.segs = segs;
        a.window = window;
        a.records = static_cast<double *>(records) + first * np * bands * segs * words;
        double *results = static_cast<double *>(out) + first * np * out_bands * words;
        const unsigned all = (unsigned)(np * count);
        if (bands > 0 && segs > 0) {
            const dim3 grid((unsigned)segs, (unsigned)bands, all);
            const hipError_t e = vec ? launch_tiles_of<true>(tile, grid, a, tab, s) : launch_tiles_of<false>(tile, grid, a, tab, s);
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(gs_spectrum_fold_k, dim3((unsigned)((words + 255) / 256), (unsigned)out_bands, all), dim3(256), 0, s,
                           a.records, bands, out_bands, segs, bins, results);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
