// gs_spectrum.hip -- tile-averaged power spectra of planes on the device (include/gs_hip.h: gs_fields_spectrum,
// gs_members_spectrum): the f32 radix-2 transform of every whole T x T tile of a plane, T = 16, 32, 64 or 128, its power
// added in f64 over segments of up to 16 tiles of a band of T rows, and the segments' records added per band.
//
// gs_spectrum_tiles_k: one workgroup of 4 waves per (plane, band, segment).  Per tile:
//   load     the tile's cells into LDS, 16 bytes per lane where gs_reads_16_bytes allows, each row's T reals at the head of
//            the row's slot of T/2 + 1 complex numbers; a cell that is not finite skips the tile (one workgroup-wide OR);
//   mean     the f64 halving order of gs_hip.h: a row's cells over min(T, 64) lanes (two cells a lane at T = 128) and xor
//            shuffles T/2 .. 1 -- lane 0 ends with ((p0 + pT/2) + (pT/4 + p3T/4)) + ..., the other lanes add the same pairs
//            swapped --, then the T row sums likewise in wave 0;
//   rows     256 / (T/2) rows at a time: the windowed reals go bit-reversed into a staging row of T complex numbers, a
//            thread owns one butterfly of one row per stage (a barrier between stages), and columns 0 .. T/2 of the result
//            replace the row's reals in its slot.  The slot pitch T/2 + 1 is odd, the staging pitch T + 1: the column pass's
//            walks over rows and the staging rows of one wave fall on different banks;
//   columns  the rows of the slots are permuted by bit reversal (a thread swaps a pair), then log2 T stages in place, a thread
//            taking butterflies whose column is the fastest index: consecutive lanes, consecutive 8-byte words;
//   power    re * re + im * im in f32, added to the thread's f64 accumulators: bin e = kr * (T/2 + 1) + kc belongs to thread
//            e % 256, ceil(T (T/2 + 1) / 256) accumulators in registers across the segment's tiles, from +0.0 in tile order.
// The record of a segment: T (T/2 + 1) f64 sums, then the tiles used and skipped as u64.
// gs_spectrum_fold_k: a thread per (plane, band, word) adds the band's records in ascending segment order from +0.0; a band
// that is not whole (the rows below the last whole band of a slab) and a band of no tiles are written as zeros.
//
// Every f32 operation is rounded on its own (-ffp-contract=off); the division by T T of the mean is a multiplication by the
// exact power of two.  The tables -- the window h[T] and the twiddles W[T/2] -- are formed by the host and travel by value
// with the launch.  T = 128 needs 71 KiB of LDS: the kernel's dynamic LDS limit is raised at its launch.
//
// Built with hipcc's default float mode (f32 denormals kept), as the other observables' units are.
#include "gs_kernels.h"
#include "gs_plane_scan.h"

namespace {

constexpr int kSpectrumSegment = 16; // tiles of a segment (gs_hip.h)

struct GsSpectrumTables {
    float h[128];           // the window, T used
    float wr[64], wi[64];   // the twiddles, T / 2 used
};

struct GsSpectrumArgs {
    GsPlaneSet set;
    int64_t bands;   // whole bands of a plane
    int64_t tiles;   // whole tiles of a band
    int64_t segs;    // segments of a band
    int32_t window;  // != 0: the window is applied
    double *records; // [plane][band][segment][T (T/2 + 1) + 2]
};

template <int T>
struct Geo {
    static constexpr int LOG = T == 16 ? 4 : (T == 32 ? 5 : (T == 64 ? 6 : 7));
    static constexpr int P = T / 2 + 1;                       // complex numbers of a row's slot
    static constexpr int HB = T / 2;                          // butterflies of a row (or column) per stage
    static constexpr int RB = 256 / HB < T ? 256 / HB : T;    // rows transformed at a time
    static constexpr int SP = T + 1;                          // pitch of a staging row, complex numbers
    static constexpr int BINS = T * P;
    static constexpr int NB = (BINS + 255) / 256;             // bins (accumulators) of a thread
    static constexpr int LPR = T < 64 ? T : 64;               // lanes that add a row
    static constexpr size_t LDS = (size_t)T * 8 + (size_t)BINS * 8 + (size_t)RB * SP * 8 + (size_t)HB * 8 + (size_t)T * 4 + 8;
};

template <int T>
__device__ __forceinline__ int bit_reversed(int i)
{
    return (int)(__brev((unsigned)i) >> (32 - Geo<T>::LOG));
}

// One butterfly of gs_hip.h on x[lo] and x[hi]: t = b w, x[lo] = a + t, x[hi] = a - t.
__device__ __forceinline__ void butterfly(float2 *x, int lo, int hi, float2 w)
{
    const float2 a = x[lo], b = x[hi];
    const float tr = b.x * w.x - b.y * w.y;
    const float ti = b.x * w.y + b.y * w.x;
    x[lo] = make_float2(a.x + tr, a.y + ti);
    x[hi] = make_float2(a.x - tr, a.y - ti);
}

// Grid (segments of a band, bands, planes) of workgroups of 256 threads; Geo<T>::LDS bytes of dynamic LDS.
template <int T, bool VEC>
__global__ __launch_bounds__(256) void gs_spectrum_tiles_k(GsSpectrumArgs a, GsSpectrumTables tab)
{
    using G = Geo<T>;
    extern __shared__ double gs_spectrum_lds[];
    double *rs = gs_spectrum_lds;                       // T row sums
    float2 *X = reinterpret_cast<float2 *>(rs + T);     // T slots of P complex numbers
    float2 *S = X + G::BINS;                            // RB staging rows of SP complex numbers
    float2 *W = S + G::RB * G::SP;                      // T / 2 twiddles
    float *H = reinterpret_cast<float *>(W + G::HB);    // T window values
    float *mean = H + T;
    float *Xr = reinterpret_cast<float *>(X);           // a row's reals: 2 P floats apart

    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;
    if (t < T) H[t] = tab.h[t];
    if (t < G::HB) W[t] = make_float2(tab.wr[t], tab.wi[t]);

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
        __syncthreads();                // the tile before has been added (and, for the first one, the tables are in place)
        const float *tile = plane + band * T * pitch + j * T;
        bool bad = false;
        for (int q = t; q < T * T / 4; q += 256) {
            const int r = q / (T / 4), c = q % (T / 4) * 4;
            const float *src = tile + r * pitch + c;
            const float4 v = VEC ? *reinterpret_cast<const float4 *>(src) : make_float4(src[0], src[1], src[2], src[3]);
            bad = bad || !(__builtin_isfinite(v.x) && __builtin_isfinite(v.y) && __builtin_isfinite(v.z) && __builtin_isfinite(v.w));
            float *dst = Xr + r * (2 * G::P) + c; // (8-byte aligned: 2 P and c are even)
            *reinterpret_cast<float2 *>(dst) = make_float2(v.x, v.y);
            *reinterpret_cast<float2 *>(dst + 2) = make_float2(v.z, v.w);
        }
        if (__syncthreads_or(bad ? 1 : 0)) { // (nobody has read the slots: the next tile may overwrite them)
            ++skipped;
            continue;
        }
        ++used;

        // the mean
        constexpr int RPW = 64 / G::LPR; // rows a wave adds at a time
        for (int r0 = 0; r0 < T; r0 += 4 * RPW) {
            const int r = r0 + wave * RPW + lane / G::LPR, i = lane % G::LPR;
            const float *row = Xr + r * (2 * G::P);
            double d = (double)row[i];
            if (T == 128) d = d + (double)row[i + 64];
#pragma unroll
            for (int m = G::LPR / 2; m >= 1; m >>= 1) d = d + __shfl_xor(d, m);
            if (i == 0) rs[r] = d;
        }
        __syncthreads();
        if (wave == 0) {
            double d = lane < T ? rs[lane] : 0.0; // (the lanes past T are never added to lane 0)
            if (T == 128) d = d + rs[lane + 64];
#pragma unroll
            for (int m = G::LPR / 2; m >= 1; m >>= 1) d = d + __shfl_xor(d, m);
            if (lane == 0) *mean = (float)(d * (1.0 / (double)(T * T))); // (a power of two: the product is the quotient)
        }
        __syncthreads();
        const float m = *mean;

        // the row transforms
        const int rb = t / G::HB, jb = t % G::HB;
        const bool on = rb < G::RB; // (T = 16: the tile's 128 butterflies of a stage leave half the threads idle)
        float2 *s = S + (on ? rb : 0) * G::SP;
        for (int r0 = 0; r0 < T; r0 += G::RB) {
            const int r = r0 + (on ? rb : 0);
            if (on) {
                const float *row = Xr + r * (2 * G::P);
#pragma unroll
                for (int k = 0; k < 2; ++k) {
                    const int e = jb + k * G::HB, c = bit_reversed<T>(e);
                    float v = row[c] - m;
                    if (a.window) v = (v * H[r]) * H[c];
                    s[e] = make_float2(v, 0.0f);
                }
            }
#pragma unroll
            for (int st = 0; st < G::LOG; ++st) {
                __syncthreads();
                if (on) {
                    const int h = 1 << st, k = jb & (h - 1), i = ((jb >> st) << (st + 1)) + k;
                    butterfly(s, i, i + h, W[k << (G::LOG - 1 - st)]);
                }
            }
            __syncthreads();
            // (s[jb] and s[T/2] are read here and written next round by this thread alone: no barrier behind the reads)
            if (on) {
                X[r * G::P + jb] = s[jb];
                if (jb == 0) X[r * G::P + G::HB] = s[G::HB];
            }
        }
        __syncthreads();

        // the column transforms
        for (int e = t; e < G::BINS; e += 256) {
            const int i = e / G::P, c = e % G::P, ri = bit_reversed<T>(i);
            if (i < ri) {
                const float2 u = X[i * G::P + c], v = X[ri * G::P + c];
                X[i * G::P + c] = v;
                X[ri * G::P + c] = u;
            }
        }
#pragma unroll
        for (int st = 0; st < G::LOG; ++st) {
            __syncthreads();
            const int h = 1 << st;
            for (int e = t; e < G::HB * G::P; e += 256) {
                const int b = e / G::P, c = e % G::P, k = b & (h - 1), i = ((b >> st) << (st + 1)) + k;
                butterfly(X, i * G::P + c, (i + h) * G::P + c, W[k << (G::LOG - 1 - st)]);
            }
        }
        __syncthreads();

        // the power
#pragma unroll
        for (int n = 0; n < G::NB; ++n) {
            const int e = t + 256 * n;
            if (e < G::BINS) {
                const float2 v = X[e];
                const float re2 = v.x * v.x, im2 = v.y * v.y;
                const float p = re2 + im2;
                acc[n] = acc[n] + (double)p;
            }
        }
    }

    double *rec = a.records + unit * (int64_t)(G::BINS + 2);
#pragma unroll
    for (int n = 0; n < G::NB; ++n) {
        const int e = t + 256 * n;
        if (e < G::BINS) rec[e] = acc[n];
    }
    if (t == 0) {
        unsigned long long *counts = reinterpret_cast<unsigned long long *>(rec + G::BINS);
        counts[0] = used;
        counts[1] = skipped;
    }
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
    GsSpectrumTables tab{};
    for (int i = 0; i < tile; ++i) tab.h[i] = h[i];
    for (int i = 0; i < tile / 2; ++i) {
        tab.wr[i] = w[2 * i];
        tab.wi[i] = w[2 * i + 1];
    }
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
