// gs_spectrum_tile.h -- the per-tile work of the power spectra, one body for the whole-grid kernel (gs_spectrum.hip) and the
// regional one (gs_region_spectrum.hip): the rule of include/gs_hip.h for one T x T tile, T = 16, 32, 64 or 128, by a
// workgroup of 4 waves.  Per tile:
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
//            e % 256, ceil(T (T/2 + 1) / 256) accumulators in registers across a segment's tiles, from +0.0 in tile order.
// The record of a segment: T (T/2 + 1) f64 sums, then the tiles used and skipped as u64 (gs_spectrum_write_record).
//
// Every f32 operation is rounded on its own (-ffp-contract=off); the division by T T of the mean is a multiplication by the
// exact power of two.  The tables -- the window h[T] and the twiddles W[T/2] -- are formed by the host and travel by value
// with the launch.  T = 128 needs 71 KiB of LDS: a kernel's dynamic LDS limit is raised at its launch.
#pragma once
#include "gs_kernels.h"

namespace {

constexpr int kSpectrumSegment = 16; // tiles of a segment (gs_hip.h)

struct GsSpectrumTables {
    float h[128];           // the window, T used
    float wr[64], wi[64];   // the twiddles, T / 2 used
};

// The tables of a launch from the host's: h[tile], and w as tile / 2 (re, im) pairs.
inline GsSpectrumTables gs_spectrum_tables_of(int32_t tile, const float *h, const float *w)
{
    GsSpectrumTables tab{};
    for (int i = 0; i < tile; ++i) tab.h[i] = h[i];
    for (int i = 0; i < tile / 2; ++i) {
        tab.wr[i] = w[2 * i];
        tab.wi[i] = w[2 * i + 1];
    }
    return tab;
}

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

// A workgroup's Geo<T>::LDS bytes of dynamic LDS, taken apart.
template <int T>
struct SpectrumLds {
    double *rs;  // T row sums
    float2 *X;   // T slots of P complex numbers
    float2 *S;   // RB staging rows of SP complex numbers
    float2 *W;   // T / 2 twiddles
    float *H;    // T window values
    float *mean;
};

// The parts of `lds`, and the tables put into theirs (in place for every thread after the next barrier: a tile begins with one).
template <int T>
__device__ __forceinline__ SpectrumLds<T> gs_spectrum_lds_parts(double *lds, const GsSpectrumTables &tab)
{
    using G = Geo<T>;
    SpectrumLds<T> l;
    l.rs = lds;
    l.X = reinterpret_cast<float2 *>(l.rs + T);
    l.S = l.X + G::BINS;
    l.W = l.S + G::RB * G::SP;
    l.H = reinterpret_cast<float *>(l.W + G::HB);
    l.mean = l.H + T;
    const int t = (int)threadIdx.x;
    if (t < T) l.H[t] = tab.h[t];
    if (t < G::HB) l.W[t] = make_float2(tab.wr[t], tab.wi[t]);
    return l;
}

// The tile of T x T cells at `tile` (rows `pitch` floats apart) by a workgroup of 256 threads: its power added to acc[] --
// thread t's accumulator n is bin t + 256 n --, or, if it holds a cell that is not finite, nothing: true is returned for a
// skipped tile.  Uniform: every thread takes every barrier and sees the same verdict.
template <int T, bool VEC>
__device__ __forceinline__ bool gs_spectrum_tile(const float *tile, int64_t pitch, int32_t window, const SpectrumLds<T> &l,
                                                 double (&acc)[Geo<T>::NB])
{
    using G = Geo<T>;
    double *rs = l.rs;
    float2 *X = l.X, *S = l.S, *W = l.W;
    float *H = l.H, *mean = l.mean;
    float *Xr = reinterpret_cast<float *>(X); // a row's reals: 2 P floats apart
    const int t = (int)threadIdx.x, lane = t & 63, wave = t >> 6;

    __syncthreads(); // the tile before has been added (and, for the first one, the tables are in place)
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
    if (__syncthreads_or(bad ? 1 : 0)) return true; // (nobody has read the slots: the next tile may overwrite them)

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
                if (window) v = (v * H[r]) * H[c];
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
    return false;
}

// A segment's record at `rec`: the threads' accumulators, then {used, skipped}.
template <int T>
__device__ __forceinline__ void gs_spectrum_write_record(double *rec, const double (&acc)[Geo<T>::NB], unsigned long long used,
                                                         unsigned long long skipped)
{
    using G = Geo<T>;
    const int t = (int)threadIdx.x;
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

} // namespace
