// gs_time_stats.hip -- per-cell statistics over the samples of a run (include/gs_hip.h: gs_time_stats_accumulate,
// gs_time_stats_result): the accumulators live on the device and one launch adds one sample of up to four planes.
//
// gs_tstat_accumulate_k<GROUPS, VEC> reads a sample and reads, updates and writes back the accumulators of the selected
// groups (GROUPS, a template parameter: a group that is not selected costs no instruction and no traffic):
//   GS_TSTAT_SUM        sum = sum + (double)x                               f64
//   GS_TSTAT_SQUARES    squares = squares + (double)x * (double)x           f64 (the product of two f32 is exact in f64)
//   GS_TSTAT_EXTREMES   min = x < min ? x : min;  max = x > max ? x : max   f32, strict comparisons: a NaN never replaces an
//                                                                           extreme, nor does a zero one of the other sign
//   GS_TSTAT_CROSSINGS  if x is set (gs_is_set of gs_plane_scan.h): set_count += 1, and first_stamp = stamp where it still
//                       holds 0xffffffff                                    u32
// It has the shape of gs_row_change_k (gs_change.hip): a wave owns a row; a lane owns four consecutive columns of a block of
// 256 -- one 16-byte load of the sample, two 16-byte loads and stores per f64 accumulator, one per f32 or u32 accumulator --
// and the wave issues every load of kUnroll blocks before the first addition.  HBM-bound read-modify-write: 4 + 2 x (8 + 8 +
// 4 + 4 + 4 + 4) = 68 bytes per cell with every group selected.  VEC = false is the ragged form (rows that do not begin on
// 16-byte boundaries): per-column accesses at gs_lane_columns' clamped columns, stores to columns below `cols` alone.
//
// Built with hipcc's default float mode (f32 denormals kept): a sub-normal sample counts as the value it is.
#include "gs_kernels.h"
#include "gs_plane_scan.h"

namespace {

constexpr uint32_t kSum = 1, kSquares = 2, kExtremes = 4, kCrossings = 8; // GS_TSTAT_SUM .. GS_TSTAT_CROSSINGS
constexpr uint32_t kNever = 0xffffffffu;                                  // first_stamp of a cell that was never set

// Blocks of 256 columns whose loads a wave issues before it adds them: as many as keep what a lane holds of them -- 4 VGPRs
// of sample, 8 per f64 accumulator, 4 per f32 or u32 one -- within 96 VGPRs, at least two (profiles/time_stats.md).
constexpr int tstat_unroll(uint32_t groups)
{
    const int held = 4 + ((groups & kSum) ? 8 : 0) + ((groups & kSquares) ? 8 : 0) + ((groups & kExtremes) ? 8 : 0) +
                     ((groups & kCrossings) ? 8 : 0);
    return 96 / held >= 8 ? 8 : 96 / held >= 4 ? 4 : 2;
}

struct GsTstatLaunch {
    const float *x[4];
    GsTstatAcc acc;
    int64_t pitch, rows;
    float t[4];
    uint32_t flip[4];
    uint32_t stamp;
    int32_t cols;
};

// A lane's four columns of an array of T: one aligned access of 4 T (16 bytes, or two of 16 for f64), or the ragged form.
template <typename T, bool VEC>
__device__ __forceinline__ void load_quad(T (&v)[4], const T *row, const GsLaneColumns &at)
{
    if (VEC) {
        typedef T V __attribute__((ext_vector_type(4)));
        const V x = *reinterpret_cast<const V *>(row + at.cv);
        v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
    } else {
        v[0] = row[at.l0], v[1] = row[at.l1], v[2] = row[at.l2], v[3] = row[at.l3];
    }
}

// ... written back: columns c .. c + 3 where the lane is inside the row (16-byte form: the whole quad, which ends inside the
// pitch), or those below `cols` one by one.
template <typename T, bool VEC>
__device__ __forceinline__ void store_quad(T *row, const T (&v)[4], int c, int cols)
{
    if (VEC) {
        typedef T V __attribute__((ext_vector_type(4)));
        V x;
        x.x = v[0], x.y = v[1], x.z = v[2], x.w = v[3];
        if (c < cols) *reinterpret_cast<V *>(row + c) = x;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c + j < cols) row[c + j] = v[j];
    }
}

// grid (row groups, planes), 4 waves per workgroup, one row per wave at a time (grid-stride over rows).
template <uint32_t GROUPS, bool VEC>
__global__ __launch_bounds__(256) void gs_tstat_accumulate_k(GsTstatLaunch a)
{
    constexpr int U = tstat_unroll(GROUPS);
    constexpr bool S = (GROUPS & kSum) != 0, Q = (GROUPS & kSquares) != 0, E = (GROUPS & kExtremes) != 0,
                   C = (GROUPS & kCrossings) != 0;
    const int lane = (int)(threadIdx.x & 63);
    const int y = (int)blockIdx.y;
    const float *plane = a.x[y];
    const int64_t first = (int64_t)y * a.acc.plane_stride;
    const float t = a.t[y];
    const uint32_t flip = a.flip[y], stamp = a.stamp;
    const int cols = a.cols;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < a.rows; r += (int64_t)gridDim.x * 4) {
        const int64_t at_row = first + r * a.pitch;
        const float *xr = plane + r * a.pitch;
        double *sr = nullptr, *qr = nullptr;
        float *mnr = nullptr, *mxr = nullptr;
        uint32_t *nr = nullptr, *fr = nullptr;
        if (S) sr = a.acc.sum + at_row;
        if (Q) qr = a.acc.squares + at_row;
        if (E) mnr = a.acc.mn + at_row, mxr = a.acc.mx + at_row;
        if (C) nr = a.acc.set_count + at_row, fr = a.acc.first_stamp + at_row;
        for (int c0 = 4 * lane; c0 < cols; c0 += 256 * U) {
            float x[U][4], mn[U][4], mx[U][4];
            double s[U][4], q[U][4];
            uint32_t n[U][4], f[U][4];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const GsLaneColumns at = gs_lane_columns(c0 + 256 * u, cols);
                load_quad<float, VEC>(x[u], xr, at);
                if (S) load_quad<double, VEC>(s[u], sr, at);
                if (Q) load_quad<double, VEC>(q[u], qr, at);
                if (E) load_quad<float, VEC>(mn[u], mnr, at), load_quad<float, VEC>(mx[u], mxr, at);
                if (C) load_quad<uint32_t, VEC>(n[u], nr, at), load_quad<uint32_t, VEC>(f[u], fr, at);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int c = c0 + 256 * u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float v = x[u][j];
                    if (S) s[u][j] = s[u][j] + (double)v;
                    if (Q) q[u][j] = q[u][j] + (double)v * (double)v;
                    if (E) {
                        mn[u][j] = v < mn[u][j] ? v : mn[u][j];
                        mx[u][j] = v > mx[u][j] ? v : mx[u][j];
                    }
                    if (C) {
                        const bool set = gs_is_set(v, flip, t);
                        n[u][j] += set ? 1u : 0u;
                        f[u][j] = (set && f[u][j] == kNever) ? stamp : f[u][j];
                    }
                }
                if (S) store_quad<double, VEC>(sr, s[u], c, cols);
                if (Q) store_quad<double, VEC>(qr, q[u], c, cols);
                if (E) store_quad<float, VEC>(mnr, mn[u], c, cols), store_quad<float, VEC>(mxr, mx[u], c, cols);
                if (C) store_quad<uint32_t, VEC>(nr, n[u], c, cols), store_quad<uint32_t, VEC>(fr, f[u], c, cols);
            }
        }
    }
}

// The accumulators whose reset value is no run of zero bytes -- min, max, first_stamp --, one per blockIdx.y.
struct GsTstatFill {
    uint32_t *p[3];
    uint32_t value[3];
    int64_t count; // elements of each
};

__global__ __launch_bounds__(256) void gs_tstat_reset_k(GsTstatFill fill)
{
    uint32_t *p = fill.p[blockIdx.y];
    const uint32_t value = fill.value[blockIdx.y];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < fill.count; i += (int64_t)gridDim.x * 256) p[i] = value;
}

constexpr int kMean = 0, kVariance = 1, kMin = 2, kMax = 3, kOccupancy = 4, kArrival = 5; // GS_TSTAT_MEAN .. GS_TSTAT_ARRIVAL

// One result plane from one plane's accumulators (`acc` points at them): f64 throughout, every operation rounded once -- the
// divisions are the compiler's IEEE sequence --, one conversion to f32 at the end.  grid (blocks of 256 columns, row groups).
template <int WHICH>
__global__ __launch_bounds__(256) void gs_tstat_result_k(GsTstatAcc acc, int64_t pitch, int64_t rows, int32_t cols, double n, float *out)
{
    const int c = (int)(blockIdx.x * 256 + threadIdx.x);
    if (c >= cols) return;
    for (int64_t r = blockIdx.y; r < rows; r += gridDim.y) {
        const int64_t i = r * pitch + c;
        float v;
        if (WHICH == kMean) {
            v = (float)(acc.sum[i] / n);
        } else if (WHICH == kVariance) {
            const double m = acc.sum[i] / n;
            const double d = acc.squares[i] / n - m * m;
            v = (float)(!(d <= 0.0) ? d : 0.0); // (a NaN stays NaN)
        } else if (WHICH == kMin) {
            v = acc.mn[i];
        } else if (WHICH == kMax) {
            v = acc.mx[i];
        } else if (WHICH == kOccupancy) {
            v = (float)((double)acc.set_count[i] / n);
        } else {
            const uint32_t f = acc.first_stamp[i];
            v = f == kNever ? -1.0f : (float)f;
        }
        out[i] = v;
    }
}

template <uint32_t GROUPS>
void launch_accumulate(bool vec, dim3 grid, const GsTstatLaunch &a, hipStream_t s)
{
    if (vec)
        hipLaunchKernelGGL((gs_tstat_accumulate_k<GROUPS, true>), grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((gs_tstat_accumulate_k<GROUPS, false>), grid, dim3(256), 0, s, a);
}

} // namespace

hipError_t gs_launch_tstat_accumulate(const float *const *planes, int np, int64_t pitch, int64_t rows, int32_t cols, uint32_t groups,
                                      const GsTstatAcc &acc, const float *t, const uint32_t *flip, uint32_t stamp,
                                      int64_t max_groups, hipStream_t s)
{
    if (np < 1 || np > 4 || rows <= 0 || cols <= 0) return hipSuccess;
    if (groups < 1 || groups > 15) return hipErrorInvalidValue;
    GsTstatLaunch a{};
    a.acc = acc;
    a.pitch = pitch, a.rows = rows, a.cols = cols, a.stamp = stamp;
    for (int i = 0; i < np; ++i) a.x[i] = planes[i], a.t[i] = t[i], a.flip[i] = flip[i];
    // the 16-byte form: every sample row on a 16-byte boundary; the accumulators share the pitch and begin on 256 bytes
    const bool vec = gs_reads_16_bytes(planes, np, 1, 0, pitch) && acc.plane_stride % 4 == 0;
    int64_t wg;
    if (!gs_scan_groups(rows, 0, max_groups, np, wg)) return hipErrorInvalidValue;
    const dim3 grid((unsigned)wg, (unsigned)np);
    switch (groups) {
#define GS_TSTAT_CASE(G) case G: launch_accumulate<G>(vec, grid, a, s); break;
        GS_TSTAT_CASE(1) GS_TSTAT_CASE(2) GS_TSTAT_CASE(3) GS_TSTAT_CASE(4) GS_TSTAT_CASE(5)
        GS_TSTAT_CASE(6) GS_TSTAT_CASE(7) GS_TSTAT_CASE(8) GS_TSTAT_CASE(9) GS_TSTAT_CASE(10)
        GS_TSTAT_CASE(11) GS_TSTAT_CASE(12) GS_TSTAT_CASE(13) GS_TSTAT_CASE(14) GS_TSTAT_CASE(15)
#undef GS_TSTAT_CASE
    }
    return hipGetLastError();
}

hipError_t gs_launch_tstat_reset(int np, uint32_t groups, const GsTstatAcc &acc, hipStream_t s)
{
    const int64_t count = (int64_t)np * acc.plane_stride;
    if (np < 1 || count <= 0) return hipSuccess;
    hipError_t e = hipSuccess;
    if (groups & kSum) e = hipMemsetAsync(acc.sum, 0, (size_t)count * sizeof(double), s);
    if (e == hipSuccess && (groups & kSquares)) e = hipMemsetAsync(acc.squares, 0, (size_t)count * sizeof(double), s);
    if (e == hipSuccess && (groups & kCrossings)) e = hipMemsetAsync(acc.set_count, 0, (size_t)count * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    GsTstatFill fill{};
    fill.count = count;
    unsigned n = 0;
    if (groups & kExtremes) {
        fill.p[n] = reinterpret_cast<uint32_t *>(acc.mn), fill.value[n++] = 0x7f800000u; // +inf
        fill.p[n] = reinterpret_cast<uint32_t *>(acc.mx), fill.value[n++] = 0xff800000u; // -inf
    }
    if (groups & kCrossings) fill.p[n] = acc.first_stamp, fill.value[n++] = kNever;
    if (n == 0) return hipSuccess;
    const int64_t blocks = (count + 255) / 256;
    hipLaunchKernelGGL(gs_tstat_reset_k, dim3((unsigned)(blocks < 4096 ? blocks : 4096), n), dim3(256), 0, s, fill);
    return hipGetLastError();
}

hipError_t gs_launch_tstat_result(int which, int plane, const GsTstatAcc &acc, int64_t pitch, int64_t rows, int32_t cols, uint64_t n,
                                  float *out, hipStream_t s)
{
    if (rows <= 0 || cols <= 0) return hipSuccess;
    GsTstatAcc at = acc;
    const int64_t off = (int64_t)plane * acc.plane_stride;
    if (at.sum) at.sum += off;
    if (at.squares) at.squares += off;
    if (at.mn) at.mn += off, at.mx += off;
    if (at.set_count) at.set_count += off, at.first_stamp += off;
    const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)(rows < 4096 ? rows : 4096));
    const double dn = (double)n;
    switch (which) {
#define GS_TSTAT_CASE(W) case W: hipLaunchKernelGGL(gs_tstat_result_k<W>, grid, dim3(256), 0, s, at, pitch, rows, cols, dn, out); break;
        GS_TSTAT_CASE(kMean) GS_TSTAT_CASE(kVariance) GS_TSTAT_CASE(kMin) GS_TSTAT_CASE(kMax) GS_TSTAT_CASE(kOccupancy)
        GS_TSTAT_CASE(kArrival)
#undef GS_TSTAT_CASE
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
