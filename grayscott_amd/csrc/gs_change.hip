// gs_change.hip -- two planes compared on the device (include/gs_hip.h: gs_fields_compare, gs_members_compare).
//
// gs_row_change_k writes one record per (pair, row): the row partials of sum |d| and sum d * d, d = (double)a - (double)b,
// in the summaries' fold order (64 lane accumulators in f64 over columns 256 k + 4 l + j, then halved: p[0:32] + p[32:64],
// ...), the row's largest |d|, the count of cells whose 32 bits differ and the count of cells where a or b is not finite.
// It has the shape of gs_row_summary_k (gs_summary.hip): a wave owns a row; its lanes read 16 B of a and 16 B of b each
// (two 1 KiB wave-instructions per k), eight k ahead of the adds.  The field fold (rows added in ascending global row
// order) is the host's for Species and gs_change_fold_k's for ensemble members, so that only two records per member leave
// the device.  HBM-bound: the f64 work is 7 operations per cell pair (two conversions, a subtraction, a multiplication, two additions, a maximum).
//
// Built with hipcc's default float mode (f32 denormals kept): a sub-normal cell counts as the value it is.
#include "gs_kernels.h"

namespace {

constexpr int kChangeUnroll = 8; // k blocks of 256 columns whose loads a wave issues before it adds them

struct ChangeAcc {
    double s, q, mx;
    uint32_t df, nf;
};

// One cell of a row pair: `valid` = the column is inside the row.  A cell that is skipped or not comparable adds +0.0,
// which leaves an accumulator that started at +0.0 bit for bit as it was (it only ever holds sums of |d| and d * d >= +0).
__device__ __forceinline__ void take(ChangeAcc &acc, float a, float b, bool valid)
{
    const bool fin = valid && __builtin_isfinite(a) && __builtin_isfinite(b);
    const double d = fin ? (double)a - (double)b : 0.0; // one f64 subtraction
    const double ad = __builtin_fabs(d);
    acc.s += ad;
    acc.q += d * d;
    acc.mx = fmax(acc.mx, ad);
    acc.df += (valid && __float_as_uint(a) != __float_as_uint(b)) ? 1u : 0u;
    acc.nf += (valid && !fin) ? 1u : 0u;
}

__device__ __forceinline__ float4 load4(const float *row, int c, int cols, bool vec)
{
    float4 x;
    if (vec && c + 3 < cols) {
        x = *reinterpret_cast<const float4 *>(row + c);
    } else {
        x.x = c < cols ? row[c] : 0.0f;
        x.y = c + 1 < cols ? row[c + 1] : 0.0f;
        x.z = c + 2 < cols ? row[c + 2] : 0.0f;
        x.w = c + 3 < cols ? row[c + 3] : 0.0f;
    }
    return x;
}

struct GsChangePlanes {
    const float *a[4], *b[4];
};

// grid (row groups, pairs), 4 waves per workgroup, one row per wave at a time (grid-stride over rows).
template <bool VEC>
__global__ __launch_bounds__(256) void gs_row_change_k(GsChangePlanes planes, int64_t pitch, int64_t rows, int32_t cols,
                                                       GsRowChange *out)
{
    const int lane = (int)(threadIdx.x & 63);
    const float *plane_a = planes.a[blockIdx.y], *plane_b = planes.b[blockIdx.y];
    GsRowChange *rec = out + (int64_t)blockIdx.y * rows;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const float *ra = plane_a + r * pitch, *rb = plane_b + r * pitch;
        ChangeAcc acc{0.0, 0.0, 0.0, 0u, 0u};
        for (int c0 = 4 * lane; c0 < cols; c0 += 256 * kChangeUnroll) {
            float4 x[kChangeUnroll], y[kChangeUnroll];
#pragma unroll
            for (int u = 0; u < kChangeUnroll; ++u) {
                x[u] = load4(ra, c0 + 256 * u, cols, VEC);
                y[u] = load4(rb, c0 + 256 * u, cols, VEC);
            }
#pragma unroll
            for (int u = 0; u < kChangeUnroll; ++u) {
                const int c = c0 + 256 * u;
                take(acc, x[u].x, y[u].x, c < cols);
                take(acc, x[u].y, y[u].y, c + 1 < cols);
                take(acc, x[u].z, y[u].z, c + 2 < cols);
                take(acc, x[u].w, y[u].w, c + 3 < cols);
            }
        }
        // lane combine: after the step of offset m lane l holds (its sum) + (lane l ^ m's); lane 0 ends with
        // ((p0 + p32) + (p16 + p48)) + ..., the halving order of gs_hip.h (the other lanes add the same pairs swapped)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            acc.s = acc.s + __shfl_xor(acc.s, m);
            acc.q = acc.q + __shfl_xor(acc.q, m);
            acc.mx = fmax(acc.mx, __shfl_xor(acc.mx, m));
            acc.df += (uint32_t)__shfl_xor((int)acc.df, m);
            acc.nf += (uint32_t)__shfl_xor((int)acc.nf, m);
        }
        if (lane == 0) {
            GsRowChange o;
            o.sum_abs = acc.s;
            o.sum_sq = acc.q;
            o.max_abs = acc.mx;
            o.differing = acc.df;
            o.nonfinite = acc.nf;
            rec[r] = o;
        }
    }
}

// One thread per (member, species): the member's row records added in row order from +0.0.
__global__ __launch_bounds__(256) void gs_change_fold_k(const GsRowChange *rec, int64_t count, int64_t rows, GsChangeTotal *out)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 2 * count) return;
    const int64_t member = g >> 1, species = g & 1;
    const GsRowChange *p = rec + (species * count + member) * rows;
    GsChangeTotal o{0.0, 0.0, 0.0, 0ull, 0ull};
    for (int64_t r = 0; r < rows; ++r) {
        o.sum_abs = o.sum_abs + p[r].sum_abs;
        o.sum_sq = o.sum_sq + p[r].sum_sq;
        o.max_abs = fmax(o.max_abs, p[r].max_abs);
        o.differing += p[r].differing;
        o.nonfinite += p[r].nonfinite;
    }
    out[g] = o;
}

} // namespace

hipError_t gs_launch_row_change(const float *const *a, const float *const *b, int n, int64_t pitch, int64_t rows, int32_t cols,
                                GsRowChange *out, hipStream_t s)
{
    if (n < 1 || n > 4 || rows <= 0) return hipSuccess;
    GsChangePlanes p{};
    bool vec = pitch % 4 == 0;
    for (int i = 0; i < n; ++i) {
        p.a[i] = a[i];
        p.b[i] = b[i];
        vec = vec && reinterpret_cast<uintptr_t>(a[i]) % 16 == 0 && reinterpret_cast<uintptr_t>(b[i]) % 16 == 0;
    }
    const int64_t groups = (rows + 3) / 4;
    const dim3 grid((unsigned)(groups < 65536 ? groups : 65536), (unsigned)n);
    if (vec)
        hipLaunchKernelGGL(gs_row_change_k<true>, grid, dim3(256), 0, s, p, pitch, rows, cols, out);
    else
        hipLaunchKernelGGL(gs_row_change_k<false>, grid, dim3(256), 0, s, p, pitch, rows, cols, out);
    return hipGetLastError();
}

hipError_t gs_launch_change_fold(const GsRowChange *rec, int64_t count, int64_t rows, GsChangeTotal *out, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    const int64_t blocks = (2 * count + 255) / 256;
    hipLaunchKernelGGL(gs_change_fold_k, dim3((unsigned)blocks), dim3(256), 0, s, rec, count, rows, out);
    return hipGetLastError();
}
