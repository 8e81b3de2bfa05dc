// gs_summary.hip -- summaries of planes on the device (include/gs_hip.h: gs_fields_summarize, gs_members_summarize).
//
// gs_row_summary_k writes one record per (plane, row): the row partial of the fold order that gs_hip.h defines (64 lane
// accumulators in f64 over columns 256 k + 4 l + j, then halved: p[0:32] + p[32:64], ...), the row's minimum, maximum and
// non-finite count.  A wave owns a row; its lanes read 16 B each (one 1 KiB wave-instruction per k), eight k ahead of the
// adds.  The field fold (rows added in ascending global row order) is the host's for Species -- the rows of several slabs
// and processes meet there -- and gs_summary_fold_k's for ensemble members, so that only two records per member leave the
// device.  HBM-bound: the f64 work is 4 operations per cell.
//
// Built with hipcc's default float mode (f32 denormals kept): a sub-normal cell counts as the value it is.
#include "gs_kernels.h"

namespace {

constexpr int kSumUnroll = 8; // k blocks of 256 columns whose loads a wave issues before it adds them

struct RowAcc {
    double s, q;
    float mn, mx;
    uint32_t nf;
};

// One cell of a row: `valid` = the column is inside the row.  A skipped cell adds +0.0, which leaves an accumulator that
// started at +0.0 bit for bit as it was (it never holds -0.0: +0 + -0 = +0 and x + -x = +0).
__device__ __forceinline__ void take(RowAcc &a, float x, bool valid)
{
    const bool fin = valid && __builtin_isfinite(x);
    const double d = fin ? (double)x : 0.0;
    a.s += d;
    a.q += d * d; // exact: a 24-bit significand squared fits in 53 bits
    a.mn = fminf(a.mn, fin ? x : __builtin_huge_valf());
    a.mx = fmaxf(a.mx, fin ? x : -__builtin_huge_valf());
    a.nf += (valid && !fin) ? 1u : 0u;
}

struct GsSumPlanes {
    const float *p[4];
};

// grid (row groups, planes), 4 waves per workgroup, one row per wave at a time (grid-stride over rows).
template <bool VEC>
__global__ __launch_bounds__(256) void gs_row_summary_k(GsSumPlanes planes, int64_t pitch, int64_t rows, int32_t cols,
                                                        GsRowSummary *out)
{
    const int lane = (int)(threadIdx.x & 63);
    const float *plane = planes.p[blockIdx.y];
    GsRowSummary *rec = out + (int64_t)blockIdx.y * rows;
    for (int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); r < rows; r += (int64_t)gridDim.x * 4) {
        const float *row = plane + r * pitch;
        RowAcc a{0.0, 0.0, __builtin_huge_valf(), -__builtin_huge_valf(), 0u};
        for (int c0 = 4 * lane; c0 < cols; c0 += 256 * kSumUnroll) {
            float4 x[kSumUnroll];
#pragma unroll
            for (int u = 0; u < kSumUnroll; ++u) {
                const int c = c0 + 256 * u;
                if (VEC && c + 3 < cols) {
                    x[u] = *reinterpret_cast<const float4 *>(row + c);
                } else {
                    x[u].x = c < cols ? row[c] : 0.0f;
                    x[u].y = c + 1 < cols ? row[c + 1] : 0.0f;
                    x[u].z = c + 2 < cols ? row[c + 2] : 0.0f;
                    x[u].w = c + 3 < cols ? row[c + 3] : 0.0f;
                }
            }
#pragma unroll
            for (int u = 0; u < kSumUnroll; ++u) {
                const int c = c0 + 256 * u;
                take(a, x[u].x, c < cols);
                take(a, x[u].y, c + 1 < cols);
                take(a, x[u].z, c + 2 < cols);
                take(a, x[u].w, c + 3 < cols);
            }
        }
        // lane combine: after the step of offset m lane l holds (its sum) + (lane l ^ m's); lane 0 ends with
        // ((p0 + p32) + (p16 + p48)) + ..., the halving order of gs_hip.h (the other lanes add the same pairs swapped)
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            a.s = a.s + __shfl_xor(a.s, m);
            a.q = a.q + __shfl_xor(a.q, m);
            a.mn = fminf(a.mn, __shfl_xor(a.mn, m));
            a.mx = fmaxf(a.mx, __shfl_xor(a.mx, m));
            a.nf += (uint32_t)__shfl_xor((int)a.nf, m);
        }
        if (lane == 0) {
            GsRowSummary o;
            o.sum = a.s;
            o.sum_sq = a.q;
            o.min = a.mn;
            o.max = a.mx;
            o.nonfinite = a.nf;
            o.pad = 0u;
            rec[r] = o;
        }
    }
}

// One thread per (member, species): the member's row records added in row order from +0.0.
__global__ __launch_bounds__(256) void gs_summary_fold_k(const GsRowSummary *rec, int64_t count, int64_t rows,
                                                         GsRowSummary *out)
{
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 2 * count) return;
    const int64_t member = g >> 1, species = g & 1;
    const GsRowSummary *p = rec + (species * count + member) * rows;
    double s = 0.0, q = 0.0;
    float mn = __builtin_huge_valf(), mx = -__builtin_huge_valf();
    uint32_t nf = 0u;
    for (int64_t r = 0; r < rows; ++r) {
        s = s + p[r].sum;
        q = q + p[r].sum_sq;
        mn = fminf(mn, p[r].min);
        mx = fmaxf(mx, p[r].max);
        nf += p[r].nonfinite;
    }
    GsRowSummary o;
    o.sum = s;
    o.sum_sq = q;
    o.min = mn;
    o.max = mx;
    o.nonfinite = nf;
    o.pad = 0u;
    out[g] = o;
}

} // namespace

hipError_t gs_launch_row_summary(const float *const *planes, int n, int64_t pitch, int64_t rows, int32_t cols,
                                 GsRowSummary *out, hipStream_t s)
{
    if (n < 1 || n > 4 || rows <= 0) return hipSuccess;
    GsSumPlanes p{};
    bool vec = pitch % 4 == 0;
    for (int i = 0; i < n; ++i) {
        p.p[i] = planes[i];
        vec = vec && reinterpret_cast<uintptr_t>(planes[i]) % 16 == 0;
    }
    const int64_t groups = (rows + 3) / 4;
    const dim3 grid((unsigned)(groups < 65536 ? groups : 65536), (unsigned)n);
    if (vec)
        hipLaunchKernelGGL(gs_row_summary_k<true>, grid, dim3(256), 0, s, p, pitch, rows, cols, out);
    else
        hipLaunchKernelGGL(gs_row_summary_k<false>, grid, dim3(256), 0, s, p, pitch, rows, cols, out);
    return hipGetLastError();
}

hipError_t gs_launch_summary_fold(const GsRowSummary *rec, int64_t count, int64_t rows, GsRowSummary *out, hipStream_t s)
{
    if (count <= 0) return hipSuccess;
    const int64_t blocks = (2 * count + 255) / 256;
    hipLaunchKernelGGL(gs_summary_fold_k, dim3((unsigned)blocks), dim3(256), 0, s, rec, count, rows, out);
    return hipGetLastError();
}
