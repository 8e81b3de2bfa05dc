// gs_reduce.hip -- reduced result images (include/gs_hip.h: gs_field_download_reduced and kin): a plane averaged over
// f x f blocks into a dense staging buffer, in one pass that reads every cell once and writes 1 / f^2 as many.
//
// The fold order is the header's: per block, every row's cells are added in f64 in ascending column order from +0.0 (the
// row partial), the row partials are added in ascending row order from +0.0, and the pixel is (float)(sum / count).  Both
// kernels keep to it literally; a cell outside the plane adds +0.0, which leaves an accumulator that started at +0.0 bit
// for bit as it was (it never holds -0.0: +0 + -0 = +0 and x + -x = +0), so edge blocks need no second code path.
//
//   gs_reduce_vec_k  f = 2 and f = 4: a lane owns a pixel and reads its block's rows as one float2 / float4 each -- a wave's
//                    load covers consecutive 128-byte lines -- UB blocks (8 row loads) ahead of the adds.
//   gs_reduce_lds_k  every other f: a workgroup owns one row of blocks over up to 1024 columns.  Its lanes read rows ACROSS
//                    (16 B per lane, 1 KiB per wave-instruction, up to 8 rows ahead of the adds) into LDS, where the
//                    transposition happens: 32 lanes per row then walk one block's columns each (block starts f | 1 floats
//                    apart: an odd stride, no bank conflicts), leave the row partial in the block's first two words, and
//                    one lane per pixel adds the partials in row order.
//
// HBM-bound: one f32 -> f64 conversion and one f64 add per cell.  Built with hipcc's default float mode (f32 denormals
// kept), as gs_summary.hip is: a sub-normal cell counts as the value it is and a sub-normal pixel is kept.
#include "gs_kernels.h"

#include <type_traits>

namespace {

constexpr int kRedRows = 8;        // rows a workgroup of gs_reduce_lds_k loads before it adds them
constexpr int kRedTileCols = 1024; // columns of its tile at most: 256 lanes x 16 B
constexpr int kRedMaxPix = 340;    // pixels of its tile at most (f = 3); two per lane at most
constexpr int kRedStride = 1200;   // floats of LDS per tile row: columns + one pad per pixel for even f (f = 6: 1008 + 168)

template <int F, int UB>
__global__ __launch_bounds__(256) void gs_reduce_vec_k(const float *row0, int pitch, int rows, int cols, int out_rows,
                                                       int out_cols, int vec, float *dst)
{
    using V = typename std::conditional<F == 2, float2, float4>::type;
    const int C = blockIdx.x * 256 + threadIdx.x;
    if (C >= out_cols) return;
    const int c = C * F;
    const int nc = cols - c < F ? cols - c : F;
    const bool whole = vec && nc == F;
    for (int R0 = blockIdx.y * UB; R0 < out_rows; R0 += gridDim.y * UB) {
        float x[UB][F][F];
#pragma unroll
        for (int u = 0; u < UB; ++u)
#pragma unroll
            for (int i = 0; i < F; ++i) {
                const int r = (R0 + u) * F + i;
                const float *row = row0 + (ptrdiff_t)r * pitch + c;
                if (r < rows && whole) {
                    const V v = *reinterpret_cast<const V *>(row);
                    const float *e = reinterpret_cast<const float *>(&v);
#pragma unroll
                    for (int j = 0; j < F; ++j) x[u][i][j] = e[j];
                } else {
#pragma unroll
                    for (int j = 0; j < F; ++j) x[u][i][j] = (r < rows && j < nc) ? row[j] : 0.0f;
                }
            }
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const int R = R0 + u;
            if (R >= out_rows) break;
            double sum = 0.0;
#pragma unroll
            for (int i = 0; i < F; ++i) {
                double p = 0.0;
#pragma unroll
                for (int j = 0; j < F; ++j) p = p + (double)x[u][i][j];
                sum = sum + p;
            }
            const int nr = rows - R * F < F ? rows - R * F : F;
            dst[(size_t)R * out_cols + C] = (float)(sum / (double)(nr * nc));
        }
    }
}

// grid (column tiles, rows of blocks); npix pixels = npix * f columns (a multiple of 4) per tile
__global__ __launch_bounds__(256) void gs_reduce_lds_k(const float *row0, int pitch, int rows, int cols, int f, int npix,
                                                       int out_rows, int out_cols, int vec, float *dst)
{
    __shared__ float tile[kRedRows * kRedStride];
    const int tid = (int)threadIdx.x;
    const int sp = f | 1;       // floats between the starts of two blocks of a tile row
    const int W = npix * f;     // columns of a tile
    const int C0 = blockIdx.x * npix, c0 = C0 * f;
    const int ct = 4 * tid;     // this lane's four columns of the tile ...
    const bool loads = ct < W;
    int off[4];                 // ... and where they go in a tile row
#pragma unroll
    for (int j = 0; j < 4; ++j) off[j] = (ct + j) / f * (sp - f) + ct + j;
    const int pu = tid >> 5, pl = tid & 31; // the row and the first pixel this lane walks
    for (int R = blockIdx.y; R < out_rows; R += gridDim.y) {
        const int nr = rows - R * f < f ? rows - R * f : f;
        double acc[2] = {0.0, 0.0};
        for (int rb = 0; rb < nr; rb += kRedRows) {
            const int n = nr - rb < kRedRows ? nr - rb : kRedRows;
            float4 x[kRedRows];
#pragma unroll
            for (int u = 0; u < kRedRows; ++u) {
                x[u] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (!loads || u >= n) continue;
                const int c = c0 + ct;
                const float *row = row0 + (ptrdiff_t)(R * f + rb + u) * pitch;
                if (vec && c + 3 < cols) {
                    x[u] = *reinterpret_cast<const float4 *>(row + c);
                } else {
                    x[u].x = c < cols ? row[c] : 0.0f;
                    x[u].y = c + 1 < cols ? row[c + 1] : 0.0f;
                    x[u].z = c + 2 < cols ? row[c + 2] : 0.0f;
                    x[u].w = c + 3 < cols ? row[c + 3] : 0.0f;
                }
            }
            if (loads) {
#pragma unroll
                for (int u = 0; u < kRedRows; ++u) {
                    float *t = tile + u * kRedStride;
                    t[off[0]] = x[u].x;
                    t[off[1]] = x[u].y;
                    t[off[2]] = x[u].z;
                    t[off[3]] = x[u].w;
                }
            }
            __syncthreads();
            // row partials: 32 lanes per row, a block each, its cells in ascending column order
            if (pu < n)
                for (int p = pl; p < npix; p += 32) {
                    float *b = tile + pu * kRedStride + p * sp;
                    double s = 0.0;
                    for (int i = 0; i < f; ++i) s = s + (double)b[i];
                    const unsigned long long bits = (unsigned long long)__double_as_longlong(s);
                    b[0] = __uint_as_float((unsigned)bits);
                    b[1] = __uint_as_float((unsigned)(bits >> 32));
                }
            __syncthreads();
            // block sums: a lane per pixel, the partials in ascending row order
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int p = tid + 256 * k;
                if (p >= npix) continue;
                for (int u = 0; u < n; ++u) {
                    const float *b = tile + u * kRedStride + p * sp;
                    const unsigned long long bits = (unsigned long long)__float_as_uint(b[0]) | ((unsigned long long)__float_as_uint(b[1]) << 32);
                    acc[k] = acc[k] + __longlong_as_double((long long)bits);
                }
            }
            __syncthreads();
        }
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int p = tid + 256 * k, C = C0 + p;
            if (p >= npix || C >= out_cols) continue;
            const int nc = cols - C * f < f ? cols - C * f : f;
            dst[(size_t)R * out_cols + C] = (float)(acc[k] / (double)(nr * nc));
        }
    }
}

} // namespace

hipError_t gs_launch_reduce(const float *row0, int32_t pitch, int32_t rows, int32_t cols, int32_t f, float *dst, hipStream_t s)
{
    if (rows <= 0 || cols <= 0) return hipSuccess;
    if (f < 2 || f > 64) return hipErrorInvalidValue;
    const int out_rows = (rows + f - 1) / f, out_cols = (cols + f - 1) / f;
    const int vec = pitch % 4 == 0 && reinterpret_cast<uintptr_t>(row0) % 16 == 0;
    if (f == 2 || f == 4) {
        const int ub = f == 2 ? 4 : 2;
        const int groups = (out_rows + ub - 1) / ub;
        const dim3 grid((unsigned)((out_cols + 255) / 256), (unsigned)(groups < 32768 ? groups : 32768));
        if (f == 2)
            hipLaunchKernelGGL((gs_reduce_vec_k<2, 4>), grid, dim3(256), 0, s, row0, pitch, rows, cols, out_rows, out_cols, vec, dst);
        else
            hipLaunchKernelGGL((gs_reduce_vec_k<4, 2>), grid, dim3(256), 0, s, row0, pitch, rows, cols, out_rows, out_cols, vec, dst);
        return hipGetLastError();
    }
    int npix = kRedTileCols / f;
    if (npix > kRedMaxPix) npix = kRedMaxPix;
    npix &= ~3; // tiles begin at a multiple of 4 columns (f = 64: 16 pixels)
    if (npix * (f | 1) > kRedStride) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((out_cols + npix - 1) / npix), (unsigned)(out_rows < 32768 ? out_rows : 32768));
    hipLaunchKernelGGL(gs_reduce_lds_k, grid, dim3(256), 0, s, row0, pitch, rows, cols, f, npix, out_rows, out_cols, vec, dst);
    return hipGetLastError();
}
