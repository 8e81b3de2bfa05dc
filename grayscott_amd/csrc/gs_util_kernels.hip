// gs_util_kernels.hip -- plane utilities that are not arithmetic-flavour dependent.
//
// colormap is the per-pixel work of data-to-pics (V plane -> RGB8 through a palette).
// fill_rect backs Concentration::zeros / ones / fill_slice
// (/root/reference/data/src/concentration/mod.rs:205-243) directly in HBM: the seed
// rectangle of Species::new (:36-59) is written on the device, there is no host staging
// copy to upload (contrast ImageConcentration, data/src/concentration/gpu/image/mod.rs:86-131).
#include "gs_kernels.h"

namespace {
__global__ __launch_bounds__(256) void gs_fill_rect_k(float *row0, int pitch, int r0, int c0,
                                                      int c1, float value)
{
    const int r = r0 + blockIdx.y;
    const int c = c0 + blockIdx.x * 256 + threadIdx.x;
    if (c < c1) row0[(ptrdiff_t)r * pitch + c] = value;
}
// A plane's `cols` columns without its padding, row after row: the staging copy of gs_field_download_async.  (Not
// hipMemcpy2DAsync: a device-to-device copy may go to the same copy engines that carry the images to the host, and an
// image then leaves every 168 us where the link takes 152 -- tools/ubench/d2h_probe.hip, tools/call_pattern.py.)
template <typename T>
__global__ __launch_bounds__(256) void gs_pack_rows_k(const float *row0, int pitch, int rows, int cols_t, T *dst)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols_t) return;
    for (int r = blockIdx.y; r < rows; r += gridDim.y)
        dst[(size_t)r * cols_t + c] = reinterpret_cast<const T *>(row0 + (ptrdiff_t)r * pitch)[c];
}
// Colour mapping of a result plane, data-to-pics/src/main.rs:139-144:
//     let color = ui::GRADIENT.eval_continuous((ui::AMPLITUDE_SCALE * value).into());
// i.e. an f32 multiply, widened to f64, handed to colorous 1.0.16 (Cargo.lock:389-392; the crate is not
// vendored).  Its sequential gradients are a port of d3-scale-chromatic's `ramp`: a table of n colours
// indexed with floor(t * n) clamped to [0, n - 1]; a NaN or negative t lands on entry 0 (saturating
// float -> usize cast).  The table itself is DATA handed in by the caller (for the reference: the 256
// entries of colorous::INFERNO), so only that indexing rule is restated here.
__global__ __launch_bounds__(256) void gs_colormap_k(const float *row0, int pitch, int rows, int cols, float scale,
                                                     const uint8_t *palette, int n, uint8_t *rgb)
{
    const int c = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (c >= cols || r >= rows) return;
    const double t = (double)(scale * row0[(ptrdiff_t)r * pitch + c]);
    const double x = floor(t * (double)n);
    const int i = !(x >= 0.0) ? 0 : (x >= (double)n ? n - 1 : (int)x);
    uint8_t *px = rgb + ((size_t)r * cols + c) * 3;
    px[0] = palette[3 * i];
    px[1] = palette[3 * i + 1];
    px[2] = palette[3 * i + 2];
}
// The probe of gs_fields_place: one pass that reads two blocks and writes both back, word for word what it read (the
// XOR with a kernel argument that is zero at run time keeps the compiler from dropping the stores) -- the HBM traffic of
// one time step on a slot's two planes, and the blocks keep their contents.  Two 1 GiB blocks of ONE physical region
// ("group") take 0.86-0.96 ms, two of different groups 0.72-0.79 ms (tools/ubench/hbm_kinds.hip, profiles/r06_placement.md).
__global__ __launch_bounds__(256) void gs_pair_probe_k(uint4 *x, uint4 *y, size_t n, uint32_t zero)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        uint4 a = x[i], b = y[i];
        a.x ^= zero; a.y ^= zero; a.z ^= zero; a.w ^= zero;
        b.x ^= zero; b.y ^= zero; b.z ^= zero; b.w ^= zero;
        x[i] = a;
        y[i] = b;
    }
}
// Species::new's pattern in every member of an ensemble (dense [members, rows, cols] planes; 64-bit indices).
__global__ void gs_ens_seed_k(float *u, float *v, uint64_t total, int32_t rows, int32_t cols, int32_t r0, int32_t r1,
                              int32_t c0, int32_t c1)
{
    const uint64_t cells = (uint64_t)rows * (uint64_t)cols;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t in = (uint32_t)(i % cells); // a member has < 2^31 cells
        const int32_t r = (int32_t)(in / (uint32_t)cols), c = (int32_t)(in - (uint32_t)r * (uint32_t)cols);
        const bool spot = r >= r0 && r < r1 && c >= c0 && c < c1;
        u[i] = spot ? 0.0f : 1.0f;
        v[i] = spot ? 1.0f : 0.0f;
    }
}
// Ensembles with an active set (gs_members_set_active): U and V of the listed members from one slot of the ensemble to the
// other, so that a member that no longer advances holds the same bits in both.  T = uint4 (16 bytes per lane; `per` and
// member offsets in units of T) when a member's cell count is a multiple of 4, else uint32_t.  Workgroup b copies chunk
// b % chunks -- kMirrorChunk elements of T per plane -- of member list[b / chunks]; member offsets are 64-bit.
constexpr uint32_t kMirrorChunk = 1024;
template <typename T>
__global__ __launch_bounds__(256) void gs_members_mirror_k(const uint32_t *list, const T *su, const T *sv, T *du, T *dv,
                                                           uint32_t per, uint32_t chunks)
{
    const uint32_t m = blockIdx.x / chunks, chunk = blockIdx.x - m * chunks;
    const uint64_t off = (uint64_t)list[m] * per;
    const uint32_t i0 = chunk * kMirrorChunk, i1 = i0 + kMirrorChunk < per ? i0 + kMirrorChunk : per;
    for (uint32_t i = i0 + threadIdx.x; i < i1; i += 256) {
        du[off + i] = su[off + i];
        dv[off + i] = sv[off + i];
    }
}

} // namespace

hipError_t gs_launch_members_mirror(const uint32_t *list, uint64_t n, const float *src_u, const float *src_v, float *dst_u,
                                    float *dst_v, uint64_t cells, hipStream_t s)
{
    if (n == 0 || cells == 0) return hipSuccess;
    if (!list || cells > 0x7fffffffull) return hipErrorInvalidValue;
    const bool wide = cells % 4 == 0 && (reinterpret_cast<uintptr_t>(src_u) | reinterpret_cast<uintptr_t>(src_v) |
                                         reinterpret_cast<uintptr_t>(dst_u) | reinterpret_cast<uintptr_t>(dst_v)) % 16 == 0;
    uint32_t per = (uint32_t)(wide ? cells / 4 : cells), chunks = (per + kMirrorChunk - 1) / kMirrorChunk;
    const void *fn = wide ? reinterpret_cast<const void *>(&gs_members_mirror_k<uint4>)
                          : reinterpret_cast<const void *>(&gs_members_mirror_k<uint32_t>);
    const uint64_t per_launch = (uint64_t)kGsEnsMaxGroups / chunks; // members per launch (chunks <= 2^21: cells < 2^31)
    if (per_launch == 0) return hipErrorInvalidConfiguration;
    for (uint64_t m0 = 0; m0 < n; m0 += per_launch) {
        const uint32_t *l = list + m0;
        const uint64_t count = n - m0 < per_launch ? n - m0 : per_launch;
        void *kargs[] = {&l, &src_u, &src_v, &dst_u, &dst_v, &per, &chunks};
        const hipError_t e = hipLaunchKernel(fn, dim3((unsigned)(count * chunks)), dim3(256), kargs, 0, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t gs_launch_ens_seed(float *u, float *v, uint64_t members, int32_t rows, int32_t cols, int32_t r0, int32_t r1,
                              int32_t c0, int32_t c1, hipStream_t s)
{
    uint64_t total = members * (uint64_t)rows * (uint64_t)cols;
    if (total == 0) return hipSuccess;
    const uint64_t want = (total + 255) / 256;
    const unsigned grid = (unsigned)(want < 65536 ? want : 65536);
    void *kargs[] = {&u, &v, &total, &rows, &cols, &r0, &r1, &c0, &c1};
    return hipLaunchKernel(reinterpret_cast<const void *>(&gs_ens_seed_k), dim3(grid), dim3(256), kargs, 0, s);
}

hipError_t gs_launch_pair_probe(void *x, void *y, size_t bytes, hipStream_t s)
{
    size_t n = bytes / sizeof(uint4);
    if (n == 0) return hipSuccess;
    uint4 *px = static_cast<uint4 *>(x), *py = static_cast<uint4 *>(y);
    uint32_t zero = 0;
    const size_t want = (n + 255) / 256;
    const unsigned grid = (unsigned)(want < 4096 ? want : 4096);
    void *kargs[] = {&px, &py, &n, &zero};
    return hipLaunchKernel(reinterpret_cast<const void *>(&gs_pair_probe_k), dim3(grid), dim3(256), kargs, 0, s);
}

hipError_t gs_launch_colormap(const float *row0, int32_t pitch, int32_t rows, int32_t cols, float scale,
                              const uint8_t *palette, int32_t n, uint8_t *rgb, hipStream_t s)
{
    if (rows <= 0 || cols <= 0) return hipSuccess;
    for (int32_t b0 = 0; b0 < rows; b0 += 32768) { // gridDim.y is limited to 65535
        const int32_t nb = rows - b0 > 32768 ? 32768 : rows - b0;
        const float *src = row0 + (ptrdiff_t)b0 * pitch;
        uint8_t *dst = rgb + (size_t)b0 * cols * 3;
        void *kargs[] = {&src, &pitch, const_cast<int32_t *>(&nb), &cols, &scale, &palette, &n, &dst};
        hipError_t e = hipLaunchKernel(reinterpret_cast<const void *>(&gs_colormap_k), dim3((unsigned)((cols + 255) / 256), (unsigned)nb),
                                       dim3(256), kargs, 0, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t gs_launch_pack_rows(const float *row0, int32_t pitch, int32_t rows, int32_t cols, float *dst, hipStream_t s)
{
    if (rows <= 0 || cols <= 0) return hipSuccess;
    const unsigned gy = (unsigned)(rows < 32768 ? rows : 32768);
    // 16 bytes per lane where the rows allow it (the planes' pitch is a multiple of 64 floats, hipMalloc aligns to 256 B)
    if (cols % 4 == 0 && pitch % 4 == 0 && (reinterpret_cast<uintptr_t>(row0) | reinterpret_cast<uintptr_t>(dst)) % 16 == 0) {
        const int ct = cols / 4;
        hipLaunchKernelGGL(gs_pack_rows_k<float4>, dim3((unsigned)((ct + 255) / 256), gy), dim3(256), 0, s, row0, pitch, rows, ct,
                           reinterpret_cast<float4 *>(dst));
    } else {
        hipLaunchKernelGGL(gs_pack_rows_k<float>, dim3((unsigned)((cols + 255) / 256), gy), dim3(256), 0, s, row0, pitch, rows, cols, dst);
    }
    return hipGetLastError();
}

hipError_t gs_launch_fill_rect(float *row0, int32_t pitch, int32_t r0, int32_t r1, int32_t c0,
                               int32_t c1, float value, hipStream_t s)
{
    if (r1 <= r0 || c1 <= c0) return hipSuccess;
    // gridDim.y is limited to 65535: walk tall rectangles in bands.
    for (int32_t b0 = r0; b0 < r1; b0 += 32768) {
        const int32_t b1 = (r1 - b0 > 32768) ? b0 + 32768 : r1;
        dim3 grid((unsigned)((c1 - c0 + 255) / 256), (unsigned)(b1 - b0));
        void *kargs[] = {&row0, &pitch, &b0, &c0, &c1, &value};
        hipError_t e = hipLaunchKernel(reinterpret_cast<const void *>(&gs_fill_rect_k), grid, dim3(256),
                                       kargs, 0, s);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Link words of a domain mask (gs_ctx_set_mask; the bits of gs_cell.h: link_bit): bit (i * 3 + j) when the cell at
// (r + i - 1, c + j - 1) is a wall, bit 9 when (r, c) is.  A wall is a mask value != 0.0f (NaN included, +-0 is fluid).
// A neighbour outside the slab's rows is its ghost row where a slab lies above / below (`top` / `bottom`); outside the
// grid it wraps under the periodic rule and is no wall under the others -- the clipped, zero-halo and zero-flux edge
// cells never read that position, or read one the word already covers (the zero-flux rule's clamped neighbour).
namespace {
__global__ __launch_bounds__(256) void gs_mask_links_k(const float *mask, uint32_t *link, int pitch, int rows, int cols,
                                                       int top, int bottom, int periodic)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= cols) return;
    for (int r = blockIdx.y; r < rows; r += gridDim.y) {
        uint32_t w = mask[(ptrdiff_t)r * pitch + c] != 0.0f ? 1u << 9 : 0u;
        for (int i = 0; i < 3; ++i) {
            int rr = r + i - 1;
            if (rr < 0 && !top) {
                if (!periodic) continue;
                rr += rows;
            }
            if (rr >= rows && !bottom) {
                if (!periodic) continue;
                rr -= rows;
            }
            for (int j = 0; j < 3; ++j) {
                if (i == 1 && j == 1) continue;
                int cc = c + j - 1;
                if (cc < 0 || cc >= cols) {
                    if (!periodic) continue;
                    cc = cc < 0 ? cc + cols : cc - cols;
                }
                if (mask[(ptrdiff_t)rr * pitch + cc] != 0.0f) w |= 1u << (i * 3 + j);
            }
        }
        link[(ptrdiff_t)r * pitch + c] = w;
    }
}
} // namespace

hipError_t gs_launch_mask_links(const float *mask, uint32_t *link, int32_t pitch, int32_t rows, int32_t cols, int32_t top,
                                int32_t bottom, int32_t periodic, hipStream_t s)
{
    if (rows <= 0 || cols <= 0) return hipSuccess;
    const dim3 grid((unsigned)((cols + 255) / 256), (unsigned)(rows < 65535 ? rows : 65535));
    void *kargs[] = {&mask, &link, &pitch, &rows, &cols, &top, &bottom, &periodic};
    return hipLaunchKernel(reinterpret_cast<const void *>(&gs_mask_links_k), grid, dim3(256), kargs, 0, s);
}
