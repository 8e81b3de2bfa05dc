// gs_components.hip -- connected components of thresholded planes on the device (include/gs_hip.h: gs_fields_components,
// gs_members_components): label equivalence with union-find (gs_unionfind.h) over a u32 parent array, one entry per cell of
// `planes` planes of rows x cols cells that lie one after the other -- cell (r, c) of plane y is entry (y * rows + r) * cols + c,
// fewer than 2^32 in all (the caller's check) -- and a u32 size array of the same length.  One (plane set, threshold) per
// call; four launches on one stream, each complete before the next begins:
//   tile     gs_comp_tile_k: a workgroup thresholds a tile of kCompTileRows x kCompTileCols cells (16 B per lane, as
//            gs_plane_quads_k reads) into LDS -- a set cell starts as the first cell of its horizontal run inside the tile,
//            found with two ballots, so that only vertical and diagonal unions remain --, unites inside LDS and writes
//            parent[cell] = the entry of the cell's root in the tile, the smallest entry of its component there; an unset
//            cell gets kUfUnset.  size[] is zeroed.  A component never leaves its plane: tiles do not straddle planes.
//   border   gs_comp_border_k: one thread per cell of a tile's first row (rows kCompTileRows, 2 kCompTileRows, ... of a plane)
//            unites it with the set cells above it -- straight up; up-left and up-right under 8-connectivity --, one per cell
//            of a tile's first column with those to its left -- left; up-left and down-left under 8.  Every pair of
//            neighbours in different tiles is met at least once.
//   flatten  gs_comp_flatten_k: every set cell finds its root, stores it and adds 1 to size[root] -- one atomic per run of
//            lanes with the same root.
//   tally    gs_comp_tally_k: every root adds itself to its plane's counters (gs_components' layout), collected per
//            workgroup in LDS first.  gs_comp_seam_k then copies (root, size of root) of a plane's first and last row out.
//
// No kernel waits for another wave or workgroup: no flags, no spinning, every phase its own launch.  TERMINATION: parent[i] <= i
// holds at all times -- the tile phase writes roots that are the smallest entry of their piece, a union only ever lowers an
// entry with an atomic minimum (to an index smaller than the entry's own), and flatten stores a root it reached by walking
// down.  So every find follows strictly decreasing indices and ends after at most i steps whatever runs beside it, and a
// union that lost its race retries from a strictly smaller root (gs_unionfind.h): its loop ends too.
//
// Built with hipcc's default float mode (f32 denormals kept), as gs_morphology.hip is: a sub-normal cell is compared as the
// value it is.
//
// The component lists (gs_component_list.hip) run the tile, border and flatten launches alone (gs_launch_component_labels) and
// continue from parent[] and size[] on the same stream.  The match of two planes (gs_match.hip) labels a third time: the cells
// set in both, read from the two label arrays (gs_launch_piece_labels: the tile kernel's BOTH form, then border and flatten as
// they are).
#include "gs_kernels.h"
#include "gs_plane_scan.h"

#define GS_UF_FN __device__ __forceinline__
#define GS_UF_LOAD(p) __atomic_load_n((p), __ATOMIC_RELAXED)
#define GS_UF_MIN(p, v) atomicMin((p), (v))
#include "gs_unionfind.h"

namespace {

constexpr int kRows = kCompTileRows, kCols = kCompTileCols; // a tile: 4 waves x 4 rows, 64 lanes x 4 columns
static_assert(kCols == 256 && kRows % 4 == 0, "a lane holds four columns of a 256-column tile row");
constexpr int kCounters = 35; // gs_components in u64 words: components, set_cells, largest, by_size[32]

struct GsCompArgs {
    union {
        const float *p; // plane y at p + y * stride (no GsPlaneSet: it costs gs_comp_tile_k two waits, profiles/plane_scan_refactor.md)
        const uint32_t *both_b; // gs_comp_tile_k's BOTH form reads two label arrays in place of the plane, t and flip: the first
    };
    int64_t stride, pitch, rows, planes;
    int32_t cols;
    float t;          // the threshold and ...
    uint32_t flip;    // ... the sign flip of gs_is_set
    int32_t eight;    // 8-connectivity
    uint32_t *parent, *size;
    union {
        unsigned long long *out; // [planes][kCounters], zeroed by the caller (the tally alone)
        const uint32_t *both_a;  // the BOTH form's second label array: the pieces are never tallied, and the struct keeps its size
    };
};

// BOTH: the source is not a plane but two label arrays of the same dense layout as parent[] -- a cell is set where both hold
// a label (gs_match.hip: the pieces that two planes' components share).
template <bool VEC, bool BOTH = false>
__global__ __launch_bounds__(256) void gs_comp_tile_k(GsCompArgs a)
{
    __shared__ uint32_t lab[kRows * kCols];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int cols = a.cols;
    const int64_t rows = a.rows;
    const int64_t tiles_c = ((int64_t)cols + kCols - 1) / kCols, tiles_r = (rows + kRows - 1) / kRows;
    const int64_t per_plane = tiles_c * tiles_r;
    const int64_t y = (int64_t)blockIdx.x / per_plane, tile = (int64_t)blockIdx.x % per_plane;
    const int64_t r0 = (tile / tiles_c) * kRows;
    const int c0 = (int)(tile % tiles_c) * kCols, c = c0 + 4 * lane;
    const float *plane = a.p + y * a.stride;
    const unsigned own = (c < cols ? 1u : 0u) | (c + 1 < cols ? 2u : 0u) | (c + 2 < cols ? 4u : 0u) | (c + 3 < cols ? 8u : 0u);
    const GsLaneColumns at = gs_lane_columns(c, cols);

    // threshold: the lane's four cells of rows wave, wave + 4, ... of the tile; a set cell starts as its run's first cell
#pragma unroll
    for (int i = 0; i < kRows / 4; ++i) {
        const int lr = wave + 4 * i;
        const int64_t r = r0 + lr;
        const float *row = plane + (r < rows ? r : rows - 1) * a.pitch; // (an address that exists; masked below)
        unsigned m;
        if constexpr (BOTH) {
            const uint64_t e = ((uint64_t)y * (uint64_t)rows + (uint64_t)(r < rows ? r : rows - 1)) * (uint64_t)cols + (uint64_t)c;
            m = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k) // (own: an entry past the row's end belongs to the next row, or to nobody)
                if (((own >> k) & 1u) && a.both_b[e + k] != kUfUnset && a.both_a[e + k] != kUfUnset) m |= 1u << k;
        } else {
            const float4 x = gs_load_columns<VEC>(row, at);
            m = (gs_is_set(x.x, a.flip, a.t) ? 1u : 0u) | (gs_is_set(x.y, a.flip, a.t) ? 2u : 0u) |
                (gs_is_set(x.z, a.flip, a.t) ? 4u : 0u) | (gs_is_set(x.w, a.flip, a.t) ? 8u : 0u);
        }
        m &= r < rows ? own : 0u;
        // the run that reaches the lane's column 0 from the left: the lanes below this one that are full (all four set) up
        // to lane j, the nearest that is not; it begins in lane j if that one's column 3 is set, else in lane j + 1
        const unsigned long long full = __ballot(m == 15u);
        const unsigned long long below = ~full & ((1ull << lane) - 1ull);
        const int j = below ? 63 - __clzll((long long)below) : -1;
        const unsigned mj = (unsigned)__shfl((int)m, j < 0 ? 0 : j);
        int start = 4 * (j + 1); // the run's first column inside the tile ...
        if (j >= 0 && (mj & 8u)) start = 4 * j + ((mj & 4u) ? ((mj & 2u) ? 1 : 2) : 3); // (mj != 15: the run ends inside lane j)
        const uint32_t base = (uint32_t)(lr * kCols);
        uint32_t run = (m & 1u) ? base + (uint32_t)start : 0u;
        uint32_t *dst = lab + base + 4 * lane;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool set = (m >> k) & 1u;
            if (set && k > 0 && !((m >> (k - 1)) & 1u)) run = base + (uint32_t)(4 * lane + k); // a run begins here
            dst[k] = set ? run : kUfUnset;
        }
    }
    __syncthreads();

    // unions inside the tile: a cell joins the run above it -- where its left neighbour has not already done the same
#pragma unroll
    for (int i = 0; i < kRows / 4; ++i) {
        const int lr = wave + 4 * i;
        if (lr == 0) continue;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lc = 4 * lane + k;
            const uint32_t me = (uint32_t)(lr * kCols + lc);
            if (lab[me] == kUfUnset) continue;
            const bool left = lc > 0 && lab[me - 1] != kUfUnset;
            const bool up = lab[me - kCols] != kUfUnset;
            const bool upleft = lc > 0 && lab[me - kCols - 1] != kUfUnset;
            const bool upright = lc + 1 < kCols && lab[me - kCols + 1] != kUfUnset;
            if (up) {
                if (!(left && upleft)) gs_uf_unite(lab, me, me - kCols);
            } else if (a.eight) {
                if (upleft && !left) gs_uf_unite(lab, me, me - kCols - 1);
                if (upright) gs_uf_unite(lab, me, me - kCols + 1);
            }
        }
    }
    __syncthreads();

    // the root inside the tile, as an entry of the parent array
    const uint64_t plane_at = (uint64_t)y * (uint64_t)rows * (uint64_t)cols;
#pragma unroll
    for (int i = 0; i < kRows / 4; ++i) {
        const int lr = wave + 4 * i;
        const int64_t r = r0 + lr;
        if (r >= rows) continue;
        const uint64_t at = plane_at + (uint64_t)r * (uint64_t)cols + (uint64_t)c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c + k >= cols) continue;
            const uint32_t me = (uint32_t)(lr * kCols + 4 * lane + k);
            uint32_t v = kUfUnset;
            if (lab[me] != kUfUnset) {
                const uint32_t root = gs_uf_find(lab, me);
                const int rr = (int)(root / kCols), rc = (int)(root % kCols);
                v = (uint32_t)(plane_at + (uint64_t)(r0 + rr) * (uint64_t)cols + (uint64_t)(c0 + rc));
            }
            a.parent[at + k] = v;
            a.size[at + k] = 0u;
        }
    }
}

// Thread t of plane y: t < hs * cols: a cell of a tile's first row; then vs * rows cells of tiles' first columns.
__global__ __launch_bounds__(256) void gs_comp_border_k(GsCompArgs a, int64_t per_plane, int64_t total)
{
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (g >= total) return;
    const int64_t y = g / per_plane, t = g % per_plane;
    const int64_t rows = a.rows, cols = a.cols;
    const int64_t hs = (rows - 1) / kRows;
    uint32_t *parent = a.parent;
    const uint64_t plane_at = (uint64_t)y * (uint64_t)rows * (uint64_t)cols;
    auto at = [&](int64_t r, int64_t c) -> uint32_t { return (uint32_t)(plane_at + (uint64_t)r * (uint64_t)cols + (uint64_t)c); };
    auto join = [&](uint32_t me, int64_t r, int64_t c) {
        if (r < 0 || r >= rows || c < 0 || c >= cols) return;
        const uint32_t o = at(r, c);
        if (GS_UF_LOAD(parent + o) != kUfUnset) gs_uf_unite(parent, me, o);
    };
    if (t < hs * cols) {
        const int64_t r = (t / cols + 1) * kRows, c = t % cols;
        const uint32_t me = at(r, c);
        if (GS_UF_LOAD(parent + me) == kUfUnset) return;
        join(me, r - 1, c);
        if (a.eight) {
            join(me, r - 1, c - 1);
            join(me, r - 1, c + 1);
        }
    } else {
        const int64_t u = t - hs * cols;
        const int64_t c = (u / rows + 1) * kCols, r = u % rows;
        const uint32_t me = at(r, c);
        if (GS_UF_LOAD(parent + me) == kUfUnset) return;
        join(me, r, c - 1);
        if (a.eight) {
            join(me, r - 1, c - 1);
            join(me, r + 1, c - 1);
        }
    }
}

// One thread per entry (whole waves: `total` is rounded up by the grid; entries beyond it count as unset).
__global__ __launch_bounds__(256) void gs_comp_flatten_k(GsCompArgs a, uint64_t total)
{
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    uint32_t root = kUfUnset;
    if (i < total && GS_UF_LOAD(a.parent + i) != kUfUnset) {
        root = gs_uf_find(a.parent, (uint32_t)i);
        a.parent[i] = root;
    }
    // runs of lanes with one root: the run's first lane adds its length
    const uint32_t prev = (uint32_t)__shfl_up((int)root, 1);
    const bool head = lane == 0 || prev != root;
    const unsigned long long heads = __ballot(head);
    if (head && root != kUfUnset) {
        const unsigned long long next = lane == 63 ? 0ull : (heads & (~0ull << (lane + 1)));
        const int len = (next ? __ffsll((long long)next) - 1 : 64) - lane;
        atomicAdd(a.size + root, (uint32_t)len);
    }
}

// 1-D grid of planes x groups workgroups; a workgroup takes every groups-th stretch of 256 entries of its plane.
__global__ __launch_bounds__(256) void gs_comp_tally_k(GsCompArgs a, int64_t groups)
{
    __shared__ unsigned bins[32];
    __shared__ unsigned n, largest;
    __shared__ unsigned long long cells;
    const int64_t y = (int64_t)blockIdx.x / groups, g = (int64_t)blockIdx.x % groups;
    if (threadIdx.x < 32) bins[threadIdx.x] = 0u;
    if (threadIdx.x == 32) n = 0u, largest = 0u, cells = 0ull;
    __syncthreads();
    const uint64_t plane_cells = (uint64_t)a.rows * (uint64_t)a.cols, plane_at = (uint64_t)y * plane_cells;
    for (uint64_t j = (uint64_t)g * 256 + threadIdx.x; j < plane_cells; j += (uint64_t)groups * 256) {
        const uint64_t i = plane_at + j;
        if (a.parent[i] != (uint32_t)i) continue;
        const uint32_t s = a.size[i];
        atomicAdd(&n, 1u);
        atomicAdd(&cells, (unsigned long long)s);
        atomicMax(&largest, s);
        atomicAdd(&bins[31 - __clz((int)s)], 1u); // (s >= 1: a root counts itself)
    }
    __syncthreads();
    unsigned long long *out = a.out + y * kCounters;
    if (threadIdx.x < 32 && bins[threadIdx.x]) atomicAdd(out + 3 + threadIdx.x, (unsigned long long)bins[threadIdx.x]);
    if (threadIdx.x == 32 && n) {
        atomicAdd(out + 0, (unsigned long long)n);
        atomicAdd(out + 1, cells);
        atomicMax(out + 2, (unsigned long long)largest);
    }
}

// seams[0 .. 4 cols): the first row's roots, the sizes of those roots, the last row's roots, their sizes (plane 0).
__global__ __launch_bounds__(256) void gs_comp_seam_k(GsCompArgs a, uint32_t *seams)
{
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= a.cols) return;
    const uint64_t first = (uint64_t)c, lastrow = (uint64_t)(a.rows - 1) * (uint64_t)a.cols + (uint64_t)c;
    const uint32_t r0 = a.parent[first], r1 = a.parent[lastrow];
    seams[c] = r0;
    seams[(int64_t)a.cols + c] = r0 == kUfUnset ? 0u : a.size[r0];
    seams[2 * (int64_t)a.cols + c] = r1;
    seams[3 * (int64_t)a.cols + c] = r1 == kUfUnset ? 0u : a.size[r1];
}

} // namespace

// The tile, border and flatten launches: on return (of the launches) parent[cell] is the root of the cell's component, its
// first cell in row-major order (kUfUnset: the cell is not set), and size[root] the component's cells.
static hipError_t launch_labels(GsCompArgs &a, const float *plane, int64_t planes, int64_t stride, int64_t pitch, int64_t rows,
                                int32_t cols, float threshold, int32_t sense, int32_t connectivity, uint32_t *parent,
                                uint32_t *size, hipStream_t s, const uint32_t *both_b = nullptr, const uint32_t *both_a = nullptr)
{
    const uint64_t total = (uint64_t)planes * (uint64_t)rows * (uint64_t)cols;
    if (total >= (1ull << 32)) return hipErrorInvalidValue;
    a = GsCompArgs{};
    a.p = plane;
    a.stride = stride;
    a.pitch = pitch;
    a.rows = rows;
    a.planes = planes;
    a.cols = cols;
    const bool vec = !both_b && gs_reads_16_bytes(&plane, 1, planes, stride, pitch);
    gs_set_rule(threshold, sense, a.t, a.flip);
    a.eight = connectivity == 8 ? 1 : 0;
    a.parent = parent;
    a.size = size;
    if (both_b) a.both_b = both_b, a.both_a = both_a;

    const int64_t tiles = (((int64_t)cols + kCols - 1) / kCols) * ((rows + kRows - 1) / kRows) * planes;
    if (tiles > INT32_MAX) return hipErrorInvalidValue;
    if (both_b)
        hipLaunchKernelGGL((gs_comp_tile_k<false, true>), dim3((unsigned)tiles), dim3(256), 0, s, a);
    else if (vec)
        hipLaunchKernelGGL((gs_comp_tile_k<true>), dim3((unsigned)tiles), dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL((gs_comp_tile_k<false>), dim3((unsigned)tiles), dim3(256), 0, s, a);

    const int64_t per_plane = ((rows - 1) / kRows) * (int64_t)cols + (((int64_t)cols - 1) / kCols) * rows;
    const int64_t border = per_plane * planes;
    if (border > 0)
        hipLaunchKernelGGL(gs_comp_border_k, dim3((unsigned)((border + 255) / 256)), dim3(256), 0, s, a, per_plane, border);

    hipLaunchKernelGGL(gs_comp_flatten_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, total);
    return hipSuccess;
}

hipError_t gs_launch_component_labels(const float *plane, int64_t planes, int64_t stride, int64_t pitch, int64_t rows, int32_t cols,
                                      float threshold, int32_t sense, int32_t connectivity, uint32_t *parent, uint32_t *size,
                                      hipStream_t s)
{
    if (planes < 1 || (connectivity != 4 && connectivity != 8)) return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    GsCompArgs a;
    const hipError_t e = launch_labels(a, plane, planes, stride, pitch, rows, cols, threshold, sense, connectivity, parent, size, s);
    return e != hipSuccess ? e : hipGetLastError();
}

// The flatten launch alone, behind a labelling of another lattice of walls (gs_region_components.hip).
hipError_t gs_launch_component_flatten(uint32_t *parent, uint32_t *size, uint64_t total, hipStream_t s)
{
    if (total == 0) return hipSuccess;
    if (total >= (1ull << 32)) return hipErrorInvalidValue;
    GsCompArgs a{};
    a.parent = parent;
    a.size = size;
    hipLaunchKernelGGL(gs_comp_flatten_k, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, total);
    return hipGetLastError();
}

hipError_t gs_launch_piece_labels(const uint32_t *both_b, const uint32_t *both_a, int64_t planes, int64_t rows, int32_t cols,
                                  int32_t connectivity, uint32_t *parent, uint32_t *size, hipStream_t s)
{
    if (planes < 1 || (connectivity != 4 && connectivity != 8) || !both_b || !both_a) return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    GsCompArgs a;
    const hipError_t e = launch_labels(a, nullptr, planes, 0, 0, rows, cols, 0.0f, 1, connectivity, parent, size, s, both_b, both_a);
    return e != hipSuccess ? e : hipGetLastError();
}

hipError_t gs_launch_components(const float *plane, int64_t planes, int64_t stride, int64_t pitch, int64_t rows, int32_t cols,
                                float threshold, int32_t sense, int32_t connectivity, int64_t max_groups, uint32_t *parent,
                                uint32_t *size, unsigned long long *out, uint32_t *seams, hipStream_t s)
{
    if (planes < 1 || (connectivity != 4 && connectivity != 8) || (seams && planes != 1)) return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    GsCompArgs a;
    const hipError_t e = launch_labels(a, plane, planes, stride, pitch, rows, cols, threshold, sense, connectivity, parent, size, s);
    if (e != hipSuccess) return e;
    a.out = out;

    // As many workgroups per plane as it has stretches of 256 entries, at most the caller's share, and no floor: there are fewer
    // than 2^32 entries.  gs_scan_groups divides its units by 4, and ceil(ceil(n / 64) / 4) = ceil(n / 256).
    int64_t groups;
    if (!gs_scan_groups((int64_t)(((uint64_t)rows * (uint64_t)cols + 63) / 64), 0, max_groups, planes, groups))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(gs_comp_tally_k, dim3((unsigned)(groups * planes)), dim3(256), 0, s, a, groups);

    if (seams) hipLaunchKernelGGL(gs_comp_seam_k, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, s, a, seams);
    return hipGetLastError();
}
