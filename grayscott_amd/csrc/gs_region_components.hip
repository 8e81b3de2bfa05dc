// gs_region_components.hip -- connected components of every region of rh x rw cells of a thresholded plane (include/gs_hip.h:
// gs_fields_region_components): the labelling of gs_components.hip on the same tile lattice and the same dense u32 entries
// r * cols + c of one slab, with the regions' borders as walls -- two set cells in different regions are never neighbours,
// neither across a side nor across a corner --, and a tally per region.  One (plane, threshold) per call; four launches on
// one stream, each complete before the next begins:
//   tile     gs_region_comp_tile_k: gs_comp_tile_k with walls.  rw is a multiple of 4, so a lane's four columns lie in one
//            region; the run that reaches a lane's column 0 from the left stops at the nearest lane whose first column is a
//            multiple of rw (a second ballot beside that of the full lanes).  A cell of a row that is a multiple of rh unites
//            with nothing above it, a cell of a column that is a multiple of rw has no left and no up-left neighbour, and a
//            cell left of such a column has no up-right neighbour.
//   border   gs_region_comp_border_k: gs_comp_border_k with the same unions skipped.
//   flatten  gs_comp_flatten_k as it is (gs_launch_component_flatten).
//   tally    gs_region_comp_tally_k: every root adds itself to the 35 counters of the region it lies in -- a component lies in
//            one region, so its root does.  A workgroup walks consecutive stretches of 256 entries; while they lie in one
//            region it collects in LDS and flushes when the region changes, a stretch that meets several regions adds its
//            roots to the regions' counters one by one.
// Rows are the slab's own: a slab begins at a multiple of rh rows (band_results' refusal otherwise), so they decide the walls
// as global rows would.  No kernel waits for another wave or workgroup, and parent[i] <= i holds at all times exactly as in
// gs_components.hip: the walls only take unions away.  Roots stay the smallest entry of their component.
//
// Built with hipcc's default float mode (f32 denormals kept), as gs_components.hip is.
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

struct GsRegionCompArgs {
    const float *p;
    int64_t pitch, rows;
    int32_t cols;
    int32_t rh, rw;   // the region shape: rh >= 1, rw a multiple of 4
    float t;          // the threshold and ...
    uint32_t flip;    // ... the sign flip of gs_is_set
    int32_t eight;    // 8-connectivity
    uint32_t *parent, *size;
};

// 16 bytes per lane and row, as gs_comp_tile_k's VEC form reads: a field's rows begin on 16 bytes and are a multiple of 4 floats
// apart (plane_layout), and only fields have regions -- there is no form for other planes, the launcher refuses them.
__global__ __launch_bounds__(256) void gs_region_comp_tile_k(GsRegionCompArgs a)
{
    __shared__ uint32_t lab[kRows * kCols];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int cols = a.cols, rh = a.rh, rw = a.rw;
    const int64_t rows = a.rows;
    const int64_t tiles_c = ((int64_t)cols + kCols - 1) / kCols;
    const int64_t tile = (int64_t)blockIdx.x;
    const int64_t r0 = (tile / tiles_c) * kRows;
    const int c0 = (int)(tile % tiles_c) * kCols, c = c0 + 4 * lane;
    const unsigned own = (c < cols ? 1u : 0u) | (c + 1 < cols ? 2u : 0u) | (c + 2 < cols ? 4u : 0u) | (c + 3 < cols ? 8u : 0u);
    const GsLaneColumns at = gs_lane_columns(c, cols);
    // the lanes at or below this one whose first column begins a region: no run passes the nearest of them
    const unsigned long long walls = __ballot(c % rw == 0) & ((2ull << lane) - 1ull);
    const int w = walls ? 63 - __clzll((long long)walls) : -1;

    // threshold: the lane's four cells of rows wave, wave + 4, ... of the tile; a set cell starts as its run's first cell
#pragma unroll
    for (int i = 0; i < kRows / 4; ++i) {
        const int lr = wave + 4 * i;
        const int64_t r = r0 + lr;
        const float *row = a.p + (r < rows ? r : rows - 1) * a.pitch; // (an address that exists; masked below)
        const float4 x = gs_load_columns<true>(row, at);
        unsigned m = (gs_is_set(x.x, a.flip, a.t) ? 1u : 0u) | (gs_is_set(x.y, a.flip, a.t) ? 2u : 0u) |
                     (gs_is_set(x.z, a.flip, a.t) ? 4u : 0u) | (gs_is_set(x.w, a.flip, a.t) ? 8u : 0u);
        m &= r < rows ? own : 0u;
        // the run that reaches the lane's column 0 from the left, as in gs_comp_tile_k: through the full lanes below this one
        // down to lane j, the nearest that is not full -- but no further than lane w, whose first column begins the region
        const unsigned long long full = __ballot(m == 15u);
        const unsigned long long below = ~full & ((1ull << lane) - 1ull);
        const int j = below ? 63 - __clzll((long long)below) : -1;
        const unsigned mj = (unsigned)__shfl((int)m, j < 0 ? 0 : j);
        int start = 4 * (j + 1);
        if (j >= 0 && (mj & 8u)) start = 4 * j + ((mj & 4u) ? ((mj & 2u) ? 1 : 2) : 3); // (mj != 15: the run ends inside lane j)
        if (w > j) start = 4 * w; // (w == lane: the cell has no left neighbour)
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

    // unions inside the tile: a cell joins the run above it -- where its left neighbour has not already done the same --, never
    // through a wall
#pragma unroll
    for (int i = 0; i < kRows / 4; ++i) {
        const int lr = wave + 4 * i;
        if (lr == 0 || (int)(r0 + lr) % rh == 0) continue; // (the region's first row: nothing above it)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int lc = 4 * lane + k;
            const uint32_t me = (uint32_t)(lr * kCols + lc);
            if (lab[me] == kUfUnset) continue;
            // k > 0: inside the lane's four columns, which lie in one region; k == 0: the lane's first column may begin one
            const bool open_left = lc > 0 && (k > 0 || w != lane);
            const bool open_right = lc + 1 < kCols && (k < 3 || (c + 4) % rw != 0);
            const bool left = open_left && lab[me - 1] != kUfUnset;
            const bool up = lab[me - kCols] != kUfUnset;
            const bool upleft = open_left && lab[me - kCols - 1] != kUfUnset;
            const bool upright = open_right && lab[me - kCols + 1] != kUfUnset;
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
#pragma unroll
    for (int i = 0; i < kRows / 4; ++i) {
        const int lr = wave + 4 * i;
        const int64_t r = r0 + lr;
        if (r >= rows) continue;
        const uint64_t e = (uint64_t)r * (uint64_t)cols + (uint64_t)c;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (c + k >= cols) continue;
            const uint32_t me = (uint32_t)(lr * kCols + 4 * lane + k);
            uint32_t v = kUfUnset;
            if (lab[me] != kUfUnset) {
                const uint32_t root = gs_uf_find(lab, me);
                const int rr = (int)(root / kCols), rc = (int)(root % kCols);
                v = (uint32_t)((uint64_t)(r0 + rr) * (uint64_t)cols + (uint64_t)(c0 + rc));
            }
            a.parent[e + k] = v;
            a.size[e + k] = 0u;
        }
    }
}

// Thread t: t < hs * cols: a cell of a tile's first row; then vs * rows cells of tiles' first columns.  Fewer than 2^32 cells,
// so fewer border cells: 32-bit arithmetic throughout.
__global__ __launch_bounds__(256) void gs_region_comp_border_k(GsRegionCompArgs a, uint32_t total)
{
    const uint32_t t = blockIdx.x * 256u + threadIdx.x;
    if (t >= total) return;
    const int32_t rows = (int32_t)a.rows, cols = a.cols, rh = a.rh, rw = a.rw;
    const uint32_t hs = (uint32_t)(rows - 1) / kRows;
    uint32_t *parent = a.parent;
    auto at = [&](int32_t r, int32_t c) -> uint32_t { return (uint32_t)r * (uint32_t)cols + (uint32_t)c; };
    auto join = [&](uint32_t me, int32_t r, int32_t c) {
        if (r < 0 || r >= rows || c < 0 || c >= cols) return;
        const uint32_t o = at(r, c);
        if (GS_UF_LOAD(parent + o) != kUfUnset) gs_uf_unite(parent, me, o);
    };
    if (t < hs * (uint32_t)cols) {
        const int32_t r = (int32_t)(t / (uint32_t)cols + 1u) * kRows, c = (int32_t)(t % (uint32_t)cols);
        if (r % rh == 0) return; // a wall above the whole row
        const uint32_t me = at(r, c);
        if (GS_UF_LOAD(parent + me) == kUfUnset) return;
        join(me, r - 1, c);
        if (a.eight) {
            if (c % rw != 0) join(me, r - 1, c - 1);
            if ((c + 1) % rw != 0) join(me, r - 1, c + 1);
        }
    } else {
        const uint32_t u = t - hs * (uint32_t)cols;
        const int32_t c = (int32_t)(u / (uint32_t)rows + 1u) * kCols, r = (int32_t)(u % (uint32_t)rows);
        if (c % rw == 0) return; // a wall left of the whole column
        const uint32_t me = at(r, c);
        if (GS_UF_LOAD(parent + me) == kUfUnset) return;
        join(me, r, c - 1);
        if (a.eight) {
            if (r % rh != 0) join(me, r - 1, c - 1);
            if ((r + 1) % rh != 0) join(me, r + 1, c - 1);
        }
    }
}

// Workgroup g takes the stretches [g * per_group, (g + 1) * per_group) of 256 entries each.  out: the counters of region
// (band i, column j) of the slab at out[(i * rc + j) * region_words ...], region_words u64 apart (nt results of 35 words
// lie side by side: the caller points at its threshold's).
__global__ __launch_bounds__(256) void gs_region_comp_tally_k(GsRegionCompArgs a, uint32_t total, uint32_t per_group, int32_t rc,
                                                              int64_t region_words, unsigned long long *out)
{
    __shared__ unsigned bins[32];
    __shared__ unsigned n, largest;
    __shared__ unsigned long long cells;
    if (threadIdx.x < 32) bins[threadIdx.x] = 0u;
    if (threadIdx.x == 32) n = 0u, largest = 0u, cells = 0ull;
    __syncthreads();
    const uint32_t cols = (uint32_t)a.cols, rh = (uint32_t)a.rh, rw = (uint32_t)a.rw; // (entries are 32-bit, and so is all here)
    auto region_of = [&](uint32_t e) -> int64_t { return (int64_t)((e / cols / rh) * (uint32_t)rc + (e % cols) / rw); };
    // what LDS holds goes to region `held`, and LDS is zero again (every thread calls this: it has barriers)
    auto flush = [&](int64_t held) {
        __syncthreads();
        unsigned long long *dst = out + held * region_words;
        if (threadIdx.x < 32 && bins[threadIdx.x]) {
            atomicAdd(dst + 3 + threadIdx.x, (unsigned long long)bins[threadIdx.x]);
            bins[threadIdx.x] = 0u;
        }
        if (threadIdx.x == 32 && n) {
            atomicAdd(dst + 0, (unsigned long long)n);
            atomicAdd(dst + 1, cells);
            atomicMax(dst + 2, (unsigned long long)largest);
            n = 0u, largest = 0u, cells = 0ull;
        }
        __syncthreads();
    };
    int64_t held = -1; // the region whose roots LDS holds
    const uint32_t stretches = (total - 1u) / 256u + 1u, first = blockIdx.x * per_group; // (the launcher: first < stretches)
    for (uint32_t st = first; st - first < per_group && st < stretches; ++st) {
        // the stretch's first and last entry: one region where they share a row and a region column, or -- the stretch runs
        // over whole rows then -- a band of a grid that is one region wide
        const uint32_t e0 = st * 256u, e1 = total - 1u - e0 > 255u ? e0 + 255u : total - 1u;
        const uint32_t ra = e0 / cols, rb = e1 / cols;
        const bool one = ra / rh == rb / rh && (ra == rb ? (e0 % cols) / rw == (e1 % cols) / rw : rc == 1);
        const int64_t here = region_of(e0);
        if (one && held >= 0 && held != here) flush(held); // (the same verdict in every thread)
        if (one) held = here;
        if (threadIdx.x > e1 - e0) continue;
        const uint32_t i = e0 + threadIdx.x;
        if (a.parent[i] != i) continue;
        const uint32_t s = a.size[i];
        const int bin = 31 - __clz((int)s); // (s >= 1: a root counts itself)
        if (one) {
            atomicAdd(&n, 1u);
            atomicAdd(&cells, (unsigned long long)s);
            atomicMax(&largest, s);
            atomicAdd(&bins[bin], 1u);
        } else {
            unsigned long long *dst = out + region_of(i) * region_words;
            atomicAdd(dst + 0, 1ull);
            atomicAdd(dst + 1, (unsigned long long)s);
            atomicMax(dst + 2, (unsigned long long)s);
            atomicAdd(dst + 3 + bin, 1ull);
        }
    }
    if (held >= 0) flush(held);
}

} // namespace

hipError_t gs_launch_region_components(const float *plane, int64_t pitch, int64_t rows, int32_t cols, int32_t rh, int32_t rw,
                                       float threshold, int32_t sense, int32_t connectivity, int64_t max_groups,
                                       uint32_t *parent, uint32_t *size, int64_t region_words, unsigned long long *out,
                                       hipStream_t s)
{
    if ((connectivity != 4 && connectivity != 8) || rh < 1 || rw < 4 || rw % 4 != 0 || region_words < kCounters)
        return hipErrorInvalidValue;
    if (rows <= 0 || cols <= 0) return hipSuccess;
    const uint64_t total = (uint64_t)rows * (uint64_t)cols;
    if (total >= (1ull << 32)) return hipErrorInvalidValue;
    GsRegionCompArgs a{};
    a.p = plane;
    a.pitch = pitch;
    a.rows = rows;
    a.cols = cols;
    a.rh = rh;
    a.rw = rw;
    gs_set_rule(threshold, sense, a.t, a.flip);
    a.eight = connectivity == 8 ? 1 : 0;
    a.parent = parent;
    a.size = size;

    const int64_t tiles = (((int64_t)cols + kCols - 1) / kCols) * ((rows + kRows - 1) / kRows);
    if (tiles > INT32_MAX) return hipErrorInvalidValue;
    if (!gs_reads_16_bytes(&plane, 1, 1, 0, pitch)) return hipErrorInvalidValue; // (no field's plane)
    hipLaunchKernelGGL(gs_region_comp_tile_k, dim3((unsigned)tiles), dim3(256), 0, s, a);

    const int64_t border = ((rows - 1) / kRows) * (int64_t)cols + (((int64_t)cols - 1) / kCols) * rows;
    if (border > 0)
        hipLaunchKernelGGL(gs_region_comp_border_k, dim3((unsigned)((border + 255) / 256)), dim3(256), 0, s, a, (uint32_t)border);

    const hipError_t e = gs_launch_component_flatten(parent, size, total, s);
    if (e != hipSuccess) return e;

    // consecutive stretches per workgroup, so that LDS is flushed only where the region changes; as many workgroups as
    // gs_launch_components' tally has
    const int64_t stretches = (int64_t)((total + 255) / 256);
    int64_t groups;
    if (!gs_scan_groups((int64_t)((total + 63) / 64), 0, max_groups, 1, groups)) return hipErrorInvalidValue;
    const int64_t per_group = (stretches + groups - 1) / groups;
    groups = (stretches + per_group - 1) / per_group;
    const int32_t rc = (int32_t)(((int64_t)cols + rw - 1) / rw);
    hipLaunchKernelGGL(gs_region_comp_tally_k, dim3((unsigned)groups), dim3(256), 0, s, a, (uint32_t)total, (uint32_t)per_group, rc,
                       region_words, out);
    return hipGetLastError();
}
