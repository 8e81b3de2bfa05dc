// gs_component_list.hip -- one record per connected component (include/gs_hip.h: gs_field_component_list,
// gs_members_component_list), formed behind the labelling of gs_components.hip on the same stream.  After its flatten launch
// parent[cell] is the root of the cell's component -- parent[i] <= i throughout, so a root IS its component's first cell in
// row-major order -- and size[root] the component's cells.  Entries are dense: cell (r, c) of plane y is entry
// i = (y * rows + r) * cols + c, fewer than 2^32 in all.  Six launches, each complete before the next begins:
//   open    gs_list_open_k (slab chains only): the roots of the components that touch the plane's first or last row are
//           marked in a bitmap of one bit per entry -- they are listed whatever their size, because min_size can only be
//           applied after the seam merge (gs_components_merge.h).
//   count   gs_list_count_k: a root is SELECTED if size >= min_size or it is marked; every workgroup of 256 entries leaves the
//           number it selects.
//   scan    gs_list_scan_k: ONE workgroup turns the counts into their exclusive prefix sums and leaves the total, which the
//           host reads once to size the record memory exactly.
//   write   gs_list_write_k: a selected root gets the dense index prefix + its rank inside the workgroup -- the records are in
//           ascending order of their first cell, with no sort -- and its record: the size copied, the sums zero, an empty box,
//           the first cell from the root.  size[root] becomes the dense index (kUfUnset for a root that is not selected):
//           every thread reads and writes its own entry alone.
//   gather  gs_list_gather_k: a wave walks kChunks x 64 consecutive entries.  Lanes that follow one another with one dense
//           index form a run, which may continue from chunk to chunk; a run is a RANGE of entries [a, b], so the sums of its
//           cells' rows and columns and its box have closed forms -- whether or not the range crosses row ends -- and the
//           run's last lane adds them to the record: one set of integer atomics per run, one per 1024 cells where a
//           component fills the span (profiles/component_list.md).  A minimum or maximum that a plain load shows to be no
//           news is not sent: the box only ever grows, so a stale load errs to the safe side.
//   seam    gs_list_seam_k (slab chains only): the dense indices of the first and the last row's cells.
//
// No kernel waits for another wave or workgroup: no flags, no spinning, no look-back; every dependency is a launch boundary (the
// scan's barriers are those of its one workgroup).  TERMINATION: every loop here has a trip count fixed by the launch
// (kChunks; the scan's share of the counts); nothing follows parent[] further than one step, because flatten left roots.
// Integer atomics only: the result does not depend on the order of arrival.
//
// Built with hipcc's default float mode, as gs_components.hip is (nothing here touches a float).
#include "gs_kernels.h"
#include "gs_unionfind.h" // kUfUnset

namespace {

#ifndef GS_LIST_CHUNKS
#define GS_LIST_CHUNKS 16 // (1: a run never continues past 64 entries -- the form it was measured against, profiles/component_list.md)
#endif
constexpr int kChunks = GS_LIST_CHUNKS; // chunks of 64 entries a wave of the gather walks

struct GsListArgs {
    const uint32_t *parent;
    uint32_t *size;       // sizes; from the write launch on: dense indices
    const uint32_t *open; // one bit per entry, or null: no component is open
    uint32_t *counts;     // one per workgroup of 256 entries
    uint32_t *selected;   // the total
    GsComponentRecord *records;
    uint64_t min_size;
    uint32_t total, rows, cols; // entries; rows of a plane; columns
};

__device__ __forceinline__ bool gs_list_selects(const GsListArgs &a, uint32_t i)
{
    if (a.parent[i] != i) return false;
    if ((uint64_t)a.size[i] >= a.min_size) return true;
    return a.open && ((a.open[i >> 5] >> (i & 31u)) & 1u);
}

// The roots of plane 0's first and last row, marked.
__global__ __launch_bounds__(256) void gs_list_open_k(const uint32_t *parent, uint32_t *open, uint32_t rows, uint32_t cols)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= cols) return;
    const uint32_t r0 = parent[c], r1 = parent[(rows - 1u) * cols + c];
    if (r0 != kUfUnset) atomicOr(open + (r0 >> 5), 1u << (r0 & 31u));
    if (r1 != kUfUnset) atomicOr(open + (r1 >> 5), 1u << (r1 & 31u));
}

__global__ __launch_bounds__(256) void gs_list_count_k(GsListArgs a)
{
    __shared__ uint32_t n[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x; // (fewer than 2^32 entries: the grid's last workgroup cannot wrap)
    const bool sel = i < a.total && gs_list_selects(a, i);
    const unsigned long long mine = __ballot(sel);
    if ((threadIdx.x & 63u) == 0u) n[threadIdx.x >> 6] = (uint32_t)__popcll(mine);
    __syncthreads();
    if (threadIdx.x == 0u) a.counts[blockIdx.x] = n[0] + n[1] + n[2] + n[3];
}

// One workgroup: thread t owns counts [t * share, (t + 1) * share).
__global__ __launch_bounds__(1024) void gs_list_scan_k(uint32_t *counts, uint32_t groups, uint32_t *selected)
{
    __shared__ uint32_t part[1024];
    const uint32_t t = threadIdx.x, share = (groups + 1023u) / 1024u;
    const uint64_t lo64 = (uint64_t)t * share;
    const uint32_t lo = lo64 < groups ? (uint32_t)lo64 : groups, hi = groups - lo < share ? groups : lo + share;
    uint32_t sum = 0u;
    for (uint32_t j = lo; j < hi; ++j) sum += counts[j];
    part[t] = sum;
    __syncthreads();
    for (uint32_t d = 1u; d < 1024u; d <<= 1) {
        const uint32_t below = t >= d ? part[t - d] : 0u;
        __syncthreads();
        part[t] += below;
        __syncthreads();
    }
    uint32_t at = part[t] - sum;
    for (uint32_t j = lo; j < hi; ++j) {
        const uint32_t c = counts[j];
        counts[j] = at;
        at += c;
    }
    if (t == 1023u) *selected = part[1023];
}

__global__ __launch_bounds__(256) void gs_list_write_k(GsListArgs a)
{
    __shared__ uint32_t n[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool root = i < a.total && a.parent[i] == i;
    const bool sel = root && gs_list_selects(a, i);
    const unsigned long long mine = __ballot(sel);
    if (lane == 0u) n[wave] = (uint32_t)__popcll(mine);
    __syncthreads();
    if (!root) return;
    uint32_t slot = kUfUnset;
    if (sel) {
        slot = a.counts[blockIdx.x] + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
        for (uint32_t w = 0u; w < wave; ++w) slot += n[w];
        GsComponentRecord rec;
        rec.size = a.size[i];
        rec.sum_row = 0ull;
        rec.sum_col = 0ull;
        rec.first_row = i / a.cols; // (counted over all planes: the host takes the plane from it)
        rec.first_col = i % a.cols;
        rec.row_min = 0xffffffffu;
        rec.row_max = 0u;
        rec.col_min = 0xffffffffu;
        rec.col_max = 0u;
        a.records[slot] = rec;
    }
    a.size[i] = slot;
}

// Entries [first, last] of one plane, all of the component of record `rec`, added to it.
__device__ __forceinline__ void gs_list_add_range(GsComponentRecord *rec, uint32_t first, uint32_t last, uint32_t rows, uint32_t cols)
{
    const uint32_t j = first % (rows * cols); // (rows * cols <= total < 2^32)
    const uint32_t ra = j / cols, ca = j % cols;
    const uint32_t n = last - first + 1u;
    const uint32_t end = ca + (n - 1u); // (< 2^32: ca < cols and the range stays inside its plane)
    const uint32_t rb = ra + end / cols, cb = end % cols;
    uint64_t sum_r, sum_c;
    uint32_t cmin, cmax;
    if (ra == rb) {
        sum_r = (uint64_t)ra * n;
        sum_c = ((uint64_t)ca + cb) * n / 2u;
        cmin = ca;
        cmax = cb;
    } else { // columns ca .. cols - 1 of row ra, `full` whole rows, columns 0 .. cb of row rb
        const uint64_t n0 = cols - ca, n1 = (uint64_t)cb + 1u, full = rb - ra - 1u;
        sum_r = ra * n0 + rb * n1 + (uint64_t)cols * (((uint64_t)ra + rb) * full / 2u);
        sum_c = ((uint64_t)ca + cols - 1u) * n0 / 2u + (uint64_t)cb * n1 / 2u + full * ((uint64_t)cols * (cols - 1u) / 2u);
        cmin = 0u;
        cmax = cols - 1u;
    }
    atomicAdd(reinterpret_cast<unsigned long long *>(&rec->sum_row), (unsigned long long)sum_r);
    atomicAdd(reinterpret_cast<unsigned long long *>(&rec->sum_col), (unsigned long long)sum_c);
    if (__atomic_load_n(&rec->row_min, __ATOMIC_RELAXED) > ra) atomicMin(&rec->row_min, ra);
    if (__atomic_load_n(&rec->row_max, __ATOMIC_RELAXED) < rb) atomicMax(&rec->row_max, rb);
    if (__atomic_load_n(&rec->col_min, __ATOMIC_RELAXED) > cmin) atomicMin(&rec->col_min, cmin);
    if (__atomic_load_n(&rec->col_max, __ATOMIC_RELAXED) < cmax) atomicMax(&rec->col_max, cmax);
}

__global__ __launch_bounds__(256) void gs_list_gather_k(GsListArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t span = ((uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6)) * (uint64_t)(64 * kChunks);
    // the dense index of an entry's component: kUfUnset for an unset cell, a component that is not listed, or no entry
    auto index_of = [&](uint64_t i) -> uint32_t {
        if (i >= a.total) return kUfUnset;
        const uint32_t root = a.parent[i];
        return root == kUfUnset ? kUfUnset : a.size[root];
    };
    bool carried = false;     // the run of the last chunk's lane 63 goes on in this chunk's lane 0 ...
    uint32_t carried_at = 0u; // ... and began at this entry (both the same in every lane)
#pragma unroll 1
    for (int k = 0; k < kChunks; ++k) {
        const uint64_t chunk = span + (uint64_t)(64 * k);
        if (chunk >= a.total) break; // (the same in every lane)
        const uint64_t i = chunk + lane;
        const uint32_t idx = index_of(i);
        const uint32_t prev = (uint32_t)__shfl_up((int)idx, 1);
        uint32_t next = (uint32_t)__shfl_down((int)idx, 1);
        bool tail = next != idx;
        if (lane == 63u) { // the run goes on in the wave's next chunk if that begins with the same index
            next = k + 1 < kChunks ? index_of(i + 1u) : kUfUnset;
            tail = k + 1 == kChunks || next != idx;
        }
        const bool head = lane == 0u ? !carried : prev != idx;
        const unsigned long long heads = __ballot(head);
        const unsigned long long upto = heads & ((2ull << lane) - 1ull); // the heads at or below this lane
        const uint32_t first = upto ? (uint32_t)chunk + (uint32_t)(63 - __clzll((long long)upto)) : carried_at;
        if (tail && idx != kUfUnset) gs_list_add_range(a.records + idx, first, (uint32_t)i, a.rows, a.cols);
        const bool goes_on = __shfl((int)(tail ? 0 : 1), 63) != 0;
        if (goes_on && heads) carried_at = (uint32_t)chunk + (uint32_t)(63 - __clzll((long long)heads));
        carried = goes_on;
    }
}

// seams[0 .. 2 cols): the dense indices of the first row's cells, then the last row's (plane 0); kUfUnset for an unset cell.
__global__ __launch_bounds__(256) void gs_list_seam_k(const uint32_t *parent, const uint32_t *index, uint32_t rows, uint32_t cols,
                                                      uint32_t *seams)
{
    const uint32_t c = blockIdx.x * 256u + threadIdx.x;
    if (c >= cols) return;
    const uint32_t r0 = parent[c], r1 = parent[(rows - 1u) * cols + c];
    seams[c] = r0 == kUfUnset ? kUfUnset : index[r0];
    seams[cols + c] = r1 == kUfUnset ? kUfUnset : index[r1];
}

bool list_shape(int64_t planes, int64_t rows, int32_t cols, uint32_t &total)
{
    if (planes < 1 || rows < 1 || cols < 1) return false;
    const uint64_t n = (uint64_t)planes * (uint64_t)rows * (uint64_t)cols;
    if (n >= (1ull << 32)) return false;
    total = (uint32_t)n;
    return true;
}

GsListArgs list_args(const GsListWork &w, const uint32_t *parent, uint32_t *size, uint32_t total, int64_t rows, int32_t cols,
                     uint64_t min_size)
{
    GsListArgs a{};
    a.parent = parent;
    a.size = size;
    a.open = w.open;
    a.counts = w.counts;
    a.selected = w.selected;
    a.min_size = min_size;
    a.total = total;
    a.rows = (uint32_t)rows;
    a.cols = (uint32_t)cols;
    return a;
}

} // namespace

uint64_t gs_list_groups(uint64_t entries) { return (entries + 255u) / 256u; }

hipError_t gs_launch_list_count(const uint32_t *parent, uint32_t *size, int64_t planes, int64_t rows, int32_t cols, uint64_t min_size,
                                const GsListWork &w, hipStream_t s)
{
    uint32_t total;
    if (!list_shape(planes, rows, cols, total) || (w.open && planes != 1) || !w.counts || !w.selected) return hipErrorInvalidValue;
    const GsListArgs a = list_args(w, parent, size, total, rows, cols, min_size);
    const unsigned groups = (unsigned)gs_list_groups(total);
    if (w.open) {
        const hipError_t e = hipMemsetAsync(w.open, 0, (size_t)((total + 31ull) / 32ull) * sizeof(uint32_t), s);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(gs_list_open_k, dim3(((unsigned)cols + 255u) / 256u), dim3(256), 0, s, parent, w.open, a.rows, a.cols);
    }
    hipLaunchKernelGGL(gs_list_count_k, dim3(groups), dim3(256), 0, s, a);
    hipLaunchKernelGGL(gs_list_scan_k, dim3(1), dim3(1024), 0, s, w.counts, groups, w.selected);
    return hipGetLastError();
}

hipError_t gs_launch_list_fill(const uint32_t *parent, uint32_t *size, int64_t planes, int64_t rows, int32_t cols, uint64_t min_size,
                               const GsListWork &w, GsComponentRecord *records, uint32_t *seams, hipStream_t s)
{
    uint32_t total;
    if (!list_shape(planes, rows, cols, total) || (seams && planes != 1) || !records) return hipErrorInvalidValue;
    GsListArgs a = list_args(w, parent, size, total, rows, cols, min_size);
    a.records = records;
    hipLaunchKernelGGL(gs_list_write_k, dim3((unsigned)gs_list_groups(total)), dim3(256), 0, s, a);
    const uint64_t per_group = 4ull * 64ull * (uint64_t)kChunks;
    hipLaunchKernelGGL(gs_list_gather_k, dim3((unsigned)((total + per_group - 1u) / per_group)), dim3(256), 0, s, a);
    if (seams)
        hipLaunchKernelGGL(gs_list_seam_k, dim3(((unsigned)cols + 255u) / 256u), dim3(256), 0, s, parent, size, a.rows, a.cols, seams);
    return hipGetLastError();
}
