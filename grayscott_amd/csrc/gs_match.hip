// gs_match.hip -- the overlaps of two planes' components (include/gs_hip.h: gs_fields_match, gs_members_match), formed behind
// three labellings on the same stream: `before` and `after` labelled and listed by the launches of gs_components.hip and
// gs_component_list.hip, each in label memory of its own, and the PIECES -- the connected pieces of the cells set in both planes,
// labelled by gs_launch_piece_labels from the two parent arrays, no plane is read a second time.  A piece lies inside exactly
// one before-component and one after-component, so one cell of it names both.  Entries are dense as everywhere: cell (r, c) of
// plane y is entry i = (y * rows + r) * cols + c, fewer than 2^32 in all.  After the lists' fill launches size[root] of
// `before` and of `after` is the root's record index (kUfUnset: not listed), and after the pieces' count and scan launches
// (gs_launch_list_count with min_size 1: every piece is selected) counts[] holds the exclusive prefix sums of the pieces per
// workgroup of 256 entries.  One launch remains:
//   pairs   gs_match_pairs_k: one thread per entry; the thread of a piece's root -- its first cell i -- takes the piece's slot,
//           prefix + its rank among the roots of its workgroup (the lists' write pattern: pieces come out in first-cell order,
//           so in plane order), and writes one 16-byte overlap: b = indexB[parentB[i]], a = indexA[parentA[i]], the piece's
//           cells.  Where either component is not listed the overlap is a DROPPED MARK: before = after = kUfUnset.  Every
//           thread writes its own slot alone; nothing is read that this launch writes.
// The host (gs_match_merge.h) makes the indices global, drops the marks, sorts and adds the cells of equal pairs.
//
// No kernel waits for another wave or workgroup: no flags, no spinning, no look-back; every dependency is a launch boundary.
// TERMINATION: the kernel has no loop but the one over the workgroup's four waves; nothing follows parent[] further than one
// step, because flatten left roots.  No atomics: every slot has one writer.
//
// Built with hipcc's default float mode, as gs_component_list.hip is (nothing here touches a float).
#include "gs_kernels.h"
#include "gs_unionfind.h" // kUfUnset

namespace {

struct GsMatchArgs {
    const uint32_t *parent_b, *index_b; // `before`: roots, and the record index of a root
    const uint32_t *parent_a, *index_a; // `after`
    const uint32_t *parent_p, *size_p;  // the pieces: roots, and the cells of a root
    const uint32_t *counts;             // pieces before each workgroup of 256 entries
    GsMatchOverlap *overlaps;
    uint32_t total;
};

__global__ __launch_bounds__(256) void gs_match_pairs_k(GsMatchArgs a)
{
    __shared__ uint32_t n[4];
    const uint32_t i = blockIdx.x * 256u + threadIdx.x; // (fewer than 2^32 entries: the grid's last workgroup cannot wrap)
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const bool root = i < a.total && a.parent_p[i] == i;
    const unsigned long long mine = __ballot(root);
    if (lane == 0u) n[wave] = (uint32_t)__popcll(mine);
    __syncthreads();
    if (!root) return;
    uint32_t slot = a.counts[blockIdx.x] + (uint32_t)__popcll(mine & ((1ull << lane) - 1ull));
    for (uint32_t w = 0u; w < wave; ++w) slot += n[w];
    // (a piece's cells are set in both planes: neither parent is kUfUnset here, and flatten left roots)
    const uint32_t b = a.index_b[a.parent_b[i]], c = a.index_a[a.parent_a[i]];
    const bool listed = b != kUfUnset && c != kUfUnset;
    GsMatchOverlap o;
    o.before = listed ? b : kUfUnset;
    o.after = listed ? c : kUfUnset;
    o.cells = a.size_p[i];
    a.overlaps[slot] = o;
}

} // namespace

hipError_t gs_launch_match_pairs(const uint32_t *parent_b, const uint32_t *index_b, const uint32_t *parent_a, const uint32_t *index_a,
                                 const uint32_t *parent_p, const uint32_t *size_p, const uint32_t *counts, int64_t planes,
                                 int64_t rows, int32_t cols, GsMatchOverlap *overlaps, hipStream_t s)
{
    if (planes < 1 || rows < 1 || cols < 1 || !overlaps || !counts) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)planes * (uint64_t)rows * (uint64_t)cols;
    if (total >= (1ull << 32)) return hipErrorInvalidValue;
    GsMatchArgs a{parent_b, index_b, parent_a, index_a, parent_p, size_p, counts, overlaps, (uint32_t)total};
    hipLaunchKernelGGL(gs_match_pairs_k, dim3((unsigned)gs_list_groups(total)), dim3(256), 0, s, a);
    return hipGetLastError();
}
