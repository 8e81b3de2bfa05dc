// gs_hist_count.h -- what the kernels that count cells into histogram slots in LDS share (gs_histogram.hip,
// gs_region_hist.hip): the slot of a cell by the rule of include/gs_hip.h, and the wave's way of adding 64 cells to u32 words
// of LDS without 64 adds to one word.  Device code only; nothing here survives inlining.
#pragma once
#include <hip/hip_runtime.h>

// The slot of one cell (gs_hip.h): [0, bins) the bins, bins = below, bins + 1 = above, bins + 2 = nan; bins + 3 for a
// column outside the row.
__device__ __forceinline__ int slot_of(float x, bool valid, float lo, float hi, float scale, int bins)
{
    const bool isnan = x != x, below = x < lo, above = x > hi;
    const float in = (isnan || below || above) ? lo : x; // (keeps the conversion below defined; the slot is replaced)
    const float t = (in - lo) * scale;
    int b = (int)t;
    b = b < bins - 1 ? b : bins - 1;
    b = below ? bins : b;
    b = above ? bins + 1 : b;
    b = isnan ? bins + 2 : b;
    return valid ? b : bins + 3;
}

// The wave's run: `n` cells that belong to slot `slot` and are not in LDS yet.  Both are wave-uniform.
struct Run {
    int slot, n;
};

// 64 cells, one per lane (every lane active): the lanes whose slot is the first lane's go to the run, the others to LDS.
// `s` is the index of the lane's word in `h`, whatever the kernel makes of it: a plane's slot, or region and slot together.
// (Two other forms were measured and lost, profiles/histogram.md: every lane adds 1 to its slot in LDS; the run only when
// all 64 lanes hold one slot, else every lane adds.  gs_experiments.h names the last commit that builds them.)
__device__ __forceinline__ void count(unsigned *h, Run &run, int s, int lane)
{
    const int first = __builtin_amdgcn_readfirstlane(s);
    const int same = __popcll(__ballot(s == first));
    if (s != first) atomicAdd(&h[s], 1u);
    if (first == run.slot) {
        run.n += same;
    } else {
        if (lane == 0) atomicAdd(&h[run.slot], (unsigned)run.n);
        run.slot = first;
        run.n = same;
    }
}
