// gs_plane_scan.h -- what the kernels that scan planes for an observable share (gs_histogram.hip, gs_morphology.hip,
// gs_correlation.hip, gs_components.hip): the planes of a launch, the set rule, the grid's size, a lane's four-column load.
// Nothing here survives inlining.  Also plain C++: a host program gets the host half and gs_is_set (tests/cpp/plane_scan.cpp).
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define GS_PS_HD __host__ __device__ __forceinline__
#else
#define GS_PS_HD inline // (a host program: the device half below is left out)
#endif

// np (1..4) planes of one shape -- rows [0, rows) of `pitch` floats, `cols` columns -- repeated `stride` floats apart
// (ensembles: np = 2, a member's cells): plane y of the launch is p[y % np] + (y / np) * stride, and what a launch keeps per
// plane -- ranges, thresholds, rows above -- it keeps per p[], in front of the set.  That order and np, cols at the set's end
// are measured: fewest and widest argument loads, no VGPR more in gs_plane_quads_k (profiles/plane_scan_refactor.md).
struct GsPlaneSet {
    const float *p[4];
    int64_t stride;      // floats between one group of np planes and the next
    int64_t pitch, rows; // of every plane
    int32_t np;
    int32_t cols;        // of every plane
};

// True when every lane of a launch over these planes may read 16 bytes at once: rows, repeats and planes all begin on
// 16-byte boundaries, and so does whatever `also` names per plane (null entries do).
inline bool gs_reads_16_bytes(const float *const *planes, int np, int64_t repeat, int64_t stride, int64_t pitch,
                              const float *const *also = nullptr)
{
    bool vec = pitch % 4 == 0 && (repeat == 1 || stride % 4 == 0);
    for (int i = 0; i < np; ++i)
        vec = vec && reinterpret_cast<uintptr_t>(planes[i]) % 16 == 0 && (!also || reinterpret_cast<uintptr_t>(also[i]) % 16 == 0);
    return vec;
}

// The planes of a launch from its launcher's arguments, and gs_reads_16_bytes' verdict on them.
inline bool gs_plane_set(GsPlaneSet &set, const float *const *planes, int np, int64_t repeat, int64_t stride, int64_t pitch,
                         int64_t rows, int32_t cols, const float *const *also = nullptr)
{
    set = GsPlaneSet{{}, stride, pitch, rows, np, cols};
    for (int i = 0; i < np; ++i) set.p[i] = planes[i];
    return gs_reads_16_bytes(planes, np, repeat, stride, pitch, also);
}

// The set rule of include/gs_hip.h: a cell x is set when it is above the threshold, or, with the other sense, below it; NaN
// is never set.  The launchers negate the threshold where the sense is "below" and flip every cell's sign bit: x < t <=>
// -x > -t, NaN stays NaN.
GS_PS_HD bool gs_is_set(float x, uint32_t flip, float t)
{
    return __builtin_bit_cast(float, __builtin_bit_cast(uint32_t, x) ^ flip) > t;
}

// One threshold and its sense (!= 0: set above it) as gs_is_set takes them.
inline void gs_set_rule(float threshold, int32_t sense, float &t, uint32_t &flip)
{
    t = sense ? threshold : -threshold;
    flip = sense ? 0u : 0x80000000u;
}

// nt thresholds for each of np planes, thresholds[i * nt + k], with sense[i].
inline void gs_set_rules(float t[4][4], uint32_t flip[4], const float *thresholds, const int32_t *sense, int np, int nt)
{
    for (int i = 0; i < np; ++i)
        for (int k = 0; k < nt; ++k) gs_set_rule(thresholds[i * nt + k], sense[i], t[i][k], flip[i]);
}

// Workgroups per plane for `units` units of work, a wave taking one at a time: as many as there are units for (4 waves each),
// at most the caller's share of max_groups per plane -- fewer workgroups, fewer flushes --, and, with units_per_group > 0, never
// so few that one takes more than that: the bound that keeps a kernel's u32 counters from wrapping.  False: too large a grid.
inline bool gs_scan_groups(int64_t units, int64_t units_per_group, int64_t max_groups, int64_t nplanes, int64_t &groups)
{
    groups = (units + 3) / 4;
    const int64_t share = max_groups / nplanes > 1 ? max_groups / nplanes : 1;
    if (groups > share) groups = share;
    const int64_t least = units_per_group > 0 ? (units + units_per_group - 1) / units_per_group : 0;
    if (groups < least) groups = least;
    return groups * nplanes <= INT32_MAX;
}

#ifdef __HIPCC__
// Plane y of the launch and `which` of p[] it is a repeat of.
__device__ __forceinline__ const float *gs_plane_at(const GsPlaneSet &set, int64_t y, int &which)
{
    which = (int)(y % set.np);
    return set.p[which] + (y / set.np) * set.stride;
}

// Where a lane that holds columns c .. c + 3 of a row of `cols` columns reads them: the 16-byte form needs c + 3 < pitch only
// (the caller masks what lies beyond cols; a lane wholly outside reads column 0), the ragged one clamps every column.
struct GsLaneColumns {
    int cv, l0, l1, l2, l3;
};

__device__ __forceinline__ GsLaneColumns gs_lane_columns(int c, int cols)
{
    const int last = cols - 1;
    return {c < cols ? c : 0, c < last ? c : last, c + 1 < last ? c + 1 : last, c + 2 < last ? c + 2 : last,
            c + 3 < last ? c + 3 : last};
}

template <bool VEC>
__device__ __forceinline__ float4 gs_load_columns(const float *row, const GsLaneColumns &at)
{
    if (VEC) return *reinterpret_cast<const float4 *>(row + at.cv);
    return make_float4(row[at.l0], row[at.l1], row[at.l2], row[at.l3]);
}
#endif
