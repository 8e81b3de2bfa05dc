// gs_experiments.h -- every switch of libgs_hip.so that is NOT part of the product's interface, in one place.
//
// (1) Build-time switches of diagnostic builds (tools/ab_build.py NAME -DGS_...=v builds
//     grayscott_amd/variants/libgs_hip_NAME.so; GS_HIP_LIBRARY makes capi.py load it).  The shipped build sets
//     none of them.  A switch with a default gets it here (#ifndef NAME / #define NAME value: what ships), an entry
//     starts its comment line with the switch's name; tests/test_experiments_cpu.py holds the kernels to this list.
// (2) Run-time GS_HIP_* environment switches read by the launchers (A/B timing of launch policies, traces).
//     They never change results -- every combination is bit-identical and covered by the GPU parity suite --
//     and are documented for users in include/gs_hip.h ("Environment").
// Besides the switches, part (1) holds what a GS_TB_TRACE build needs beside its buffer: the stamp macros and the body of the
// host-side readers (gs_trace_read).
#pragma once
#include <cstdlib>

// ---- (1) build-time --------------------------------------------------------------------------------------
// Retired: the A/B switches whose experiments are closed (results: profiles/) and the forms they built are
//     gone from the source; f483d0f is the last commit that builds them.  Marching kernel: GS_TB_XLANE (0 = DPP wave
//     shifts), GS_TB_HSHARE, GS_TB_LATE_FETCH, GS_TB_AUX_LOAD, GS_TB_AUX_STORE, GS_VS_ABLATE_HALO (timing only, wrong
//     results).  Window kernel: GS_WIN_TAGGED (0 = round 4's flag exchange), GS_WIN_PAIR_SYNC, GS_WIN_PAIR_PRIO,
//     GS_WIN_PRIO_AHEAD / _LEVEL / _BEHIND, GS_WIN_WAVES_LEAVE_ALONE, GS_WIN_LATE_ROW, GS_WIN_FIRST_POLL_SLEEP,
//     GS_WIN_EDGE_POLLS_AT_ONCE, GS_WIN_POLL_SLEEP, GS_WIN_PAIR_POLL_SLEEP, GS_WIN_TRACE 3 and 4 (with GS_WIN_BUDGET,
//     GS_WIN_BUDGET_ADD; their tools are in tools/archive/).  Histograms (gs_hist_count.h): GS_HIST_FORM 1 and 2.
// GS_WIN_TRACE     (diagnostic builds of the persistent window kernel, gs_window_kernel.h) 1 = wave 0 of every workgroup
//                  stamps the 100 MHz real-time counter at seven points of each of its last 8 super-steps
//                  (tools/window_timeline.py); 2 = every wave of the first 256 workgroups stamps four points of each of the
//                  launch's last 4 steps (tools/window_step_timeline.py).
// GS_TB_TRACE      (defined = on; tools/wave_timeline.py) every wave of gs_step_tb_k leaves five stamps of the
//                  100 MHz real-time counter -- entry, first level-0 rows used (tick 3), level pipeline full (tick
//                  2K), last level-0 row taken (tick nticks - 2K), exit -- plus the shader-clock counter at entry
//                  and exit, its hardware id and its unit in a device buffer that gs_debug_trace_read*() copy out.
#if defined(GS_TB_TRACE) && defined(__HIPCC__)
constexpr int kTraceWords = 8, kTraceUnits = 1 << 17;
__device__ unsigned long long gs_trace_buf[kTraceWords * kTraceUnits];
__device__ __forceinline__ unsigned long long trace_now()
{
    unsigned long long t;
    asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    return t;
}
#define GS_TRACE_AT(COND, SLOT) do { if (COND) ts[SLOT] = trace_now(); } while (0)
#define GS_TRACE_PARAM , unsigned long long (&ts)[5] /* tb_march's extra parameter ... */
#define GS_TRACE_ARG , ts                            /* ... and what gs_step_tb_k passes for it */
// Copies the trace buffer of THIS translation unit's kernels out: the body of gs_debug_trace_read_<flavour> (the main unit)
// and gs_debug_trace_read_op (gs_step_op.hip).
static inline int32_t gs_trace_read(unsigned long long *dst, int32_t units, int32_t clear)
{
    if (units > kTraceUnits) units = kTraceUnits;
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(gs_trace_buf), (size_t)units * kTraceWords * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (clear) {
        void *p = nullptr;
        if (hipGetSymbolAddress(&p, HIP_SYMBOL(gs_trace_buf)) != hipSuccess) return -1;
        if (hipMemset(p, 0, (size_t)units * kTraceWords * sizeof(unsigned long long)) != hipSuccess) return -1;
    }
    return 0;
}
#else
#define GS_TRACE_AT(COND, SLOT) do { } while (0)
#define GS_TRACE_PARAM
#define GS_TRACE_ARG
#endif

// ---- (2) run-time ----------------------------------------------------------------------------------------
// Integer environment switch, clamped to [lo, hi]; `unset` when the variable is absent or empty.
//   GS_HIP_TRACE_LAUNCH   1 = print the first 64 kernel launches of the process (label, row ranges, layout)
//   GS_HIP_TRACE_TUNER    1 = print every timing window of gs_run's on-line tuner and its choice (and gs_fields_place's probes)
//   GS_HIP_PLACE_ALL      1 = gs_fields_place draws all its candidates even when it has two blocks of each kind (diagnostics)
//   GS_HIP_EDGE_KINDS     0 = every edge unit of the marching kernel takes the general path (default 1: cheap kinds)
//   GS_HIP_EDGE_SPLIT     0 / 1 = never / always dispatch edge units as two half-height units (default: by size)
//   GS_HIP_FAIR           0 / 1 = never / always run one-round launches as in-step 16-wave workgroups
//   GS_HIP_FAIR_FROM      progress (0 ... 256) from which the in-step form steers priorities (default 0)
//   GS_HIP_XCD_M          0 = plain workgroup order; n = XCD-aware renumbering in groups of 8 n (default: 16 on
//                         multi-round launches); GS_HIP_XCD_M_STREAM: the same for the single-step kernel
//   GS_HIP_TILE_LDS_FLOOR bytes of dynamic LDS the LDS-window kernel asks for at least (limits workgroups per CU)
//   GS_HIP_WINDOW_PATIENCE polls (2-3 us each) a wave of the persistent window kernel waits for its neighbours' cells
//                         before the launch gives up (default 2^20, 2-3 s; tests set 1 to provoke it)
//   GS_HIP_WINDOW_WAVES   "left,interior,right": waves in use per window of the left-most / inner / right-most tile column
//                         of the persistent window kernel's tiling (gs_window.cpp: plan_windows)
//   GS_HIP_QUIET_UNITS    0 = units at rest are recomputed like any other: the production entries run (default 1: the quiet
//                         entries where a call is eligible); read when a context is created
constexpr int kGsXcdGroupMax = 512; // 8 * 512 workgroups per renumbered group at most
inline int gs_env_int(const char *name, int unset, int lo, int hi)
{
    const char *v = std::getenv(name);
    if (!v || !*v) return unset;
    long x = std::strtol(v, nullptr, 10);
    if (x < lo) x = lo;
    if (x > hi) x = hi;
    return (int)x;
}
