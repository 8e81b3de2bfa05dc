// gs_step_kernels.hip -- gfx950 (CDNA4, wave64) kernels for the Gray-Scott time step: the main translation unit of the step
// kernels (gs_step_flavour.h lists the others) -- the simple, streaming, resident, tile, window, LDS-staged and marching
// kernels' general variants, the ensemble kernels' plain and listed forms, and the launchers of all step kernels but the
// ensembles' noise forms (gs_step_noise.hip), handed to the host side as one table per flavour (gs_kernels.h: GsLaunchers).
//
// Arithmetic spec: compute_naive::Simulation::perform_step,
// compute/naive/src/lib.rs:42-83 -- for every cell, a row-major fold
//     acc = acc + w[i][j] * (elem - centre)
// over the 3x3 window CLIPPED to the grid, weights indexed from the window's top-left
// corner (:57-71), then the reaction update (:74-79).  Each reference operation is one
// rounded f32 operation here, in the same order; the step kernels' units are compiled with
// -ffp-contract=off so the compiler never fuses, each once per arithmetic flavour (gs_step_flavour.h: GS_MATH_FUSED).
//
// Facts the kernels rely on (derived from the spec, checked by tests/test_oracle_kat.py):
//   * the centre tap contributes w * (u - u) = +0 and acc is never -0, so it is skipped;
//   * a clipped (absent) neighbour equals "neighbour value := centre value" (adds +0);
//   * with the row above absent (global top edge) the centre row takes weight row 0 and the
//     row below weight row 1; same shift for the columns on the global left edge;
//   * "0.0f + first tap" is kept: it turns a -0 product into +0 exactly as the fold does.
//
// Kernels
//   gs_step_simple_k   one thread per cell, literal window loop (cross-check kernel).
//   gs_step_stream_k   one step per launch: a wave owns a 256-column strip (one 16-B load
//       per lane per row and species), marches down `rows_per_unit` rows keeping a 3-row
//       window in registers, and gets its left/right neighbours from the adjacent lanes
//       with DPP wave shifts (no LDS, no extra memory traffic); only lanes 0 and 63 fetch
//       one halo column each.  Each input element is read from HBM once per step except
//       the 2 rows shared by vertically adjacent units.  HBM-bound: 16 B per cell-step.
//   gs_step_tb_k<K,FAST> the production kernel of gs_run: K <= 4 time steps per launch
//       (temporal blocking), K register-resident time levels per wave, sacrificial edge
//       lanes instead of halo loads.  ~16 B of HBM traffic per cell for K steps;
//       VALU-issue bound for K >= 3.  Bit-identical to K single steps.
//   ..._pk             the periodic rule's forms (GsStepArgs::zero_halo = 2) of the simple, streaming, marching, tile and
//       ensemble kernels: kernels of their own, so that the code of the others does not depend on the rule's existence.
//       Units and windows on an edge read wrapped rows and columns and run the interior cell code; the resident kernels'
//       periodic forms (gs_run_resident_pk, gs_ens_resident_pk: ZH = 2) keep their LDS ring filled with the opposite edge.
//   ..._nk             the zero-flux (Neumann) rule's forms (GsStepArgs::zero_halo = 3) of the same kernels.  Edge units and
//       windows run the rule's edge cell (cell<ZH = 3>: a missing row or column is the cell's own) at every fused level; the
//       resident forms (ZH = 3) keep their LDS ring filled with the edge cells' own values.  Slab seams read ghost rows.
//   ..._mk<..., RULE>  the parameter map's forms (second argument GsMapPlanes, gs_ctx_set_param_map) of the simple,
//       streaming and marching kernels, one instance per kernel set of a boundary rule (RULE = rule_set()): the reaction
//       takes F[r, c] and F[r, c] + K[r, c] of the cell it updates (react's map form); the Laplacian is the rule's own.  The
//       marching kernel's map forms (K = 1..4, 1, 2 and 4 columns per lane, the general variant and, strict only, .op) are
//       built in a translation unit of their own (gs_step_map.hip).  The difference-sharing, fair-progress, tile, resident,
//       window, LDS-staged and ensemble kernels have none.
//   ..._wk<..., RULE>  the domain mask's forms (second argument GsMaskPlanes, gs_ctx_set_mask) of the same three kernels:
//       every cell through cell_masked (a tap that reads a wall reads the cell's own value; a wall keeps its input), from
//       the link words formed at attach time.  The marching forms, the same set as the map's, are built in a translation
//       unit of their own (gs_step_mask.hip).  No difference sharing: a wall breaks it.
//   ..._zk<..., RULE>  the noise forms (second argument GsNoiseArgs, gs_ctx_set_noise) of the same three kernels: the
//       reference cell, then react_noise (gs_cell.h) -- a Philox2x32-10 draw at the cell's global (row, column) with the key
//       of the level's step, one multiply and one add per species.  The marching forms, the same set as the map's, are built
//       in a translation unit of their own (gs_step_noise.hip).  No difference sharing, no units at rest.
//   gs_ens_resident_z*, gs_ens_tile_z*  the noise forms of the two ensemble kernels (second argument GsEnsNoiseArgs,
//       gs_members_set_noise; gs_ensemble.h): a seed, sigmas and a step counter per member, the step key formed on the
//       device.  Built in the noise translation units too, with their launchers (gs_launch_ens_*_noise_*).
//
// This file includes the flavour macros (gs_step_flavour.h) and the kernels -- gs_cell.h (per-cell arithmetic), gs_march.h
// (gs_step_tb_k and its variant with full difference sharing), gs_single_step.h (simple / stream / LDS-staged),
// gs_lds_resident.h (resident and LDS-window kernels), gs_window_kernel.h (the persistent window kernel) -- and holds their
// launchers.  The launchers of the simple, streaming and marching kernels take the slab's attachment (GsAttached: none, a
// parameter map, a domain mask or noise), index one table of names and one of entries by its kind, and hand its planes on
// as the kernel's second argument.  Build-time switches of diagnostic builds (none is set in the shipped build) and the
// run-time GS_HIP_* switches of the launchers live in gs_experiments.h.
#include "gs_step_flavour.h"
#include <cstdio>
#include <mutex>

#include "gs_cell.h"
#include "gs_march.h"
#include "gs_single_step.h"
#include "gs_lds_resident.h"
#include "gs_ensemble.h"
#include "gs_window_kernel.h"
#include "gs_ens_launch.h"

// A table of names (gs_step_flavour.h: GS_RULES_OF) per kind of attachment (GsAttached::kind): the uniform kernels' names,
// then the parameter map's kernel sets' (the same rules, a "/map" suffix behind the rule's), the domain mask's (a "/mask"
// suffix) and the noise forms' (a "/noise" suffix)
#define GS_KINDS(M, BASE) {GS_RULES_OF(M, BASE, ""), GS_RULES_OF(M, BASE, "/map"), GS_RULES_OF(M, BASE, "/mask"), GS_RULES_OF(M, BASE, "/noise")}
#define GS_NAME1(BASE, R) GS_NAME(BASE, "", R)

// The attachment as a launcher takes it: a known kind with its planes in place.
static bool attached_ok(const GsAttached &at)
{
    return at.kind == GS_ATTACH_NONE || (at.kind == GS_ATTACH_MAP && at.plane[0] && at.plane[1]) || (at.kind == GS_ATTACH_MASK && at.plane[0]) ||
           at.kind == GS_ATTACH_NOISE;
}
// Launches entry `fn` of the attachment's kernel set (256-thread workgroups, no LDS): the uniform kernels take `args` alone,
// the map's and the mask's forms the slab's planes as their second argument, the noise forms the keys and sigmas.
static hipError_t launch_attached(const void *fn, long blocks, GsStepArgs &args, const GsAttached &at, hipStream_t s)
{
    GsMapPlanes mp{at.plane[0], at.plane[1]};
    GsMaskPlanes mk{at.plane[0]};
    GsNoiseArgs nz = at.noise;
    void *kargs[] = {&args, at.kind == GS_ATTACH_MAP     ? static_cast<void *>(&mp)
                            : at.kind == GS_ATTACH_NOISE ? static_cast<void *>(&nz)
                                                         : static_cast<void *>(&mk)};
    return hipLaunchKernel(fn, dim3((unsigned)blocks), dim3(256), kargs, 0, s);
}

hipError_t GS_SUFFIX(gs_launch_simple)(const GsStepArgs &a, hipStream_t s, const char **name, const GsAttached &at)
{
    // [kind][rule]: the periodic and zero-flux rules run kernels of their own, and so do the parameter map (gs_step_simple_mk)
    // and the domain mask (gs_step_simple_wk); the noise forms are gs_step_simple_zk
    static const char *const names[GS_ATTACH_KINDS][3] = GS_KINDS(GS_NAME1, "simple");
    static const void *const fns[GS_ATTACH_KINDS][3] = {
        {GS_PLAIN_FN(gs_step_simple_k), GS_PLAIN_FN(gs_step_simple_pk), GS_PLAIN_FN(gs_step_simple_nk)},
        {GS_FN(gs_step_simple_mk, 0), GS_FN(gs_step_simple_mk, 1), GS_FN(gs_step_simple_mk, 2)},
        {GS_FN(gs_step_simple_wk, 0), GS_FN(gs_step_simple_wk, 1), GS_FN(gs_step_simple_wk, 2)},
        {GS_FN(gs_step_simple_zk, 0), GS_FN(gs_step_simple_zk, 1), GS_FN(gs_step_simple_zk, 2)}};
    if (!attached_ok(at)) return hipErrorInvalidValue;
    const int per = rule_set(a.zero_halo);
    if (name) *name = names[at.kind][per];
    const long nrows = (long)(a.ra1 - a.ra0) + (a.rb1 - a.rb0);
    if (nrows <= 0 || a.cols <= 0) return hipSuccess;
    if (per == 1 && (a.top_present || a.bottom_present)) return hipErrorInvalidValue; // (periodic: single slab only)
    const long bpr = (a.cols + 255) >> 8;
    const long blocks = nrows * bpr;
    if (blocks > 0x7fffffffL) return hipErrorInvalidConfiguration;
    GsStepArgs args = a;
    return launch_attached(fns[at.kind][per], blocks, args, at, s);
}

// `steps` time steps of a grid of at most kResidentCells cells in one launch (gs_run_resident_k);
// the result is stored in the out-planes when steps is odd, else back in the in-planes.
hipError_t GS_SUFFIX(gs_launch_resident)(const GsStepArgs &a, int steps, hipStream_t s, const char **name)
{
    static const char *const names[3][2] = GS_RULES(GS_NAMES_OP, "resident-lds");
    // [rule][variant]
    static const void *const fns[4][2] = {{GS_FN(gs_run_resident_k, 0, 0), GS_FN(gs_run_resident_k, kOp, 0)},
                                          {GS_FN(gs_run_resident_k, 0, 1), GS_FN(gs_run_resident_k, kOp, 1)},
                                          {GS_FN(gs_run_resident_pk, 0), GS_FN(gs_run_resident_pk, kOp)},
                                          {GS_FN(gs_run_resident_nk, 0), GS_FN(gs_run_resident_nk, kOp)}};
    const long cells = (long)a.rows * a.cols;
    if (a.rows <= 0 || a.cols <= 0 || cells > kResidentCells || steps < 0 || a.top_present || a.bottom_present)
        return hipErrorInvalidValue;
    int fast = a.fast & (GS_MATH_FUSED ? 0 : 3);
    if (fast != 3) fast = 0; // only the variant for the default parameters is built besides the general one
    const int zh = a.zero_halo >= 2 && a.zero_halo <= 3 ? a.zero_halo : (a.zero_halo ? 1 : 0); // gs_boundary
    if (name) *name = names[rule_set(zh)][fast ? 1 : 0];
    const void *fn = fns[zh][fast ? 1 : 0];
    const size_t lds = (size_t)4 * (a.rows + 2) * (a.cols + 2) * sizeof(float); // <= 74 KB (1 x 1536 cells)
    { // more than 64 KB of dynamic LDS needs the opt-in, per device and device function
        const hipError_t e = gs_ensure_dyn_lds(fn, lds > 64 * 1024 ? (size_t)80 * 1024 : lds);
        if (e != hipSuccess) return e;
    }
    GsStepArgs args = a;
    int to_out = steps & 1;
    void *kargs[] = {&args, &steps, &to_out};
    // only the waves that hold cells take part (and in the barrier of every step)
    const long threads = cells >= kResidentThreads ? kResidentThreads : ((cells + 63) / 64) * 64;
    return hipLaunchKernel(fn, dim3(1), dim3((unsigned)threads), kargs, lds, s);
}

// K <= kGsTileMaxSteps time steps of a single slab in one launch of gs_run_tile_k (in-planes -> out-planes).
// `shape`: 0 = windows of 32 rows x 64 columns (2 rows per wave), 1 = 16 x 64 (1 row), 2 = 64 x 64 (4 rows);
// 2K < window rows.
hipError_t GS_SUFFIX(gs_launch_tile)(const GsStepArgs &a, int k, int shape, hipStream_t s, const char **name)
{
    static const char *const names[3][3][2] = GS_RULES(GS_TILE_NAMES, "");
    static const void *const fns[3][3][2] = {GS_TILE_FNS(gs_run_tile_k), GS_TILE_FNS(gs_run_tile_pk), GS_TILE_FNS(gs_run_tile_nk)};
    static const int rpw[3] = {2, 1, 4};
    const int per = rule_set(a.zero_halo); // the periodic and zero-flux rules: gs_run_tile_pk / _nk
    if (a.rows <= 0 || a.cols <= 0 || k < 1 || k > kTileMaxK || shape < 0 || shape > 2 || a.top_present || a.bottom_present ||
        2 * k >= tile_rows(rpw[shape]))
        return hipErrorInvalidValue;
    int fast = a.fast & (GS_MATH_FUSED ? 0 : 3);
    if (fast != 3) fast = 0; // only the variant for the default parameters is built besides the general one
    if (name) *name = names[per][shape][fast ? 1 : 0];
    const long ho = tile_rows(rpw[shape]) - 2 * k, wo = kTileCols - 2 * k;
    const long tiles = ((a.rows + ho - 1) / ho) * ((a.cols + wo - 1) / wo);
    if (tiles > 0x7fffffffL) return hipErrorInvalidConfiguration;
    const void *fn = fns[per][shape][fast ? 1 : 0];
    size_t lds = tile_lds_bytes(rpw[shape]);
    static const int lds_floor = gs_env_int("GS_HIP_TILE_LDS_FLOOR", 0, 0, 160 * 1024);
    if (lds < (size_t)lds_floor) lds = (size_t)lds_floor; // experiment: limit the workgroups per CU
    { // more than 64 KB of dynamic LDS needs the opt-in, per device and device function
        const hipError_t e = gs_ensure_dyn_lds(fn, lds);
        if (e != hipSuccess) return e;
    }
    GsStepArgs args = a;
    void *kargs[] = {&args, &k};
    return hipLaunchKernel(fn, dim3((unsigned)tiles), dim3(kTileWaves * 64), kargs, lds, s);
}

// Ensembles (gs_ensemble.h): gs_ens_launch.h's bodies over the plain kernels and, with `list` (device list of the active
// members' indices), over their listed twins, named with a "/listed" suffix.
hipError_t GS_SUFFIX(gs_launch_ens_resident)(const GsEnsArgs &e, const uint32_t *list, int steps, int fast, hipStream_t s, const char **name)
{
    static const char *const names[2][3][2] = {GS_RULES(GS_NAMES_OP, "ensemble-resident"), GS_RULES_OF(GS_NAMES_OP, "ensemble-resident", "/listed")};
    // [rule][variant][cells per thread: 1, 2, 4, 8]; the clipped rule has no 8-cell form (gs_ens_resident_cpt)
#define GS_CPT_FNS(KER, ...) {GS_FN(KER, 1, __VA_ARGS__), GS_FN(KER, 2, __VA_ARGS__), GS_FN(KER, 4, __VA_ARGS__), GS_FN(KER, 8, __VA_ARGS__)}
#define GS_ENS_RESIDENT_FNS(K, PK, NK)                                                                \
    {{{GS_FN(K, 1, 0, 0), GS_FN(K, 2, 0, 0), GS_FN(K, 4, 0, 0), nullptr},                             \
      {GS_FN(K, 1, kOp, 0), GS_FN(K, 2, kOp, 0), GS_FN(K, 4, kOp, 0), nullptr}},                      \
     {GS_CPT_FNS(K, 0, 1), GS_CPT_FNS(K, kOp, 1)},                                                    \
     {GS_CPT_FNS(PK, 0), GS_CPT_FNS(PK, kOp)},                                                        \
     {GS_CPT_FNS(NK, 0), GS_CPT_FNS(NK, kOp)}}
    static const void *const fns[2][4][2][4] = {GS_ENS_RESIDENT_FNS(gs_ens_resident_k, gs_ens_resident_pk, gs_ens_resident_nk),
                                                GS_ENS_RESIDENT_FNS(gs_ens_resident_lk, gs_ens_resident_lpk, gs_ens_resident_lnk)};
#undef GS_ENS_RESIDENT_FNS
#undef GS_CPT_FNS
    return ens_launch_resident(e, names[list ? 1 : 0], fns[list ? 1 : 0], list ? &list : nullptr, steps, fast, s, name);
}
hipError_t GS_SUFFIX(gs_launch_ens_tile)(const GsEnsArgs &e, const uint32_t *list, int k, int shape, int fast, hipStream_t s, const char **name)
{
    static const char *const names[2][3][3][2] = {GS_RULES(GS_TILE_NAMES, "ensemble-"), GS_RULES_OF(GS_TILE_NAMES, "ensemble-", "/listed")};
    static const void *const fns[2][3][3][2] = {{GS_TILE_FNS(gs_ens_tile_k), GS_TILE_FNS(gs_ens_tile_pk), GS_TILE_FNS(gs_ens_tile_nk)},
                                                {GS_TILE_FNS(gs_ens_tile_lk), GS_TILE_FNS(gs_ens_tile_lpk), GS_TILE_FNS(gs_ens_tile_lnk)}};
    return ens_launch_tile(e, names[list ? 1 : 0], fns[list ? 1 : 0], list ? &list : nullptr, k, shape, fast, s, name);
}

// One persistent launch of gs_run_window_k: `x.steps` time steps of a single slab, in-planes -> out-planes.
// rpw: rows per wave (a window is at most 16 rpw rows x 128 columns); x.desc holds the caller's tiling of the grid.
hipError_t GS_SUFFIX(gs_launch_window)(const GsStepArgs &a, const GsWindowArgs &x, int rpw, hipStream_t s, const char **name)
{
    // (5 rows per wave: 80-row windows.  The 96-row form of round 4 -- 6 rows per wave, 12 cells per lane -- spilled 43
    // registers in the strict build and tied with the marching kernel where it applied; it is gone.)
    static const char *const names[3] = {"window-r5/" GS_MATH_NAME, "window-r5/" GS_MATH_NAME ".op", "window-r5/" GS_MATH_NAME ".op.ds"};
    if (a.rows <= 0 || a.cols <= 0 || a.top_present || a.bottom_present || rpw != 5 || x.steps < 1 || x.k < 2 ||
        x.k > 8 || (x.k & 1) || 2 * x.k >= win_rows(rpw) || 2 * x.k + 2 > kWinCols || !x.flags || !x.abort || !x.xu[0] || !x.xu[1] || !x.xv[0] || !x.xv[1])
        return hipErrorInvalidValue;
    if (!x.desc || x.n_windows < 1 || x.seq < 1) return hipErrorInvalidValue;
    if (a.zero_halo >= 2) return hipErrorInvalidValue; // no periodic or zero-flux form (gs_api.cpp refuses them before this)
    // byte offsets inside a plane are 32-bit in the kernel
    if ((long)(a.rows + 8) * a.pitch * 4 > 0x7fffffffL) return hipErrorInvalidValue;
    int fast = a.fast & (GS_MATH_FUSED ? 0 : 7);
    // only the variants for the default parameters are built besides the general one: .op, and .op.ds with full
    // difference sharing inside a wave's band (gs_options.share_taps = 2 switches it off)
    if ((fast & 3) != 3) fast = 0;
    if (name) *name = names[fast == 7 ? 2 : (fast ? 1 : 0)];
    const void *fn = nullptr;
#define GS_WIN_FN(R) (fast == 7 ? reinterpret_cast<const void *>(&GS_SUFFIX(gs_run_window_k)<R, GS_MATH_FUSED ? 0 : 7>) \
                      : fast    ? reinterpret_cast<const void *>(&GS_SUFFIX(gs_run_window_k)<R, GS_MATH_FUSED ? 0 : 3>) \
                                : reinterpret_cast<const void *>(&GS_SUFFIX(gs_run_window_k)<R, 0>))
    fn = GS_WIN_FN(5);
#undef GS_WIN_FN
    const size_t lds = win_lds_bytes();
    { // more than 64 KB of dynamic LDS needs the opt-in, per device and device function
        const hipError_t e = gs_ensure_dyn_lds(fn, lds);
        if (e != hipSuccess) return e;
    }
    GsStepArgs args = a;
    GsWindowArgs xa = x;
    void *kargs[] = {&args, &xa};
    return hipLaunchKernel(fn, dim3((unsigned)x.n_windows), dim3(kWinWaves * 64), kargs, lds, s);
}

hipError_t GS_SUFFIX(gs_launch_stream)(const GsStepArgs &a, hipStream_t s, const char **name, const GsAttached &at)
{
    // [kind][rule]: gs_step_stream_pk (the periodic rule, single slab) and _nk (the zero-flux rule), the parameter map's
    // gs_step_stream_mk, the domain mask's gs_step_stream_wk and the noise forms gs_step_stream_zk
    static const char *const names[GS_ATTACH_KINDS][3] = GS_KINDS(GS_NAME1, "stream-g2");
    static const void *const fns[GS_ATTACH_KINDS][3] = {
        {GS_FN(gs_step_stream_k, 2), GS_FN(gs_step_stream_pk, 2), GS_FN(gs_step_stream_nk, 2)},
        {GS_FN(gs_step_stream_mk, 2, 0), GS_FN(gs_step_stream_mk, 2, 1), GS_FN(gs_step_stream_mk, 2, 2)},
        {GS_FN(gs_step_stream_wk, 2, 0), GS_FN(gs_step_stream_wk, 2, 1), GS_FN(gs_step_stream_wk, 2, 2)},
        {GS_FN(gs_step_stream_zk, 2, 0), GS_FN(gs_step_stream_zk, 2, 1), GS_FN(gs_step_stream_zk, 2, 2)}};
    if (!attached_ok(at)) return hipErrorInvalidValue;
    const int per = rule_set(a.zero_halo);
    if (name) *name = names[at.kind][per];
    if (a.cols <= 0 || a.rows_per_unit <= 0 || (per == 1 && (a.top_present || a.bottom_present))) return hipErrorInvalidValue;
    const long rpu = a.rows_per_unit;
    const long chunks = ((long)(a.ra1 - a.ra0) + rpu - 1) / rpu + ((long)(a.rb1 - a.rb0) + rpu - 1) / rpu;
    if (chunks <= 0) return hipSuccess;
    const long strips = (a.cols + 255) >> 8;
    const long blocks = (chunks * strips + 3) / 4;
    if (blocks > 0x7fffffffL) return hipErrorInvalidConfiguration;
    GsStepArgs args = a;
    // XCD-aware order, as in gs_launch_tb: this kernel IS bound by HBM, so the re-reads the XCDs' L2s absorb are
    // time -- 16384^2 365 k -> 376 k (6.0 TB/s algorithmic), 4096^2 323 k -> 347 k, 1080 x 1920 171 k -> 186 k; 8192^2
    // unchanged on average (265-333 k from one context to the next either way: the four planes' placement decides).
    // Groups of 8 x 64 workgroups lose 6 % (profiles/archive/r03_sweeps.md, section 12).  GS_HIP_XCD_M_STREAM = 0 / n: off / 8 n.
    static const int xcd_env = gs_env_int("GS_HIP_XCD_M_STREAM", -1, 0, kGsXcdGroupMax);
    args.xcd_m = xcd_env >= 0 ? xcd_env : 16;
    return launch_attached(fns[at.kind][per], blocks, args, at, s);
}

// Kernel entry for k fused steps, specialisation `fast` (already reduced to {0, 1, 3}) and cpl columns per lane; `per`:
// the kernel set of the boundary rule (rule_set: 1 = the periodic rule's gs_step_tb_pk, 2 = the zero-flux rule's _nk).
static const void *tb_entry(int k, int fast, int cpl, int wg = 4, int per = 0)
{
    // the general variant's entries: [rule][cpl 1, 2, 4][k - 1] of 4-wave workgroups, [rule][cpl 1, 2] of the
    // fair-progress form (16-wave workgroups, 4 fused steps)
#define GS_TB_FNS(KER, C) {GS_FN(KER, 1, 0, C, 4), GS_FN(KER, 2, 0, C, 4), GS_FN(KER, 3, 0, C, 4), GS_FN(KER, 4, 0, C, 4)}
    static const void *const fns[3][3][4] = {{GS_TB_FNS(gs_step_tb_k, 1), GS_TB_FNS(gs_step_tb_k, 2), GS_TB_FNS(gs_step_tb_k, 4)},
                                             {GS_TB_FNS(gs_step_tb_pk, 1), GS_TB_FNS(gs_step_tb_pk, 2), GS_TB_FNS(gs_step_tb_pk, 4)},
                                             {GS_TB_FNS(gs_step_tb_nk, 1), GS_TB_FNS(gs_step_tb_nk, 2), GS_TB_FNS(gs_step_tb_nk, 4)}};
#undef GS_TB_FNS
#if GS_MATH_FUSED
    // (2 columns per lane need 129 registers in the fused flavour, one more than a wave of a 16-wave workgroup may have:
    // the variant spilled a register to scratch; one-round launches of the fused flavour run as 4-wave workgroups)
    static const void *const fns16[3][2] = {{GS_FN(gs_step_tb_k, 4, 0, 1, 16), nullptr}, {GS_FN(gs_step_tb_pk, 4, 0, 1, 16), nullptr},
                                            {GS_FN(gs_step_tb_nk, 4, 0, 1, 16), nullptr}};
#else
    static const void *const fns16[3][2] = {{GS_FN(gs_step_tb_k, 4, 0, 1, 16), GS_FN(gs_step_tb_k, 4, 0, 2, 16)},
                                            {GS_FN(gs_step_tb_pk, 4, 0, 1, 16), GS_FN(gs_step_tb_pk, 4, 0, 2, 16)},
                                            {GS_FN(gs_step_tb_nk, 4, 0, 1, 16), GS_FN(gs_step_tb_nk, 4, 0, 2, 16)}};
#endif
    if (wg == 16 && (k != 4 || (cpl != 1 && cpl != 2))) return nullptr;
    if (fast) {
#if !GS_MATH_FUSED
        return gs_tb_op_kernel_strict(k, fast, cpl, wg, per);
#endif
    }
    if (k < 1 || k > 4 || (cpl != 1 && cpl != 2 && cpl != 4)) return nullptr;
    return wg == 16 ? fns16[per][cpl - 1] : fns[per][cpl == 4 ? 2 : cpl - 1][k - 1];
}

// Waves per SIMD the register file allows a kernel entry: 512 registers per lane, allocated in steps
// of 8 (MI355X_MICROARCH.md, register files); the kernels use no LDS memory.
static int tb_waves_of(const void *f)
{
    static const void *occ_fn[64];
    static int occ_waves[64], occ_n = 0;
    static std::mutex occ_lock; // contexts on different threads launch through here
    std::lock_guard<std::mutex> occ_guard(occ_lock);
    for (int i = 0; i < occ_n; ++i)
        if (occ_fn[i] == f) return occ_waves[i];
    hipFuncAttributes attr;
    attr.numRegs = 0;
    int w = 2;
    if (hipFuncGetAttributes(&attr, f) == hipSuccess && attr.numRegs > 0) {
        const int alloc = ((attr.numRegs + 7) / 8) * 8;
        w = 512 / alloc > 8 ? 8 : (512 / alloc < 1 ? 1 : 512 / alloc);
    } else {
        (void)hipGetLastError();
    }
    if (gs_env_int("GS_HIP_TRACE_TUNER", 0, 0, 1))
        std::fprintf(stderr, "gs_hip: kernel entry %p: %d registers -> %d waves per SIMD\n", f, attr.numRegs, w);
    if (occ_n < 64) { occ_fn[occ_n] = f; occ_waves[occ_n++] = w; }
    return w;
}

// The variant that runs for GsStepArgs::fast = `fast` with k fused steps, cpl columns per lane and wg waves per
// workgroup: 0 (general), 1 (side weights 0.5), 3 (and dt == 1), 7 (and full difference sharing: built for 2 columns
// per lane, 2 to 4 fused steps) or 15 (and across lanes).
static int tb_reduce_fast(int fast, int k = 0, int cpl = 0, int wg = 4, int per = 0)
{
    // The fused build has no use for bit 0 (its taps are sub + fma already) and measured slower
    // with bit 1 (profiles/archive/r01_sweeps.md, runs 48/49): it always runs the general variant.  dt == 1
    // alone (fast == 2) is not worth a variant either, and bit 2 means nothing without the other two.
    fast &= GS_MATH_FUSED ? 0 : 15;
    if (!(fast & 1)) return 0;
    if ((fast & 7) == 7) {
#if !GS_MATH_FUSED
        if ((fast & 8) && gs_tb_op_kernel_strict(k, 15, cpl, wg, per)) return 15;
        if (gs_tb_op_kernel_strict(k, 7, cpl, wg, per)) return 7;
#endif
        return 3;
    }
    return fast & 3;
}

// Kernel entry of the marching kernel in the kernel set of an attachment of `kind` (4-wave workgroups; `fast` reduced).
static const void *tb_entry_of(int kind, int k, int fast, int cpl, int per)
{
    return kind == GS_ATTACH_MAP    ? GS_SUFFIX(gs_tb_map_kernel)(k, fast, cpl, per)
           : kind == GS_ATTACH_MASK ? GS_SUFFIX(gs_tb_mask_kernel)(k, fast, cpl, per)
           : kind == GS_ATTACH_NOISE ? GS_SUFFIX(gs_tb_noise_kernel)(k, fast, cpl, per)
                                    : tb_entry(k, fast, cpl, 4, per);
}
// ... and the variant that runs there for GsStepArgs::fast = `fast`.  The parameter map's and the domain mask's kernels:
// .op (3) where the side weights are 0.5 and dt == 1 in the strict flavour and that form is built (gs_tb_mask_kernel_*
// lacks two), else the general one.
static int tb_fast_of(int kind, int fast, int k, int cpl, int per)
{
    if (kind == GS_ATTACH_NONE) return tb_reduce_fast(fast, k, cpl, 4, per);
    const int f = !GS_MATH_FUSED && (fast & 3) == 3 ? 3 : 0;
    return f && !tb_entry_of(kind, k, f, cpl, per) ? 0 : f;
}

// Wave slots of the chip for the kernel entry a launch with these parameters would use (the tuner's
// "a launch of exactly r rounds" candidates, gs_tuner.cpp); 0 = no such entry.  `boundary`: gs_boundary.
int GS_SUFFIX(gs_tb_wave_slots)(int k, int fast, int cpl, int boundary, int kind)
{
    if (k < 1 || k > 4 || (cpl != 1 && cpl != 2 && cpl != 4) || kind < GS_ATTACH_NONE || kind >= GS_ATTACH_KINDS) return 0;
    const int per = rule_set(boundary);
    const void *fn = tb_entry_of(kind, k, tb_fast_of(kind, fast, k, cpl, per), cpl, per);
    return fn ? 1024 * tb_waves_of(fn) : 0;
}

// K fused steps over the row ranges of GsStepArgs; on slab seams the ghost rows must be K deep.
hipError_t GS_SUFFIX(gs_launch_tb)(const GsStepArgs &a, int k, hipStream_t s, const char **name, const GsAttached &at, GsQuiet *quiet)
{
    if (quiet) { quiet->need = 0; quiet->launched = 0; }
    // "cN": N columns per lane (4 = the wide layout); ".op": the variant specialised for the
    // default (Oono-Puri) side weights, with or without dt == 1
    // ".op.ds": ... and with full difference sharing (cells_vshare)
    // ".op.dx": ... and across lanes (cells_xshare)
    // "f": the fair-progress form (16-wave workgroups) of one-round launches
#define GS_TB_KS(B, C, V, R) {GS_NAME(B "1" C, V, R), GS_NAME(B "2" C, V, R), GS_NAME(B "3" C, V, R), GS_NAME(B "4" C, V, R)}
#define GS_TB_NAMES(B, C, R) {GS_TB_KS(B, C, "", R), GS_TB_KS(B, C, ".op", R), GS_TB_KS(B, C, ".op.ds", R), GS_TB_KS(B, C, ".op.dx", R)}
#define GS_TB_LAYOUTS(B, R) {GS_TB_NAMES(B, "c1", R), GS_TB_NAMES(B, "c2", R), GS_TB_NAMES(B, "", R)}
#define GS_TB_VARIANTS(B, R) {GS_NAME(B, "", R), GS_NAME(B, ".op", R), GS_NAME(B, ".op.ds", R), GS_NAME(B, ".op.dx", R)}
#define GS_TB16_LAYOUTS(B, R) {GS_TB_VARIANTS(B "c1f", R), GS_TB_VARIANTS(B "c2f", R)}
    // [kind][rule][cpl 1, 2, 4][variant][k - 1]: the uniform kernels, the parameter map's (gs_step_tb_mk), the domain mask's (gs_step_tb_wk)
    static const char *const names[GS_ATTACH_KINDS][3][3][4][4] = GS_KINDS(GS_TB_LAYOUTS, "tb-k"); // (... and the noise forms, gs_step_tb_zk)
    static const char *const names16[3][2][4] = GS_RULES(GS_TB16_LAYOUTS, "tb-k4");  // [rule][cpl 1, 2][variant]
#undef GS_TB16_LAYOUTS
#undef GS_TB_VARIANTS
#undef GS_TB_LAYOUTS
#undef GS_TB_NAMES
#undef GS_TB_KS
    auto name_of = [](int f) { return f == 15 ? 3 : (f == 7 ? 2 : (f ? 1 : 0)); };
    if (k < 1 || k > 4 || a.cols <= 0 || a.rows_per_unit <= 0) return hipErrorInvalidValue;
    if (a.zero_halo == 2 && (a.top_present || a.bottom_present)) return hipErrorInvalidValue; // periodic: single slab, no bands
    const int cpl = a.cpl == 0 ? 4 : a.cpl;
    if (cpl != 1 && cpl != 2 && cpl != 4) return hipErrorInvalidValue;
    // the periodic and zero-flux rules run kernels of their own (gs_step_tb_pk / _nk and kin), named with a "/periodic" /
    // "/neumann" suffix
    const int per = rule_set(a.zero_halo);
    // the parameter map and the domain mask (at.kind): kernels of their own, the general or the .op variant, 4-wave
    // workgroups only
    if (!attached_ok(at)) return hipErrorInvalidValue;
    const int fast = tb_fast_of(at.kind, a.fast, k, cpl, per);
    if (name) *name = names[at.kind][per][cpl == 1 ? 0 : (cpl == 2 ? 1 : 2)][name_of(fast)][k - 1];
    const long rpu = a.rows_per_unit;
    const long rows_a = (long)a.ra1 - a.ra0;
    const long W = tb_cols_per_wave(k, cpl);
    const long strips = (a.cols + W - 1) / W;
    // Kernel entry first: the taper below needs its occupancy.
    const void *fn = tb_entry_of(at.kind, k, fast, cpl, per);
    if (!fn) return hipErrorInvalidValue;
    const int waves = tb_waves_of(fn);
    // Tapered tail (consecutive passes are dependent launches that cannot overlap, so the drain phase
    // of a launch is idle time): when the launch is at least two rounds of the chip's wave slots, the
    // last round of units is an eighth as tall as the others and the round before it half as tall.
    // Measured at 16384^2 (profiles/archive/r02_sweeps.md, section 7): +1...2 % over round 1's single level
    // (the last two rounds at a quarter), and unit heights of 128-192 rows become usable.
    const long slots = 1024L * waves; // 256 CUs x 4 SIMDs x waves per SIMD
    long big_chunks = rows_a > 0 ? rows_a / rpu : 0, small = rpu, mid_chunks = -1, tiny = rpu;
    if ((rows_a / rpu) * strips >= 2 * slots) {
        const long h1 = rpu / 2 >= 2L * k ? rpu / 2 : 2L * k;
        const long h2 = rpu / 8 >= 2L * k ? rpu / 8 : 2L * k;
        const long c1 = (slots + strips - 1) / strips, c2 = (slots + strips - 1) / strips;
        const long rows12 = c1 * h1 + c2 * h2;
        if (h1 < rpu && rows12 <= rows_a / 3) {
            big_chunks = (rows_a - rows12) / rpu;
            small = h1;
            if (h2 < h1) {
                tiny = h2;
                mid_chunks = (rows_a - big_chunks * rpu - c2 * h2 + h1 - 1) / h1;
                while (mid_chunks > 0 && rows_a - big_chunks * rpu - mid_chunks * h1 < 0) --mid_chunks;
                if (mid_chunks < 0) mid_chunks = 0;
            }
        }
    }
    const long rest = rows_a - big_chunks * rpu;
    const long chunks_a = rows_a <= 0 ? 0
                        : mid_chunks < 0 ? big_chunks + (rest + small - 1) / small
                                         : big_chunks + mid_chunks + (rest - mid_chunks * small + tiny - 1) / tiny;
    const long chunks = chunks_a + ((long)(a.rb1 - a.rb0) + rpu - 1) / rpu;
    if (chunks <= 0) return hipSuccess;
    if (k > a.ghost && (a.top_present || a.bottom_present)) return hipErrorInvalidValue;
    GsStepArgs args = a;
    args.big_chunks = (int32_t)big_chunks;
    args.small_rpu = (int32_t)small;
    args.mid_chunks = (int32_t)mid_chunks;
    args.tiny_rpu = (int32_t)tiny;
    // Row range of chunk cc of range a (the kernel's formulas); the last `bot` chunks -- the ones the
    // grid's bottom edge can touch, at least one -- are dispatched first, then the chunks from the top.
    auto chunk_rows = [&](long cc, long &r0, long &r1) {
        if (cc < big_chunks) { r0 = a.ra0 + cc * rpu; r1 = r0 + rpu; }
        else if (mid_chunks < 0 || cc < big_chunks + mid_chunks) { r0 = a.ra0 + big_chunks * rpu + (cc - big_chunks) * small; r1 = r0 + small < a.ra1 ? r0 + small : a.ra1; }
        else { r0 = a.ra0 + big_chunks * rpu + mid_chunks * small + (cc - big_chunks - mid_chunks) * tiny; r1 = r0 + tiny < a.ra1 ? r0 + tiny : a.ra1; }
    };
    long bot = 0, r0 = 0, r1 = 0;
    if (!a.bottom_present)
        for (; bot < chunks_a; ++bot) { chunk_rows(chunks_a - 1 - bot, r0, r1); if (!(r1 + k > a.rows)) break; }
    if (bot < 1 && chunks_a > 0) bot = 1; // the launch order of earlier rounds: the last chunk first
    args.bot_first = (int32_t)bot;
    // Edge units as two halves each when the launch is about one round of wave slots (every unit starts at
    // once, so the slow edge units would finish last: 1080 x 1920 +5.7 %, 2048 x 4096 +1.6 %; from two rounds
    // up the edge-first order does the job and halves only add recomputed rows: 8192^2 -1 %;
    // profiles/archive/r02_sweeps.md, section 11).  The kernel's dispatch order: the outer strips of every chunk, then all strips of the
    // bottom `bot` and the top chunk row of range a, then the rest.
    static const int split_env = gs_env_int("GS_HIP_EDGE_SPLIT", -1, 0, 1);
    const long er = ((strips - 1) * W + tb_sacrificial_lanes(k, cpl) * cpl >= a.cols && strips >= 2) ? 2 : 1, ne = 1 + er;
    bool split = 4 * chunks * strips <= 5 * slots && rpu >= 2;
    // Units at rest (GsQuiet, below): a pass that may skip is, on a grid mostly at rest, a launch of less than one round
    // whose length is the edge units' march -- they never rest -- so they come as halves there as in every such launch.
    // (Every position has a word per half, and a whole unit writes both: the passes of a call agree on the layout whether
    // their edge units come whole or as halves.)
    const bool quiet_ok = !GS_MATH_FUSED && quiet && quiet->mode >= 1 && quiet->mode <= 3 && at.kind == GS_ATTACH_NONE && per == 0 &&
                          fast == 15 && cpl == 2 && a.rb1 <= a.rb0 && !a.top_present && !a.bottom_present && rpu >= k && small >= k &&
                          tiny >= k && 2 * chunks * strips <= 0x7fffffffL;
    if (quiet_ok && quiet->mode == 3 && rpu >= 2) split = true;
    if (split_env >= 0) split = split_env != 0;
    long units = chunks * strips;
    args.edge_split = 1;
    args.edge_chunks = 0;
    if (split) {
        args.edge_split = 2;
        if (strips <= ne) {
            units = chunks * strips * 2;
        } else {
            const long nec = chunks_a > 0 ? (bot + 1 < chunks ? bot + 1 : chunks) : 0;
            args.edge_chunks = (int32_t)nec;
            units = chunks * ne * 2 + nec * (strips - ne) * 2 + (chunks - nec) * (strips - ne);
        }
    }
    // A launch that fits the chip in ONE round of 16-wave workgroups (one per CU, 4 waves per SIMD) runs the
    // fair-progress form of the kernel (tb_march<FAIR>): every unit starts at once there and, left to the
    // SIMDs' oldest-first arbitration, the waves of a SIMD finish one after the other, the last one alone.
    // Not for short marches of the 1-column layout: there most of a unit's ticks are the memory-bound filling
    // of the level pipeline, and waves left out of phase by the oldest-first arbitration hide each other's
    // waits.  Free-running / in step, same box (profiles/archive/r03_sweeps.md, section 2): 1 column per lane, 10-row
    // units 430 k / 390 k, 12 rows 465 k / 443 k, 16 rows 524 k / 514 k, 20 rows 565 k / 573 k, 40 rows 677 k / 705 k;
    // 2 columns per lane, 10 rows 523 k / 537 k, 15 rows 615 k / 633 k, 19 rows 687 k / 738 k, 38 rows 782 k / 865 k.
    // GS_HIP_FAIR = 0 / 1 forces it off / on.
    static const int fair_env = gs_env_int("GS_HIP_FAIR", -1, 0, 1);
    const bool fair = at.kind == GS_ATTACH_NONE && a.allow_fair && units <= 4096 && units > 1024 && (fair_env < 0 ? (cpl == 2 || rpu >= 20) : fair_env != 0);
    const int fast16 = fair ? tb_reduce_fast(a.fast, k, cpl, 16, per) : 0;
    const void *fair_fn = fair ? tb_entry(k, fast16, cpl, 16, per) : nullptr;
    static const int fair_from_env = gs_env_int("GS_HIP_FAIR_FROM", -1, 0, 256);
    args.fair_from = fair_from_env >= 0 ? fair_from_env : 0;
    void *kargs[] = {&args};
    if (fair_fn) {
        if (name) *name = names16[per][cpl == 1 ? 0 : 1][name_of(fast16)];
        return hipLaunchKernel(fair_fn, dim3((unsigned)((units + 15) / 16)), dim3(1024), kargs, 0, s);
    }
    const long blocks = (units + 3) / 4;
    if (blocks > 0x7fffffffL) return hipErrorInvalidConfiguration;
    // XCD-aware unit order (GsStepArgs::xcd_m): the dispatcher deals workgroups over the 8 XCDs round-robin, so
    // four-strip neighbours in the grid land on eight different L2s and each fetches the columns and rows their
    // windows share for itself.  With every XCD taking 16 consecutive workgroups of each group of 128, the HBM
    // reads of a 16384^2 launch fall from 2.376 to 2.239 GiB (minimum 2.0; FETCH_SIZE, tools/archive/fetch_ab.sh) and the
    // launch gains 0.3-0.5 % (8192^2 +0.8 %, 4 / 8 slabs on one GPU +1.4 / +0.6 %).  Larger groups read no less
    // (68: 2.226 GiB) and run slower (-2 %, 136: -6 %: an XCD's share of the last groups is all tall or all short
    // units).  Launches of about one round keep the plain order: 1080 x 1920 loses 1.2 % with the renumbering
    // (profiles/archive/r03_sweeps.md, section 12).  GS_HIP_XCD_M = 0 / n forces it off / to groups of 8 n.
    static const int xcd_env = gs_env_int("GS_HIP_XCD_M", -1, 0, kGsXcdGroupMax);
    args.xcd_m = xcd_env >= 0 ? xcd_env : (units >= 2 * slots ? 16 : 0);
    // the edge units at the head of the dispatch order stay dealt over all XCDs (they are the slow ones)
    args.xcd_first = (int32_t)(((chunks * ne * (args.edge_split == 2 ? 2 : 1) + 3) / 4 + 7) / 8 * 8);
#if !GS_MATH_FUSED
    // Units at rest (GsQuiet): the quiet entry in place of gs_step_tb_dx_k's 4-wave form where the geometry allows it -- a
    // whole slab with the grid's edges above and below it as one row range, and every chunk but the last (an edge chunk) at
    // least k rows high: the input window of an interior unit then lies within the chunks above and below its own and the
    // strips left and right of it, the nine positions whose words it reads.  Same label: it is the same march.
    if (quiet_ok) {
        if (const void *qfn = gs_tb_quiet_kernel_strict(k)) {
            quiet->need = 2 * chunks * strips; // a word per position and half
            if (quiet->need <= quiet->cap && quiet->in && quiet->out && quiet->edge_skips && quiet->skipped) {
                GsQuiet q = *quiet;
                void *qargs[] = {&args, &q};
                quiet->launched = units;
                // ... of them units of edge positions: the outer strips of every chunk and every strip of the chunks that
                // touch the grid's first or last rows (the top chunk and the last `bot`), halves counted one each
                const long ends = bot + 1 < chunks ? bot + 1 : chunks, inner = strips <= ne ? 0 : (chunks - ends) * (strips - ne);
                quiet->edge_launched = split ? units - inner : chunks * strips - inner;
                return hipLaunchKernel(qfn, dim3((unsigned)blocks), dim3(256), qargs, 0, s);
            }
            if (quiet->mode == 1) return hipSuccess; // (the caller makes room and comes again)
        }
    }
#endif
    return launch_attached(fn, blocks, args, at, s);
}

hipError_t GS_SUFFIX(gs_launch_lds)(const GsStepArgs &a, hipStream_t s, const char **name)
{
    if (name) *name = "lds-tile16/" GS_MATH_NAME;
    if (a.cols <= 0 || a.zero_halo >= 2) return hipErrorInvalidValue; // no periodic or zero-flux form (gs_api.cpp refuses them first)
    const long chunks = ((long)(a.ra1 - a.ra0) + kLdsTileRows - 1) / kLdsTileRows +
                        ((long)(a.rb1 - a.rb0) + kLdsTileRows - 1) / kLdsTileRows;
    if (chunks <= 0) return hipSuccess;
    const long strips = (a.cols + 255) >> 8;
    const long blocks = chunks * strips;
    if (blocks > 0x7fffffffL) return hipErrorInvalidConfiguration;
    GsStepArgs args = a;
    void *kargs[] = {&args};
    return hipLaunchKernel(reinterpret_cast<const void *>(&GS_SUFFIX(gs_step_lds_k)), dim3((unsigned)blocks),
                           dim3(256), kargs, 0, s);
}

// F + K of the parameter map (gs_ctx_set_param_map): compute/naive/src/lib.rs:77's `feed_rate + kill_rate`, one f32 add
// per cell in this translation unit's float mode -- strict: a sub-normal sum is flushed (the DenormalsFlusher); fused:
// kept.  (Named without the flavour suffix: it is no step kernel, and tests/test_isa_guard.py holds those to their size.)
#if GS_MATH_FUSED
#define GS_MAP_RATES_K gs_map_rates_keep_k
#else
#define GS_MAP_RATES_K gs_map_rates_flush_k
#endif
namespace {
__global__ __launch_bounds__(256) void GS_MAP_RATES_K(const float *feed, const float *kill, float *fpk, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        fpk[i] = feed[i] + kill[i];
}
} // namespace
hipError_t GS_SUFFIX(gs_launch_map_rates)(const float *feed, const float *kill, float *fpk, size_t n, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    const size_t blocks = (n + 255) / 256 < 65536 ? (n + 255) / 256 : 65536;
    GS_MAP_RATES_K<<<dim3((unsigned)blocks), dim3(256), 0, s>>>(feed, kill, fpk, n);
    return hipGetLastError();
}
#undef GS_MAP_RATES_K

// The launchers of this flavour, as the host side takes them (gs_kernels.h: gs_launchers).  Host pass only: the compiler
// would emit a constant of namespace scope for the device too, where the functions it names do not exist.
#if !defined(__HIP_DEVICE_COMPILE__)
const GsLaunchers GS_SUFFIX(gs_launchers) = {
    GS_SUFFIX(gs_launch_simple),       GS_SUFFIX(gs_launch_stream),   GS_SUFFIX(gs_launch_resident),
    GS_SUFFIX(gs_launch_tb),           GS_SUFFIX(gs_launch_tile),     GS_SUFFIX(gs_launch_lds),
    GS_SUFFIX(gs_launch_window),       GS_SUFFIX(gs_tb_wave_slots),   GS_SUFFIX(gs_launch_map_rates),
    GS_SUFFIX(gs_launch_ens_resident), GS_SUFFIX(gs_launch_ens_tile), GS_SUFFIX(gs_launch_ens_resident_noise),
    GS_SUFFIX(gs_launch_ens_tile_noise)};
#endif

#if defined(GS_WIN_TRACE)
extern "C" int32_t GS_SUFFIX(gs_debug_win_trace_read)(unsigned long long *dst)
{
    return hipMemcpyFromSymbol(dst, HIP_SYMBOL(gs_win_trace), sizeof(unsigned long long) * 1024 * 8 * 8) == hipSuccess ? 0 : -1;
}
#endif

#if defined(GS_TB_TRACE)
extern "C" int32_t GS_SUFFIX(gs_debug_trace_read)(unsigned long long *dst, int32_t units, int32_t clear) { return gs_trace_read(dst, units, clear); }
#endif
