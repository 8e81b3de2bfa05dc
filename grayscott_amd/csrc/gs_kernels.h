// gs_kernels.h -- host/device contract between the host side (gs_api.cpp, gs_tuner.cpp, gs_window.cpp, gs_fields.cpp,
// gs_attached.cpp, gs_ensemble.cpp, gs_dyn_lds.cpp) and the gfx950 kernels.
//
// One "plane" is a row-major f32 array of one species in one slot for one row slab:
//   element (r, c) of the slab, r in [-ghost, rows + ghost) (rows outside [0, rows) = ghost rows),
//   c in [0, pitch), lives at  base + r * pitch + c ;  pitch % 64 == 0 (256-B rows).
// Columns [cols, pitch) are padding: readable, writable, never used as neighbours.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// Largest grid (cells) gs_launch_resident_* takes (4 planes of (rows + 2) x (cols + 2) floats in LDS: at most
// 74 KB).  Above, the LDS-window kernel with its many workgroups is faster (profiles/archive/r02_sweeps.md, section 10).
constexpr int kGsResidentCells = 1536;
// gs_launch_tile_*: the most time steps one launch advances its tiles by.
constexpr int kGsTileMaxSteps = 8;

struct GsStepArgs {
    const float *in_u, *in_v; // local row 0, col 0 of the input planes
    float *out_u, *out_v;     // same for the output planes
    int32_t rows;             // rows owned by this slab
    int32_t cols;             // valid columns
    int32_t pitch;            // row pitch in floats
    // Up to two half-open local row ranges to update: [ra0, ra1) and [rb0, rb1).
    int32_t ra0, ra1, rb0, rb1;
    // 1 when the ghost row above / below holds a neighbouring slab's row (slab seam),
    // 0 when that side is a global edge (naive's clipped window applies there).
    int32_t top_present, bottom_present;
    int32_t ghost;         // ghost rows stored above / below the slab (>= fused steps on seams)
    int32_t rows_per_unit; // rows one wave marches over
    // Tapered tail of range a (temporal-blocking kernel, filled in by its launcher): the first
    // `big_chunks` chunks have rows_per_unit rows, the rest `small_rpu` rows, so that the units
    // dispatched last are short and the launch drains quickly.
    int32_t big_chunks, small_rpu;
    // second taper level: after `mid_chunks` chunks of small_rpu rows the rest have tiny_rpu rows
    // (mid_chunks < 0: one level only)
    int32_t mid_chunks, tiny_rpu;
    // how many of range a's LAST chunks are dispatched first (the chunks a bottom grid edge can touch;
    // at least 1), filled in by the launcher
    int32_t bot_first;
    // 2 = units on a global edge are dispatched as two half-height units (1 = whole): the outer strips of
    // every chunk and all strips of the first `edge_chunks` chunks in dispatch order (the bottom and top
    // chunk rows).  Edge units run the general path, ~1.6x as slow: in a launch of one or two rounds of wave
    // slots, where every unit starts at once, whole ones would finish last.  Filled in by the launcher.
    int32_t edge_split, edge_chunks;
    // Parameter-specialised variants of the temporal-blocking kernel (bit-identical results, fewer
    // instructions): bit 0 = the four side weights w[0][1], w[1][0], w[1][2], w[2][1] are exactly
    // 0.5f, bit 1 = dt is exactly 1.0f.  Both hold for Parameters::default().
    int32_t fast;
    // Columns per lane of the temporal-blocking kernel: 4 (0 means 4), 2 or 1.
    int32_t cpl;
    // 1 = this launch has the GPU to itself (a single slab, no row bands): a launch of one round may then run
    // as 16-wave workgroups that keep step (gs_launch_tb).  0 on slab chains and row bands: workgroups that
    // own whole CUs until all their waves end would keep the boundary-band kernel, the ghost-row copies and
    // RCCL's kernels out until the end of the launch (8 slabs on one GPU: 0.79 instead of 0.88 of one slab).
    int32_t allow_fair;
    // 1 = edge units of the temporal-blocking kernel take the cheap kinds of edge path where one applies
    // (gs_step_tb_k); 0 = the general path for all of them (GS_HIP_EDGE_KINDS=0, A/B timing).  Same results.
    int32_t edge_kinds;
    // In-step form: the progress (0 ... 256) from which a wave's priority is steered; before, the waves run as
    // the arbitration leaves them (filled in by the launcher).
    int32_t fair_from;
    // XCD-aware unit order (filled in by the launcher; 0 = off).  The dispatcher deals workgroups over the 8 XCDs
    // round-robin, so workgroup b runs on XCD b % 8.  From workgroup xcd_first on, every group of 8 * xcd_m
    // workgroups is renumbered so that the xcd_m workgroups an XCD gets are consecutive ones -- neighbours in the
    // grid, whose overlapping rows and columns then meet in that XCD's L2.
    int32_t xcd_m, xcd_first;
    // Boundary rule on global edges (gs_boundary in gs_hip.h): 0 = naive's clipped window (weights anchored at the
    // window's top-left corner), 1 = full window with zeros outside the grid, 2 = periodic (single slab only), 3 = zero
    // flux (a neighbour outside the grid is the nearest cell inside it).  The launchers run the last two rules' own
    // kernels, gs_*_pk / gs_*_nk and the resident kernels' ZH = 2 / 3 instances: a kernel that tests this field for
    // truth only ever sees 0 or 1.
    int32_t zero_halo;
    float w[3][3];         // stencil weights, row-major (parameters.rs:87-88)
    float du, dv, feed, feed_plus_kill, dt;
};
// Parameter map (gs_ctx_set_param_map): local row 0, column 0 of one slab's F and F + K planes, laid out like the species'
// planes (same pitch, ghost rows and guards), so that a map load reuses the byte offset of the U load at the same cell.
// The second argument of the map kernels (gs_*_mk): GsStepArgs, and with it every other kernel's code, stays as it is.
struct GsMapPlanes {
    const float *feed, *fpk;
};
// Domain mask (gs_ctx_set_mask): local row 0, column 0 of one slab's link plane -- a u32 link word per cell (gs_cell.h:
// link_bit), in the species' layout like the map planes.  The second argument of the mask kernels (gs_*_wk).
struct GsMaskPlanes {
    const float *link;
};
// Units at rest (gs_step_tb_dx_qk): two words per unit position -- row chunk cc of range a, strip -- of
// the planes a full pass reads (`in`) and of the ones it writes (`out`), at [2 * (cc * strips + strip) + part]: part 0 / 1
// = the upper / lower half of the chunk's rows, as an edge unit dispatched in two halves (edge_split = 2) divides them.
// kQuietRest = every cell of the grid in that part's rows x the strip's output columns is bitwise (U, V) = (1.0f, +0.0f) in
// that slot's planes (the padding columns a right-edge strip also stores count for nothing); kQuietActive and 0 (unknown)
// claim nothing.  A whole unit writes both words and a half its own -- two halves of a position are two waves with no
// order between them, so no word has two writers in a pass and none needs an atomic; a position is at rest when both
// parts are.  A position outside the grid does not exist and counts as at rest: no tap reads it.
// Edge positions (first and last strips, chunks that touch the grid's first or last rows) have words like any other under
// the clipped rule: the reference accumulates weight * (tap - centre) over the taps that exist, every one of them +-0 in a
// window at rest, so (1, +0) is a fixed point on the edges and in the corners as it is inside (finite weights).  Under
// the zero-halo rule it is not -- a halo cell of 0 next to U = 1 is a tap of -1, those cells really change -- and there
// an edge position's words stay 0: its units and their inner neighbours always compute.
// The second argument of the quiet entries: GsStepArgs, and with it every other kernel's code, stays as it is.  mode: 1 =
// the first full pass of a gs_run (no word is read; every unit computes and writes its words in `out`: an interior unit
// after its march, by the march's check of what it stored; a unit of an edge position before it, "at rest" when every cell
// of the input window of its march is), 2 = the second (`in` is read: a unit whose own part there says "active" writes
// "active" without a look), 3 = every later one (a unit leaves at once when every part of the existing positions among
// the nine around it is at rest in `in` and its own part -- a whole unit: both -- in `out`; the other half's word in
// `out` is that half's to write in the same pass and is not read).  A half shorter than K rows, whose window reaches past
// the other half into the next chunk, is covered: the nine positions hold it.  cap: the words each array holds.  The
// launcher hands this back with `need` = the words the launch's geometry takes, `launched` = its units and `edge_launched`
// = those of edge positions among them, or 0 when the launch is not one of the quiet entries' (it then ran the production
// entry and touched no word); with need > cap in mode 1 it launches nothing.
constexpr uint32_t kQuietRest = 1, kQuietActive = 2;
constexpr int kQuietCounters = 64, kQuietCounterStride = 16; // the skipped-unit counters: 64 lines of them, 128 bytes apart
struct GsQuiet {
    const uint32_t *in;
    uint32_t *out;
    uint32_t *edge_skips; // += 1 per skipping unit of an edge position, at the index of its word (no atomic: one writer)
    // += 1 per skipping interior unit, at [(workgroup % kQuietCounters) * kQuietCounterStride + which]: which = 2 for a unit next
    // to an edge position, 0 for a unit with interior positions all around it (tb_unit<QUIET>)
    unsigned long long *skipped;
    int32_t mode;
    int32_t pad;
    int64_t cap, need, launched, edge_launched; // (host side only)
};
// Noise (gs_ctx_set_noise; include/gs_hip.h: the definition).  The second argument of the noise kernels (gs_*_zk): the step
// keys of the pass -- level j (1 .. K) of a fused pass computes step step0 + j - 1 with key[j - 1]; a single step uses
// key[0] --, the two sigmas and the global row of the slab's local row 0 (of a row band: of the band's first row), so that a
// cell at local row r -- a ghost row's included -- draws at (row0 + r, column).  The noise has no planes.
struct GsNoiseArgs {
    uint32_t key[4];
    float sigma_u, sigma_v;
    uint32_t row0;
    uint32_t pad;
};
// What a context's per-cell data (a map, a mask or a noise term, one at a time) is to the launchers of the simple, streaming
// and marching kernels: the kernel set it selects -- GS_ATTACH_NONE: the uniform kernels -- and one slab's planes, local row
// 0, column 0: the map's F and F + K, or the mask's link plane; the noise's keys, sigmas and first global row.  The launchers
// hand them to the kernels as GsMapPlanes / GsMaskPlanes / GsNoiseArgs.
enum { GS_ATTACH_NONE = 0, GS_ATTACH_MAP = 1, GS_ATTACH_MASK = 2, GS_ATTACH_NOISE = 3, GS_ATTACH_KINDS = 4 };
struct GsAttached {
    int kind = GS_ATTACH_NONE;
    const float *plane[2] = {nullptr, nullptr};
    GsNoiseArgs noise = {};
};

// gs_launch_window_*: one persistent launch for a whole gs_run on grids of ONE round of register-resident windows.
// Every workgroup owns a rectangle of the grid (GsWindowDesc; the rectangles tile the grid) and keeps it plus a k-cell
// apron in registers: `active` window rows (waves beyond them idle) x 128 columns.  Every k steps it stores the k-cell
// ring of its owned cells into the exchange planes as granules {value, exchange number} and polls the granules of its
// own apron cells until they carry that number.  Exchange e uses the planes of parity e & 1.  (The kernel reads neither
// `nbr` nor `n_nbr`: the workgroups whose cells a window's apron covers are the planner's business: its neighbour
// limit decides which tilings plan_windows accepts.)
// The input planes are never written: a launch that gives up (abort set) has destroyed nothing.
// Windows of one tile column share their height, and columns whose cells cost more (the grid's left and right edge
// under the clipped rule) get lower windows, so that every workgroup's step takes the same time: they all wait for
// their neighbours at every exchange, the slowest sets the pace (gs_window.cpp: plan_windows).
constexpr int kGsWindowMaxNbr = 14;
struct GsWindowDesc {
    int32_t r0, c0;    // first owned row / column (global)
    int32_t oh, ow;    // owned rows / columns (the last window of a tile column / row may reach beyond the grid)
    int32_t active;    // window rows in use: oh + 2 k rounded up to whole waves (a multiple of rpw, <= 16 rpw)
    int32_t n_nbr;     // workgroups whose owned cells lie in this window's apron
    int32_t nbr[kGsWindowMaxNbr];
};
struct GsWindowArgs {
    float *xu[2], *xv[2];      // exchange planes: local row 0, column 0; the field planes' pitch, at least the grid's rows
    int32_t *flags;            // two words per workgroup, diagnostics only: a wave that gave up leaves (wave, exchange) and
                               // its polls there (resolve_window prints them); the exchange itself uses no flag
    int32_t *abort;            // sticky, 0 or the `seq` of the launch in which a poll ran out of patience (workgroups not
                               // co-resident): every workgroup of that launch and of every later one then leaves
    const GsWindowDesc *desc;  // one per workgroup (device memory)
    int32_t n_windows;
    int32_t steps;             // time steps of this launch (>= 1)
    int32_t k;                 // steps per exchange: even, 2 ... 8
    int32_t epoch;             // exchange numbers left in the planes by earlier launches are <= epoch
    int32_t patience;          // polls before a workgroup gives up
    int32_t seq;               // this launch's number on its context (>= 1): what a workgroup that gives up leaves in *abort
};

// Ensembles (gs_ensemble.h): `members` independent grids of one shape, each with its own parameters, in dense planes
// [members, rows, cols] (pitch = cols).  One entry per member in a device table, read with scalar loads: a workgroup
// belongs to one member.  feed_plus_kill is the reference's f32 add (compute/naive/src/lib.rs:77), formed by the host.
struct GsEnsParams {
    float w[3][3];
    float du, dv, feed, feed_plus_kill, dt;
    int32_t pad[2]; // 64 B per member: two s_load_dwordx8
};
// Largest member the resident ensemble kernel takes: LDS (4 planes of (rows + 2) x (cols + 2) floats, at most 160 KiB per
// workgroup) and cells per thread of a 1024-thread workgroup -- 8 under the zero-halo rule, 4 under the clipped rule,
// whose cells carry their eight weights in registers (8 cells per thread spill at 128 VGPRs).
constexpr size_t kGsEnsResidentMaxLds = 160 * 1024;
// Cells per thread of the resident ensemble kernel for members of rows x cols (1, 2, 4 or 8), 0 = not resident.
// boundary: gs_boundary -- the periodic (2) and zero-flux (3) rules have the zero-halo rule's capacity: no per-cell
// weights either.  (Their 8-cell forms hold 75 registers, 6 waves per SIMD where the zero-halo rule's run 8: members of
// 4097 to about 4900 cells, whose LDS would let two workgroups share a CU, get one.)
inline int gs_ens_resident_cpt(long rows, long cols, int boundary)
{
    const long cells = rows * cols;
    if (rows <= 0 || cols <= 0 || (size_t)16 * (rows + 2) * (cols + 2) > kGsEnsResidentMaxLds) return 0;
    const long need = (cells + 1023) / 1024;
    return need <= 1 ? 1 : need <= 2 ? 2 : need <= 4 ? 4 : (need <= 8 && boundary != 0) ? 8 : 0;
}
// Most workgroups one ensemble launch dispatches (grid x 1024 threads stays below 2^32); the launchers split above.
constexpr long kGsEnsMaxGroups = 1L << 21;
struct GsEnsArgs {
    const float *in_u, *in_v; // member 0, row 0, column 0 of the input planes
    float *out_u, *out_v;
    const GsEnsParams *params; // members entries (device)
    int64_t first;             // member of workgroup 0 of this launch (launches are split at kGsEnsMaxGroups); the listed
                               // forms (a launch with a `list`): its position in the list of active members
    int32_t members;           // members in this launch
    int32_t rows, cols;
    int32_t zero_halo;         // gs_boundary: 0 clipped, 1 zero halo, 2 periodic, 3 zero flux
};
// Noise of an ensemble (gs_members_set_noise; include/gs_hip.h): one entry per member in a device table beside GsEnsParams,
// read with scalar loads.  The member's step index at a launch is GsEnsNoiseArgs::step0 + step_offset (u64, wrapping):
// step0 is the ensemble's run_steps when the launch is enqueued, so nothing is uploaded per launch; the host adjusts the
// offsets when a member's noise is set and when a retired member comes back (the steps it sat out).
struct GsEnsNoise {
    float sigma_u, sigma_v;
    uint32_t seed_lo, seed_hi;
    uint32_t offset_lo, offset_hi;
    uint32_t pad[2]; // 32 B per member: one s_load_dwordx8
};
// The second argument of the ensemble kernels' noise forms (gs_ens_resident_z*, gs_ens_tile_z*).  list: the device list of
// the active members' indices, as the listed forms take it, or nullptr when every member runs (GsEnsArgs::first then counts
// members, else positions in the list): one wave-uniform branch, no listed twins.
struct GsEnsNoiseArgs {
    const GsEnsNoise *table; // members entries (device)
    const uint32_t *list;
    uint64_t step0;
};

// Launchers, one table per arithmetic flavour (gs_math in include/gs_hip.h), defined by the step kernels' main unit
// (gs_step_kernels.hip).  Each launcher returns the hipError_t of the launch.  `name` receives a static kernel-variant
// label.  `at` (simple, stream and marching kernels): the slab's attachment -- the launch then runs the kernel set of its
// kind.  `quiet`: GsQuiet, or nullptr.  `list` (ensembles): the device list of the active members' indices, or nullptr when
// every member runs.  map_rates: fpk[i] = feed[i] + kill[i] over n floats, one f32 add in the flavour's float mode (strict: a
// sub-normal sum is flushed, as the reference's DenormalsFlusher does).
struct GsLaunchers {
    hipError_t (*simple)(const GsStepArgs &a, hipStream_t s, const char **name, const GsAttached &at);
    hipError_t (*stream)(const GsStepArgs &a, hipStream_t s, const char **name, const GsAttached &at);
    hipError_t (*resident)(const GsStepArgs &a, int steps, hipStream_t s, const char **name);
    hipError_t (*tb)(const GsStepArgs &a, int k, hipStream_t s, const char **name, const GsAttached &at, GsQuiet *quiet);
    hipError_t (*tile)(const GsStepArgs &a, int k, int shape, hipStream_t s, const char **name);
    hipError_t (*lds)(const GsStepArgs &a, hipStream_t s, const char **name);
    hipError_t (*window)(const GsStepArgs &a, const GsWindowArgs &x, int rpw, hipStream_t s, const char **name);
    int (*tb_wave_slots)(int k, int fast, int cpl, int boundary, int kind);
    hipError_t (*map_rates)(const float *feed, const float *kill, float *fpk, size_t n, hipStream_t s);
    hipError_t (*ens_resident)(const GsEnsArgs &e, const uint32_t *list, int steps, int fast, hipStream_t s, const char **name);
    hipError_t (*ens_tile)(const GsEnsArgs &e, const uint32_t *list, int k, int shape, int fast, hipStream_t s, const char **name);
    hipError_t (*ens_resident_noise)(const GsEnsArgs &e, const GsEnsNoiseArgs &z, int steps, int fast, hipStream_t s, const char **name);
    hipError_t (*ens_tile_noise)(const GsEnsArgs &e, const GsEnsNoiseArgs &z, int k, int shape, int fast, hipStream_t s, const char **name);
};
extern const GsLaunchers gs_launchers_strict, gs_launchers_fused;
// The launchers of flavour `math` (gs_math: GS_MATH_FUSED = 1, else strict).
inline const GsLaunchers &gs_launchers(int math) { return math == 1 ? gs_launchers_fused : gs_launchers_strict; }

// Entry points of the parameter-specialised temporal-blocking kernels (strict flavour only; their
// own translation unit, gs_step_op.hip).  nullptr for an unknown variant.
// wg: waves per workgroup, 4 or 16 (the fair-progress form of one-round launches: K = 4, cpl 1 or 2 only);
// rule: the kernel set of the boundary rule, 0 = the clipped and zero-halo rules' kernels, 1 = the periodic rule's
// (gs_step_tb_pk and kin), 2 = the zero-flux rule's (gs_step_tb_nk and kin).
const void *gs_tb_op_kernel_strict(int k, int fast, int cpl, int wg, int rule = 0);
// ... and of the quiet entries (gs_step_tb_dx_qk: GsQuiet) for k = 2, 3, 4 fused steps; nullptr otherwise.
const void *gs_tb_quiet_kernel_strict(int k);
// (The map, mask and noise units' entry queries, gs_tb_{map,mask,noise}_kernel_<flavour>, are declared per flavour in
// gs_step_flavour.h.)

// Opt-in for more than 64 KB of dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize) of kernel entry `fn` on the current
// device, made once per (device, function) and size: what every launcher with dynamic LDS calls first (gs_dyn_lds.cpp).
hipError_t gs_ensure_dyn_lds(const void *fn, size_t bytes);

// Plane utilities (math-agnostic, defined once in gs_util_kernels.hip).
hipError_t gs_launch_colormap(const float *row0, int32_t pitch, int32_t rows, int32_t cols, float scale,
                              const uint8_t *palette, int32_t n, uint8_t *rgb, hipStream_t s);
hipError_t gs_launch_fill_rect(float *row0, int32_t pitch, int32_t r0, int32_t r1, int32_t c0,
                               int32_t c1, float value, hipStream_t s);
// rows x cols of a plane (row pitch `pitch` floats) to a dense array: gs_field_download_async's staging copy.
hipError_t gs_launch_pack_rows(const float *row0, int32_t pitch, int32_t rows, int32_t cols, float *dst, hipStream_t s);
// Reduced result images (gs_reduce.hip; include/gs_hip.h: gs_field_download_reduced): rows x cols of a plane averaged over
// f x f blocks (2 <= f <= 64, blocks anchored at row 0 and column 0, edge blocks over the cells that exist) into the dense
// [ceil(rows / f), ceil(cols / f)] array `dst`, in the header's fold order.
hipError_t gs_launch_reduce(const float *row0, int32_t pitch, int32_t rows, int32_t cols, int32_t f, float *dst, hipStream_t s);
// gs_fields_place's probe: reads `bytes` (a multiple of 16, 16-byte aligned) of x and of y and writes them back unchanged.
hipError_t gs_launch_pair_probe(void *x, void *y, size_t bytes, hipStream_t s);
// gs_ctx_set_mask: the link words (gs_cell.h: link_bit) of one slab's rows [0, rows) x columns [0, cols) from the mask
// plane `mask` (a wall: != 0.0f, NaN included), whose ghost rows hold the neighbouring slabs' rows where `top` / `bottom`
// (a slab above / below exists); `periodic`: neighbours outside the grid wrap (single slab), else they are no walls.
// Only those cells are written (the caller zeroes the rest of the plane).
hipError_t gs_launch_mask_links(const float *mask, uint32_t *link, int32_t pitch, int32_t rows, int32_t cols, int32_t top,
                                int32_t bottom, int32_t periodic, hipStream_t s);
// Species::new's pattern in every member of dense [members, rows, cols] planes: U = 1, V = 0, and U = 0, V = 1 in
// rows [r0, r1) x columns [c0, c1).
hipError_t gs_launch_ens_seed(float *u, float *v, uint64_t members, int32_t rows, int32_t cols, int32_t r0, int32_t r1,
                              int32_t c0, int32_t c1, hipStream_t s);
// gs_members_mirror_k: U and V of the `n` members list[0 .. n) (device list of member indices) of dense [members, cells]
// planes copied from (src_u, src_v) to (dst_u, dst_v) -- the two slots of an ensemble -- in launches over (listed member,
// chunk); 16 bytes per lane when cells % 4 == 0 (every member then starts on a 16-byte boundary), else a dword each.
hipError_t gs_launch_members_mirror(const uint32_t *list, uint64_t n, const float *src_u, const float *src_v, float *dst_u,
                                    float *dst_v, uint64_t cells, hipStream_t s);

// Summaries (gs_summary.hip; include/gs_hip.h: gs_fields_summarize).  One record per (plane, row): the row partial of the
// fold order in gs_hip.h -- 64 lane accumulators over columns 256 k + 4 l + j, halved down to one -- with the row's
// minimum, maximum and count of non-finite cells.  32 bytes.
struct GsRowSummary {
    double sum, sum_sq;
    float min, max;
    uint32_t nonfinite, pad;
};
// Records of rows [0, rows) of n (1..4) planes that share a row pitch of `pitch` floats (rows may be 64-bit: the dense
// [members x rows, cols] layout of an ensemble is one tall plane): out[p * rows + r] for plane p, row r.
hipError_t gs_launch_row_summary(const float *const *planes, int n, int64_t pitch, int64_t rows, int32_t cols,
                                 GsRowSummary *out, hipStream_t s);
// The field fold of gs_hip.h over the records gs_launch_row_summary wrote for the two species of `count` ensemble members
// of `rows` rows each (rec[s * count * rows + i * rows + r]): out[2 i + s], the rows added one after the other in order.
hipError_t gs_launch_summary_fold(const GsRowSummary *rec, int64_t count, int64_t rows, GsRowSummary *out, hipStream_t s);

// Histograms (gs_histogram.hip; include/gs_hip.h: gs_fields_histogram).  np (1..4) planes of one shape -- rows [0, rows) of
// `pitch` floats, `cols` columns -- repeated `repeat` times `stride` floats apart (ensembles: np = 2, a member's cells;
// else repeat = 1): plane y = r * np + i is planes[i] + r * stride and is counted by the rule of gs_hip.h with lo[i], hi[i],
// scale[i] into out[y * (bins + 3) ...]: counts[bins], below, above, nan.  `out` must hold zeros (the kernel adds to it);
// max_groups: workgroups the launch may use when the planes offer more work than that (some multiple of the CU count).
hipError_t gs_launch_histogram(const float *const *planes, int np, int64_t repeat, int64_t stride, int64_t pitch, int64_t rows,
                               int32_t cols, const float *lo, const float *hi, const float *scale, int32_t bins,
                               int64_t max_groups, unsigned long long *out, hipStream_t s);

// Two planes compared (gs_change.hip; include/gs_hip.h: gs_fields_compare).  One record per (pair, row): the row partials of
// sum |d| and sum d * d, d = (double)a - (double)b over the cells where both are finite, in the summaries' fold order, with
// the row's largest |d|, the count of cells whose 32 bits differ (all cells) and of cells where a or b is not finite.  32 bytes.
struct GsRowChange {
    double sum_abs, sum_sq, max_abs;
    uint32_t differing, nonfinite;
};
// The fold of a member's row records: gs_change's layout (40 bytes).
struct GsChangeTotal {
    double sum_abs, sum_sq, max_abs;
    uint64_t differing, nonfinite;
};
// Records of rows [0, rows) of n (1..4) pairs (a[p], b[p]) of planes that share a row pitch of `pitch` floats (rows may be
// 64-bit, as for gs_launch_row_summary): out[p * rows + r] for pair p, row r.
hipError_t gs_launch_row_change(const float *const *a, const float *const *b, int n, int64_t pitch, int64_t rows, int32_t cols,
                                GsRowChange *out, hipStream_t s);
// The field fold of gs_hip.h over the records gs_launch_row_change wrote for the two species of `count` ensemble members of
// `rows` rows each (rec[s * count * rows + i * rows + r]): out[2 i + s], the rows added one after the other in order.
hipError_t gs_launch_change_fold(const GsRowChange *rec, int64_t count, int64_t rows, GsChangeTotal *out, hipStream_t s);

// Bit-quad counts (gs_morphology.hip; include/gs_hip.h: gs_fields_morphology).  np (1..4) planes of one shape -- rows [0, rows)
// of `pitch` floats, `cols` columns -- repeated `repeat` times `stride` floats apart, as for gs_launch_histogram: plane
// y = r * np + i is planes[i] + r * stride, thresholded at thresholds[i * nt + k], k < nt (1..4), with sense[i] (!= 0: a cell
// is set when it is above the threshold, 0: when it is below).  The launch counts the quad rows whose LOWER row is one of the
// plane's rows [0, rows) -- the upper row of the first of them is above[i]: `cols` floats (`pitch` readable), or unset when
// above or above[i] is null (always when repeat > 1) -- and, with `bottom`, the quad row below the last row, whose lower half
// is padding; the columns run from the padding left of column 0 to the padding right of column cols - 1.  It adds Q1, Q2, Q3,
// Q4, QD to out[(y * nt + k) * 5 ...], which must hold zeros; Q0 is the complement.  max_groups: as for gs_launch_histogram.
hipError_t gs_launch_quads(const float *const *planes, const float *const *above, int np, int64_t repeat, int64_t stride,
                           int64_t pitch, int64_t rows, int32_t cols, int bottom, const float *thresholds, const int32_t *sense,
                           int32_t nt, int64_t max_groups, unsigned long long *out, hipStream_t s);

// Regional observables (gs_regions.hip; include/gs_hip.h: gs_fields_region_summaries, gs_fields_region_morphology).  n (1..4)
// planes of one shape -- rows [0, rows) of `pitch` floats, `cols` columns -- cut into regions of rh x rw cells (rw a multiple
// of 4, at least 16; rh >= 1) anchored at row 0 and column 0, ragged ones at the lower and right edge kept: rr = ceil(rows / rh)
// by rc = ceil(cols / rw) of them.
// gs_launch_region_summary writes out[(p * rr + i) * rc + j]: the whole summary of region (i, j) of plane p -- the fold order
// of gs_hip.h with columns counted from the region's first column, its rows added in ascending order from +0.0.
// A region's record is gs_summary's layout, 32 bytes: a region's count of non-finite cells is 64-bit, as a plane's is.
struct GsRegionSummary {
    double sum, sum_sq;
    float min, max;
    uint64_t nonfinite;
};
// gs_launch_region_quads adds Q1, Q2, Q3, Q4, QD of region (i, j) of plane p, padded with its own ring of unset cells and
// thresholded as for gs_launch_quads, to out[(((p * rr + i) * rc + j) * nt + k) * 6 + 1 ...], which must hold zeros: a
// result is gs_morphology's six words, so that it travels to the caller's memory as it is, and word 0 (Q0, the complement)
// is the host's.  max_groups: as for gs_launch_histogram.
hipError_t gs_launch_region_summary(const float *const *planes, int n, int64_t pitch, int64_t rows, int32_t cols, int32_t rh,
                                    int32_t rw, GsRegionSummary *out, hipStream_t s);
hipError_t gs_launch_region_quads(const float *const *planes, int np, int64_t pitch, int64_t rows, int32_t cols, int32_t rh,
                                  int32_t rw, const float *thresholds, const int32_t *sense, int32_t nt, int64_t max_groups,
                                  unsigned long long *out, hipStream_t s);

// Two-point pair counts (gs_correlation.hip; include/gs_hip.h: gs_fields_correlation).  Planes, thresholds and senses as for
// gs_launch_quads.  The launch counts, for every lag d = 0 .. max_lag (1..64) and the unit steps e_0 = (0, 1), e_1 = (1, 0),
// e_2 = (1, 1), e_3 = (1, -1), the pairs {p, p + d e_k} of set cells whose LOWER cell lies in the plane's rows [0, rows) -- the
// upper cell may lie in one of the `nabove` rows above row 0, which above[i] holds `pitch` floats apart, the farthest first;
// with above or above[i] null or nabove == 0 (always when repeat > 1) nothing above row 0 is set -- and adds them to
// out[((y * nt + j) * 4 + k) * (max_lag + 1) + d], which must hold zeros.  Pairs never wrap.  max_groups: as for
// gs_launch_histogram.
hipError_t gs_launch_pairs(const float *const *planes, const float *const *above, int32_t nabove, int np, int64_t repeat,
                           int64_t stride, int64_t pitch, int64_t rows, int32_t cols, const float *thresholds,
                           const int32_t *sense, int32_t nt, int32_t max_lag, int64_t max_groups, unsigned long long *out,
                           hipStream_t s);

// Regional two-point pair counts (gs_region_pairs.hip; include/gs_hip.h: gs_fields_region_correlation).  Planes and regions
// as for gs_launch_region_quads (no alignment is assumed), thresholds, senses and max_lag as for gs_launch_pairs.  The launch
// adds the pairs of set cells that lie in ONE region -- nothing is above a region's first row or beside its columns -- to
// out[((((p * rr + i) * rc + j) * nt + t) * 4 + k) * (max_lag + 1) + d], which must hold zeros.
hipError_t gs_launch_region_pairs(const float *const *planes, int np, int64_t pitch, int64_t rows, int32_t cols, int32_t rh,
                                  int32_t rw, const float *thresholds, const int32_t *sense, int32_t nt, int32_t max_lag,
                                  int64_t max_groups, unsigned long long *out, hipStream_t s);

// Regional histograms (gs_region_hist.hip; include/gs_hip.h: gs_fields_region_histogram).  Planes of one slab and regions as
// for gs_launch_region_quads; lo, hi, scale per plane and bins as for gs_launch_histogram.  The launch adds the cells of region
// (i, j) of plane p, by the rule of gs_hip.h, to out[((p * rr + i) * rc + j) * (bins + 3) ...]: counts[bins], below, above,
// nan.  `out` must hold zeros.  max_groups: as for gs_launch_histogram.
hipError_t gs_launch_region_hist(const float *const *planes, int np, int64_t pitch, int64_t rows, int32_t cols, int32_t rh,
                                 int32_t rw, const float *lo, const float *hi, const float *scale, int32_t bins,
                                 int64_t max_groups, unsigned long long *out, hipStream_t s);

// Regional state comparison (gs_region_change.hip; include/gs_hip.h: gs_fields_region_compare).  n (1..4) pairs (a[p], b[p])
// of planes of one slab, all 16-byte aligned with a pitch that is a multiple of 4, and regions as for
// gs_launch_region_summary.  The launch leaves out[(p * rr + i) * rc + j]: the whole change of region (i, j) of pair p -- d as
// gs_launch_row_change forms it, the fold order of gs_hip.h with columns counted from the region's first column, the region's
// rows added in ascending order from +0.0.  With `records` null a wave takes a whole region (the wave route; `out` needs no
// initial contents); else `out` must hold zeros and `records` gs_region_change_record_bytes(...) bytes: the kernel leaves a
// 16-byte record per (pair, row, region column) there and a second launch folds them (the record route).  The bits are the
// same.  gs_region_change_wants_records: the library's choice between the two -- the record route where the region is at
// least two bands high and the wave route's waves (rows of the region grid x groups of regions side by side in 256 columns)
// number fewer than kRegionChangeWavesPerCu per compute unit.
constexpr int kRegionChangeUnroll = 4;      // rows (narrow regions) or chunks of 256 columns (wide ones) of BOTH planes loaded before the adds
constexpr int kRegionChangeBand = 16;       // rows of a unit of the record route
constexpr int kRegionChangeWavesPerCu = 4;  // a wave on each of a CU's 4 SIMDs: from there on the wave route is the faster one (profiles/region_change.md)
bool gs_region_change_wants_records(int64_t rows, int32_t cols, int32_t rh, int32_t rw, int cu_count);
size_t gs_region_change_record_bytes(int n, int64_t rows, int32_t cols, int32_t rw);
hipError_t gs_launch_region_change(const float *const *a, const float *const *b, int n, int64_t pitch, int64_t rows, int32_t cols,
                                   int32_t rh, int32_t rw, GsChangeTotal *out, void *records, hipStream_t s);

// Power spectra (gs_spectrum.hip; include/gs_hip.h: gs_fields_spectrum).  np (1..4) planes of one shape repeated `repeat` times
// `stride` floats apart (gs_plane_scan.h's set), tiles of `tile` (16, 32, 64, 128) cells a side anchored at row 0 and column
// 0, `window` != 0: the window h[tile] is applied; w: the tile / 2 twiddles as (re, im) pairs.  The launches -- a workgroup
// per segment of 16 tiles writes a record into `records` (gs_spectrum_record_bytes(...) bytes, no initial contents), a fold
// adds a band's records -- leave out[plane * ceil(rows / tile) + band]: a result of gs_spectrum_result_bytes(tile) bytes, the
// band's tile (tile / 2 + 1) f64 sums and the tiles {used, skipped} as u64; zeros for the band of the rows below the last
// whole one.
constexpr size_t gs_spectrum_result_bytes(int32_t tile) { return ((size_t)tile * (size_t)(tile / 2 + 1) + 2) * 8; }
size_t gs_spectrum_record_bytes(int64_t planes, int64_t rows, int32_t cols, int32_t tile);
hipError_t gs_launch_spectrum(const float *const *planes, int np, int64_t repeat, int64_t stride, int64_t pitch, int64_t rows,
                              int32_t cols, int32_t tile, int32_t window, const float *h, const float *w, void *records,
                              void *out, hipStream_t s);

// Regional power spectra (gs_region_spectrum.hip; include/gs_hip.h: gs_fields_region_spectrum).  np (1..4) planes of one slab
// and regions of rh x rw cells as for gs_launch_region_quads, tile, window, h and w as for gs_launch_spectrum; tiles are
// anchored at every region's first row and column.  The launches -- a workgroup per segment of 16 tiles of a band of a region
// writes a record into `records` (np * gs_region_spectrum_records(rows, cols, ...) * gs_spectrum_result_bytes(tile) bytes, no
// initial contents), a fold adds a region's records -- leave out[(p * rr + i) * rc + j], a result of
// gs_spectrum_result_bytes(tile) bytes for every region of the slab: zeros where no tile fits.
// gs_region_spectrum_records: the records of one plane of rows x cols cells -- over its regions, bands of the region times
// segments of such a band.  A region grid's rows split at multiples of rh add up: the slabs' counts sum to the grid's.
uint64_t gs_region_spectrum_records(uint64_t rows, uint64_t cols, int32_t rh, int32_t rw, int32_t tile);
hipError_t gs_launch_region_spectrum(const float *const *planes, int np, int64_t pitch, int64_t rows, int32_t cols, int32_t rh,
                                     int32_t rw, int32_t tile, int32_t window, const float *h, const float *w, void *records,
                                     void *out, hipStream_t s);

// Connected components (gs_components.hip; include/gs_hip.h: gs_fields_components).  `planes` planes of rows x cols cells,
// `stride` floats apart, rows `pitch` floats apart, thresholded at `threshold` with `sense` as for gs_launch_quads and
// labelled under `connectivity` (4 or 8); a component never leaves its plane.  parent and size hold one u32 per cell of all
// planes, planes * rows * cols < 2^32, and need no initial contents.  The launches -- tile, border, flatten, tally, each its
// own, none waiting for another workgroup -- add every plane's counters, in gs_components' layout (35 u64), to
// out[y * 35 ...], which must hold zeros.  With `seams` (planes == 1): 4 * cols u32 -- the first row's roots, the sizes of
// those roots, the last row's roots and their sizes; 0xffffffff and 0 for an unset cell.  max_groups: as for
// gs_launch_histogram.
constexpr int kCompTileRows = 16, kCompTileCols = 256;
hipError_t gs_launch_components(const float *plane, int64_t planes, int64_t stride, int64_t pitch, int64_t rows, int32_t cols,
                                float threshold, int32_t sense, int32_t connectivity, int64_t max_groups, uint32_t *parent,
                                uint32_t *size, unsigned long long *out, uint32_t *seams, hipStream_t s);
// The tile, border and flatten launches of gs_launch_components alone: parent[cell] = the root of the cell's component, its
// first cell in row-major order (0xffffffff: not set), size[root] = its cells.  What the component lists start from.
hipError_t gs_launch_component_labels(const float *plane, int64_t planes, int64_t stride, int64_t pitch, int64_t rows, int32_t cols,
                                      float threshold, int32_t sense, int32_t connectivity, uint32_t *parent, uint32_t *size,
                                      hipStream_t s);

// The flatten launch alone: every set entry of parent[0 .. total) gets its root, size[root] its cells (size[] holds zeros).
hipError_t gs_launch_component_flatten(uint32_t *parent, uint32_t *size, uint64_t total, hipStream_t s);

// Regional connected components (gs_region_components.hip; include/gs_hip.h: gs_fields_region_components).  One plane of one
// slab -- a field's: rows that begin on 16 bytes, a pitch that is a multiple of 4 --, rows x cols < 2^32 cells, labelled as
// gs_launch_component_labels labels it but with the borders of the regions of rh x rw cells (rw a multiple of 4) as walls;
// every component then adds itself to the 35 counters of the region (i, j) it lies in, at out[(i * rc + j) * region_words
// ...], which must hold zeros (rc = ceil(cols / rw); region_words >= 35: the results of several thresholds lie side by side).
// parent, size and max_groups: as for gs_launch_components.
hipError_t gs_launch_region_components(const float *plane, int64_t pitch, int64_t rows, int32_t cols, int32_t rh, int32_t rw,
                                       float threshold, int32_t sense, int32_t connectivity, int64_t max_groups,
                                       uint32_t *parent, uint32_t *size, int64_t region_words, unsigned long long *out,
                                       hipStream_t s);

// Component lists (gs_component_list.hip; include/gs_hip.h: gs_field_component_list), behind gs_launch_component_labels on the
// same stream.  A record is gs_component_record's layout; first_row counts over all planes (plane * rows + row), the sums and
// the box are the plane's own rows.  A component is listed if it has at least min_size cells or, with `open` (planes == 1: a
// slab of a chain), touches the first or last row.
struct GsComponentRecord {
    uint64_t size, sum_row, sum_col;
    uint32_t first_row, first_col, row_min, row_max, col_min, col_max;
};
struct GsListWork {
    uint32_t *open;     // ceil(entries / 32) words, or null
    uint32_t *counts;   // gs_list_groups(entries) words
    uint32_t *selected; // one word: the number of records
};
uint64_t gs_list_groups(uint64_t entries);
// count: leaves *selected.  fill (records: *selected of them, at least one): writes the records in ascending order of their
// first cell, adds every listed cell to its record and, with `seams`, leaves 2 * cols u32: the record index of every cell of
// the first row, then of the last (0xffffffff: not set).  size[] holds record indices afterwards.
hipError_t gs_launch_list_count(const uint32_t *parent, uint32_t *size, int64_t planes, int64_t rows, int32_t cols, uint64_t min_size,
                                const GsListWork &w, hipStream_t s);
hipError_t gs_launch_list_fill(const uint32_t *parent, uint32_t *size, int64_t planes, int64_t rows, int32_t cols, uint64_t min_size,
                               const GsListWork &w, GsComponentRecord *records, uint32_t *seams, hipStream_t s);

// Component matching (gs_match.hip; include/gs_hip.h: gs_fields_match).  gs_launch_piece_labels (gs_components.hip) labels the
// cells that are set in BOTH of two label arrays -- the parent arrays of two labellings of planes of one shape, dense entries,
// 0xffffffff for an unset cell -- exactly as gs_launch_component_labels labels a thresholded plane: the tile kernel reads the
// two arrays in place of a plane, border and flatten run as they are.  gs_launch_match_pairs, behind the pieces' count and
// scan (gs_launch_list_count with min_size 1, which leaves `counts`) and behind both lists' fill (index_*[root] = the root's
// record index, 0xffffffff: not listed), writes one overlap per piece, in ascending order of the pieces' first cells:
// (before, after) = the record indices of the two components the piece lies in, both 0xffffffff where either is not listed.
struct GsMatchOverlap { // gs_component_overlap's layout
    uint32_t before, after;
    uint64_t cells;
};
hipError_t gs_launch_piece_labels(const uint32_t *both_b, const uint32_t *both_a, int64_t planes, int64_t rows, int32_t cols,
                                  int32_t connectivity, uint32_t *parent, uint32_t *size, hipStream_t s);
hipError_t gs_launch_match_pairs(const uint32_t *parent_b, const uint32_t *index_b, const uint32_t *parent_a, const uint32_t *index_a,
                                 const uint32_t *parent_p, const uint32_t *size_p, const uint32_t *counts, int64_t planes,
                                 int64_t rows, int32_t cols, GsMatchOverlap *overlaps, hipStream_t s);

// Time statistics (gs_time_stats.hip; include/gs_hip.h: gs_time_stats_accumulate).  Per-cell accumulators over the samples of
// np (1..4) planes of one shape -- rows [0, rows) of `pitch` floats, `cols` columns: plane y's are `plane_stride` elements
// behind plane y - 1's in each accumulator array, rows of the planes' own pitch, no ghost rows.  An array whose group
// (GS_TSTAT_SUM, _SQUARES, _EXTREMES, _CROSSINGS of gs_hip.h) is not selected is null and never touched.  t / flip: the set
// rule of gs_plane_scan.h per plane.
struct GsTstatAcc {
    double *sum, *squares;
    float *mn, *mx;
    uint32_t *set_count, *first_stamp;
    int64_t plane_stride;
};
// One sample of every plane added (rows may be 64-bit: an ensemble's members are one tall plane per species); at most
// `max_groups` workgroups.
hipError_t gs_launch_tstat_accumulate(const float *const *planes, int np, int64_t pitch, int64_t rows, int32_t cols, uint32_t groups,
                                      const GsTstatAcc &acc, const float *t, const uint32_t *flip, uint32_t stamp,
                                      int64_t max_groups, hipStream_t s);
// The selected accumulators of np planes back to their reset values.
hipError_t gs_launch_tstat_reset(int np, uint32_t groups, const GsTstatAcc &acc, hipStream_t s);
// One result plane (`which`: GS_TSTAT_MEAN .. GS_TSTAT_ARRIVAL) of plane `plane` after n samples into out, rows of `pitch` floats.
hipError_t gs_launch_tstat_result(int which, int plane, const GsTstatAcc &acc, int64_t pitch, int64_t rows, int32_t cols, uint64_t n,
                                  float *out, hipStream_t s);

// ---- statistics across the members of a bundle (gs_bundle_stats.hip) ------------------------------------------------------
// `bundles` bundles of `span` consecutive dense members of `cells` floats each, U from in[0] and V from in[1] (the first
// bundle's first member): result plane w (GS_TSTAT_MEAN .. GS_TSTAT_OCCUPANCY) of bundle b of species sp goes to
// out[sp][w] + b * cells where out[sp][w] is not null (the same w for both species).  t / flip: the set rule of
// gs_plane_scan.h per species, read for the occupancy alone.  One launch per 65535 bundles.
hipError_t gs_launch_bundle_stats(const float *const in[2], float *const out[2][5], int64_t cells, int64_t span, int64_t bundles,
                                  const float t[2], const uint32_t flip[2], hipStream_t s);
