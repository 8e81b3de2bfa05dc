/*
 * gs_hip.h -- C ABI of the MI355X-native Gray-Scott compute backend (libgs_hip.so).
 *
 * This is the drop-in boundary for ONE path of HadrienG2/grayscott: the per-timestep
 * 9-point Laplacian + u*v^2 reaction update that every compute backend of the reference
 * implements behind
 *     SimulateBase / SimulateCreate / Simulate      compute/shared/src/lib.rs:19-58
 *     Concentration / Species                       data/src/concentration/mod.rs:17-296
 * Results follow the reference's *naive* backend (compute/naive/src/lib.rs:42-83) bit for
 * bit, including its clipped-window boundary rule and FTZ-without-DAZ denormal handling.
 *
 * The reference is Rust; a backend crate binds these entry points through `extern "C"`
 * (rust/compute_hip/src/ffi.rs, shown in INTEGRATION.md).  Plain pointers, sizes and
 * integer status codes only: no C++ / torch / HIP types cross this boundary.
 *
 * Conventions
 *   - Every function returns GS_OK (0) or a negative gs_status; gs_last_error() returns a
 *     thread-local, human-readable message for the last failure on the calling thread.
 *     No exceptions, aborts or panics cross the ABI.  (The reference's error contract:
 *     `type Error: Error + From<C::Error> + Send + Sync`, compute/shared/src/lib.rs:31.)
 *   - Handles are created and destroyed by the caller.  The library never keeps a host
 *     pointer past the call that received it.
 *   - Calls on one gs_ctx must be externally serialised (the reference takes
 *     `&mut Species` in perform_steps); a context may be moved between threads: every
 *     entry point selects its own device(s).
 *   - gs_step / gs_run only enqueue work; gs_sync (or a download) waits for it.  A host-side
 *     Simulate::perform_steps is gs_run + gs_sync (every backend of the reference returns from
 *     perform_steps with the steps done: compute/shared/src/gpu/mod.rs:77-91); gs_run alone is
 *     the asynchronous SimulateGpu::prepare_steps (:70-75).
 *   - Shapes are [rows, cols] in scalar units, as in Concentration::shape()
 *     (data/src/concentration/mod.rs:191-221).  Storage is row-major f32 (`Precision`,
 *     data/src/lib.rs:11).
 *
 * Domain decomposition
 *   A context owns `n_local` row slabs (one per entry of device_ids; ids may repeat) which
 *   together cover the rows of this process; `world` processes (one per GPU when launched
 *   under torchrun) cover the global grid in rank order.  Slabs keep 4 ghost rows above and
 *   below; a pass that fuses K <= 4 time steps updates the K boundary rows of each side
 *   first and pushes them to the neighbouring slab's ghost rows -- by a device-to-device copy
 *   inside a process, by RCCL ncclSend/ncclRecv between processes -- on a side stream,
 *   overlapped with the interior update.  The reference has no multi-device code; its
 *   in-process precedent is SimulateCpu::split_grid (compute/shared/src/cpu.rs:111-154).
 *
 * Environment
 *   The library itself reads these variables (the host mirrors add one per gs_options field, GS_HIP_<FIELD>, as the
 *   reference's CliArgs do with clap's `env`).  None of them changes results: every combination is bit-identical.
 *     GS_RCCL_LIBRARY       library to bind instead of librccl (a custom RCCL build; the tests' shared-memory
 *                           transport double).  An explicit choice never falls back to the system's librccl.
 *     GS_HIP_TRACE_LAUNCH   1 = print the first 64 kernel launches (label, row ranges, layout) on stderr
 *     GS_HIP_TRACE_TUNER    1 = print every timing window of gs_run's on-line tuner and what it chose, and every probe
 *                           of gs_fields_place
 *   Launch-policy switches for A/B timing (defaults are the measured best; grayscott_amd/csrc/gs_experiments.h):
 *     GS_HIP_PLACE_ALL      1 = gs_fields_place draws all its candidates even when two fast pairs are found before
 *     GS_HIP_PLACE_DEEP     0 = gs_fields_place never draws more than `candidates` blocks (default: up to 4 x as many while more
 *                           than half of the device's memory is free)
 *     GS_HIP_PLACE_FORCE    "a,b,c,d" = test hook: gs_fields_place draws its candidates and moves the planes to blocks a, b, c, d
 *                           of those it holds (0-3 the planes' own, 4 and up drawn), without probes
 *     GS_HIP_EDGE_KINDS     0 = edge units of the marching kernel all take the general path
 *     GS_HIP_EDGE_SPLIT     0 / 1 = never / always dispatch edge units as two half-height units
 *     GS_HIP_QUIET_UNITS    0 = units of the marching kernel at rest are recomputed like any other (default 1: gs_run's full
 *                           passes skip them where the call is eligible, gs_ctx_quiet_stats); read by gs_ctx_create
 *     GS_HIP_FAIR           0 / 1 = never / always run one-round launches as in-step 16-wave workgroups
 *     GS_HIP_FAIR_FROM      progress (0 ... 256) from which the in-step form steers wave priorities
 *     GS_HIP_XCD_M          0 = plain workgroup order, n = XCD-aware renumbering in groups of 8 n workgroups
 *     GS_HIP_XCD_M_STREAM   the same for the single-step kernel
 *     GS_HIP_TILE_LDS_FLOOR least dynamic LDS (bytes) of the LDS-window kernel: limits its workgroups per CU
 *     GS_HIP_WINDOW_PATIENCE polls (2-3 us each) a wave of the persistent window kernel waits for its neighbours' cells
 *                           before the launch gives up (default 2^20: 2-3 s)
 *     GS_HIP_WINDOW_WAVES   "left,interior,right": waves in use (of 16) in the windows of the grid's left-most, inner
 *                           and right-most tile column (default 12,16,12 under the clipped rule, 16,16,16 otherwise)
 */
#ifndef GS_HIP_H
#define GS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 4

typedef enum gs_status {
    GS_OK = 0,
    GS_ERR_INVALID = -1,     /* bad argument / shape mismatch (the reference panics: mod.rs:291-295) */
    GS_ERR_HIP = -2,         /* a HIP runtime call failed                                  */
    GS_ERR_RCCL = -3,        /* librccl could not be loaded or an RCCL call failed         */
    GS_ERR_NO_DEVICE = -4,   /* no usable gfx950 device                                    */
    GS_ERR_UNSUPPORTED = -5, /* request outside what this build implements                 */
    GS_ERR_NOMEM = -6
} gs_status;

/* Parameters (data/src/parameters.rs:13-33): stencil weights row-major + the five rates. */
typedef struct gs_params {
    float w[3][3];
    float du;   /* diffusion_rate_u */
    float dv;   /* diffusion_rate_v */
    float feed; /* feed_rate        */
    float kill; /* kill_rate        */
    float dt;   /* time_step        */
} gs_params;

/* Arithmetic flavour of the step kernels.
 *   GS_MATH_STRICT  every reference operation is a separately rounded f32 op and the
 *                   kernels run with f32 denormal mode "flush results, keep inputs", which
 *                   is what MXCSR.FTZ (DenormalsFlusher, compute/shared/src/lib.rs:161-180)
 *                   does on the CPU: bit-identical to naive under FTZ, sub-normals included.
 *   GS_MATH_FUSED   the eight tap updates per species use one FMA each (exact for the
 *                   power-of-two Oono-Puri weights as long as the product is a normal
 *                   number) and denormals are kept: bit-identical to naive wherever no
 *                   intermediate is sub-normal, |diff| <= 1e-37 elsewhere.  Refused
 *                   (GS_ERR_UNSUPPORTED) for weights that are not 0 or a power of two.    */
typedef enum gs_math { GS_MATH_STRICT = 0, GS_MATH_FUSED = 1 } gs_math;

/* Which step kernel runs.  AUTO = STREAM for a single gs_step; inside gs_run, by grid size when nothing
 * is pinned: the LDS-resident whole-run kernel up to 1536 cells; WINDOW for calls of >= 32 steps on grids
 * from 0.8 M cells that one round of 80-row windows covers (one per compute unit; 8, 6, 4 or 2 steps per
 * exchange, as many as fit); TILE otherwise up to 1.5 M cells; TB with fuse_steps (default 4) otherwise, for
 * slab chains and whenever fuse_steps, rows_per_block, cols_per_lane, split or use_graph pin a schedule.
 * Under GS_BOUNDARY_PERIODIC there is no WINDOW and no LDS form: pinning either is refused at gs_ctx_create
 * (GS_ERR_UNSUPPORTED), and AUTO runs TB where it would have run WINDOW (1080 x 1920 in long calls, for one).
 * The same holds under GS_BOUNDARY_NEUMANN. */
typedef enum gs_kernel {
    GS_KERNEL_AUTO = 0,    /* best measured variant for the shape                          */
    GS_KERNEL_SIMPLE = 1,  /* one thread per cell, global loads only (cross-check kernel)  */
    GS_KERNEL_STREAM = 2,  /* register sliding window, 16-B loads, DPP halo exchange       */
    GS_KERNEL_TB = 3,      /* temporally blocked streaming kernel: fuse_steps steps / launch */
    GS_KERNEL_LDS = 4,     /* LDS-staged (tile + halo) window, one step per launch (measured
                              alternative to STREAM; never chosen by AUTO)                   */
    GS_KERNEL_TILE = 5,    /* gs_run only, single slab: up to 8 steps per launch on LDS-resident windows
                              with a K-cell apron, one cell per lane and 16 waves per window (gs_step and
                              slab chains fall back to STREAM / TB); what AUTO runs on mid-size grids  */
    GS_KERNEL_WINDOW = 6   /* gs_run only, single slab, grids of at most one register-resident window per compute unit
                              (1.5 - 2.3 M cells on 256 CUs: the reference's default 1080 x 1920 is 252 windows): the
                              whole call is ONE persistent launch; every workgroup keeps its window (72 x 120 owned
                              cells + a k-cell apron; lower windows on the grid's left and right edge, whose cells cost
                              more) in registers and trades its apron with its neighbours every k steps through
                              exchange planes, flags and sc1 accesses (fuse_steps = k: 2, 4, 6 or 8; rows_per_block =
                              full window rows: 80).  What AUTO runs for calls of >= 32 steps where such windows cover the
                              grid: 496 k against TB's 395 k Mcells x steps / s at 1080 x 1920 in 1000-step calls; in
                              32-step calls the two tie (profiles/r05_window_kernel.md).
                              A launch whose workgroups are not all resident (another long-running kernel holds CUs)
                              gives up after a bounded wait: the launches before it stand, it and the later ones are run
                              again with TB by the next call that waits for or reads results (each from its own input
                              planes, which no launch writes), and the context stays with TB  */
} gs_kernel;

/* Rule on the edges of the global grid.  The reference has the first two:
 * CLIPPED   -- compute_naive's, the parity target: the 3x3 window is clipped to the grid and the
 *              weights are indexed from the clipped window's top-left corner
 *              (compute/naive/src/lib.rs:57-71);
 * ZERO_HALO -- the Vulkan and SIMD backends': full window, weights centred, cells outside the grid
 *              read as 0 (compute/gpu/naive/src/pipeline.rs:105-113, main.comp:37-44;
 *              data/src/concentration/simd/mod.rs:281-326), here with naive's operation order.
 * PERIODIC  -- the grid wraps around (a torus), the usual setting of Gray-Scott studies: every cell takes the nine
 *              taps of ZERO_HALO's interior cell, in its order, with neighbour (r + i - 1, c + j - 1) read at
 *              ((r + i - 1) mod rows, (c + j - 1) mod cols) -- on 1 x N, N x 1 or 2 x 2 grids a neighbour can be
 *              the cell itself.  Single slab in a single process only: a context of several slabs or processes,
 *              a pinned GS_KERNEL_WINDOW or GS_KERNEL_LDS and split > 1 are refused at gs_ctx_create
 *              (GS_ERR_UNSUPPORTED).
 * NEUMANN   -- zero flux through the edges, the closed domain of most reaction-diffusion work on a finite grid:
 *              every cell takes the nine taps of ZERO_HALO's interior cell, in its order, with neighbour
 *              (r + i - 1, c + j - 1) read at (clamp(r + i - 1, 0, rows - 1), clamp(c + j - 1, 0, cols - 1)), the
 *              nearest cell inside the grid (np.pad(x, 1, mode="edge")); on 1 x N, N x 1 or 1 x 1 grids a neighbour
 *              can be the cell itself.  With F = k = 0 the sum of U + V is conserved up to rounding.  Only the global
 *              edges change, so any slab count, process count and split is accepted; a pinned GS_KERNEL_WINDOW or
 *              GS_KERNEL_LDS is refused at gs_ctx_create (GS_ERR_UNSUPPORTED). */
enum gs_boundary { GS_BOUNDARY_CLIPPED = 0, GS_BOUNDARY_ZERO_HALO = 1, GS_BOUNDARY_PERIODIC = 2, GS_BOUNDARY_NEUMANN = 3 };

/* Backend options: the C view of the Rust `CliArgs` (compute/shared/src/lib.rs:20-25 --
 * every field has a default; zero-initialise and override). */
typedef struct gs_options {
    int32_t math;            /* gs_math; default STRICT                                    */
    int32_t kernel;          /* gs_kernel; default AUTO                                    */
    int32_t rows_per_block;  /* rows each wave marches over (0 = auto)                     */
    int32_t fuse_steps;      /* steps fused per launch in gs_run (1..4; 0 = auto); single slab */
    int32_t use_graph;       /* 1 = gs_run replays batches of 16 passes through a hipGraph: one host-side *
                              * launch per batch (single slab, no row bands; 0 = off)                   */
    int32_t pitch_pad;       /* extra f32 of row pitch beyond the 64-float round-up        */
    int32_t split;           /* row bands a single slab is scheduled as (0 or 1 = off): adjacent  *
                              * bands only depend on each other's K boundary rows, so the tail *
                              * of one pass overlaps the start of the next.  Opt-in: the gain  *
                              * (up to +3 % at 16384^2) is not stable from box to box          */
    int32_t general_kernels; /* 1 = never use the kernel variants specialised for the default  *
                              * side weights (0.5) / dt == 1; results are bit-identical either *
                              * way, the switch exists for A/B timing and tests                */
    int32_t cols_per_lane;   /* columns per lane of the temporally blocked kernel: 4 (wide, for  *
                              * large grids), 2 or 1 (more, narrower waves for small grids);   *
                              * 0 = chosen on line by gs_run                                   */
    int32_t boundary;        /* gs_boundary; default CLIPPED                                     */
    int32_t no_tune;         /* 1 = gs_run never times candidate configurations: it runs the pinned *
                              * values above, a configuration set with gs_ctx_set_tuned, or the     *
                              * untuned defaults                                                   */
    int32_t tile_shape;      /* GS_KERNEL_TILE: window of a workgroup, 1 = 32 rows x 64 columns, 2 = 16 x 64,       *
                              * 3 = 64 x 64; 0 = 32 x 64.  With kernel = TILE, fuse_steps (1..8, and less than  *
                              * half the window's rows) sets the steps per launch                          */
    int32_t share_taps;      /* full difference sharing in the temporally blocked kernel (the S / SE / SW taps of a  *
                              * row are, negated, the N / NW / NE taps of the next: 46 instead of 52 arithmetic    *
                              * instructions per cell-step, bit-identical; needs side weights 0.5, dt == 1 and      *
                              * w[0][0] == w[2][2], w[0][2] == w[2][0] -- true of every stencil of the reference):  *
                              * 0 = on (form 3) unless gs_run's on-line tuner measures the chosen configuration   *
                              * faster without, 1 = on, WITHIN a lane only (46 instructions per cell-step; the halo  *
                              * columns of a lane's two go through an LDS board), 2 = off, 3 = on and ACROSS lanes   *
                              * too (the three differences that cross a lane boundary are formed by one of the two  *
                              * lanes and read by the other as DPP operands: 41 instructions per cell-step, half the *
                              * LDS traffic; 3-5 % less energy per cell-step than form 1 on every input)             */
    int32_t reserved[3];
} gs_options;

typedef struct gs_ctx gs_ctx;     /* devices, streams, row partition, RCCL communicator    */
typedef struct gs_field gs_field; /* one f32 plane [rows, cols], slab-distributed           */

/* Parameters::default() (parameters.rs:72-83) with the Oono-Puri weights (:116-122). */
void gs_default_params(gs_params *out);
void gs_default_options(gs_options *out);

int32_t gs_abi_version(void);
const char *gs_last_error(void);
int32_t gs_device_count(int32_t *out);

/* 128-byte RCCL unique id, created on rank 0 and handed to every rank out of band. */
#define GS_UNIQUE_ID_BYTES 128
int32_t gs_get_unique_id(void *out128);

/* Is RCCL usable from this process?  Loads the library exactly as a multi-process context does (GS_RCCL_LIBRARY,
 * else librccl), creates a ONE-rank communicator on `device` and moves a message of `floats` f32 to itself with the
 * call pattern of the ghost-row exchange (one group: ncclSend + ncclRecv, on a high-priority stream), then compares
 * it.  For a maintainer's first multi-GPU run; no context is needed. */
int32_t gs_rccl_selftest(int32_t device, uint64_t floats);

/* Which libraries this process's libgs_hip.so is bound to, as one JSON object: {"hip": path of the HIP runtime,
 * "hip_runtime_version", "rccl": path or null, "rccl_version", "rccl_named_by_GS_RCCL_LIBRARY"}.  libgs_hip.so links
 * the HIP runtime by SONAME (libamdhip64.so.7) and dlopens RCCL by SONAME (librccl.so.1) on first use, so it binds
 * WHATEVER COPY THE PROCESS HAS MAPPED FIRST: in a process that imported torch before creating a context -- bench.py,
 * the tests -- both are the copies the torch wheel bundles (one HIP runtime in the process, the one that owns
 * the planes' device pointers, and the RCCL built against it, which the library's communicator then shares with
 * torch's ProcessGroupNCCL if that exists); in a torch-free process -- the Rust binary -- they are /opt/rocm's.  Both
 * pairings run the one-rank exchange of gs_rccl_selftest in the GPU suite (tests/test_gpu_multiprocess.py).
 * load_rccl = 0 reports RCCL only if this process has loaded it already (nothing is loaded for the answer). */
int32_t gs_runtime_info(int32_t load_rccl, char *out, size_t cap);

/* SimulateCreate::new(params, args) (compute/shared/src/lib.rs:42-45).
 *   device_ids / n_local : local slabs, top to bottom (NULL / 0 = one slab on device 0)
 *   rank, world          : this process's place in the row-wise chain (0, 1 = single process)
 *   unique_id            : gs_get_unique_id() bytes of rank 0; required iff world > 1      */
int32_t gs_ctx_create(gs_ctx **out, const gs_params *params, const gs_options *opts,
                      const int32_t *device_ids, int32_t n_local, int32_t rank, int32_t world,
                      const void *unique_id);
int32_t gs_ctx_destroy(gs_ctx *ctx);
int32_t gs_ctx_set_params(gs_ctx *ctx, const gs_params *params);

/* Parameter map: feed and kill rates that vary from cell to cell on one grid (Munafo's (F, k) map, feed masks, gradients).
 * While a map is attached, every step of gs_step / gs_run is the reference step with feed = F[r, c] and kill = K[r, c]
 * for cell (r, c); du, dv, dt and the weights still come from gs_params, whose feed and kill are ignored.  F + K is one
 * f32 add per cell in the context's float mode (GS_MATH_STRICT flushes a sub-normal sum), and the arithmetic contract of
 * gs_math is unchanged.  Under the periodic rule a cell computed at a wrapped position takes the map at that position.
 *   feed, kill : ordinary fields of this context with the species' global shape, created and uploaded the usual way (in a
 *                multi-process run each process uploads its own rows).  The call COPIES them into two planes the library
 *                owns (F, and F + K formed on the device) and fills their ghost rows once: the caller may change or
 *                destroy its fields afterwards.  feed == kill == NULL detaches the map.
 * The call waits for enqueued work; in a multi-process run it is collective.  gs_step / gs_run on species of another
 * shape than the map's: GS_ERR_INVALID.  A context whose pinned kernel has no map form (GS_KERNEL_WINDOW, _LDS, _TILE):
 * GS_ERR_UNSUPPORTED.  With a map, gs_run runs the marching kernel at every grid size (never the resident, tile or window
 * kernel) and gs_step the streaming one; their map forms carry a "/map" suffix in gs_ctx_info (e.g.
 * "tb-k4c2/strict.op/map", "tb-k4c2/strict/periodic/map").  Graph replay and the on-line tuner keep mapped and uniform
 * runs apart: gs_ctx_get_tuned / gs_ctx_set_tuned act on the choices of the kernel set in force.  Ensembles keep their
 * own per-member parameters and ignore the map. */
int32_t gs_ctx_set_param_map(gs_ctx *ctx, gs_field *feed, gs_field *kill);

/* Domain mask: wall cells that are not part of the medium (obstacles, channels, mazes, patterns grown inside a shape).
 * Cell (r, c) is a wall when M[r, c] != 0.0f -- NaN is a wall, +-0 is fluid.  While a mask is attached, every step of
 * gs_step / gs_run is the reference step with two changes:
 *   1. a wall cell is held: its outputs are its inputs bit for bit, NaN payloads included (in fused passes at every level);
 *   2. each tap of a fluid cell reads one cell of the window as the boundary rule resolves it (the clipped rule's clipped
 *      and shifted window, the zero-halo rule's 0 outside the grid -- never a wall --, the periodic rule's wrapped cell,
 *      the zero-flux rule's clamped cell); where that cell is a wall the tap reads the centre cell's own u / v instead,
 *      so its difference is u - u.  The taps, their order and every rounding stay the reference's.
 * So no flux crosses a link into a wall, a wall's stored values never reach another cell, and with F = k = 0 under the
 * zero-flux rule the sum of U + V over the fluid cells is conserved up to rounding.  An all-fluid mask changes no bit; the
 * arithmetic contract of gs_math is unchanged.
 *   mask : an ordinary field of this context with the species' global shape (in a multi-process run each process uploads
 *          its own rows).  The call COPIES it: the library forms a plane of its own, one word per cell naming the walls
 *          among the cell's neighbours under the context's boundary rule, and fills its ghost rows once; the caller may
 *          change or destroy its field afterwards.  NULL detaches the mask; a second call replaces it.
 * The call waits for enqueued work; in a multi-process run it is collective.  gs_step / gs_run on species of another
 * shape than the mask's: GS_ERR_INVALID.  A context whose pinned kernel has no mask form (GS_KERNEL_WINDOW, _LDS, _TILE),
 * or one with a parameter map attached: GS_ERR_UNSUPPORTED (gs_ctx_set_param_map likewise refuses a masked context).
 * With a mask, gs_run runs the marching kernel at every grid size (never the resident, tile or window kernel), gs_step the
 * streaming one and a pinned GS_KERNEL_SIMPLE the simple one; their mask forms carry a "/mask" suffix in gs_ctx_info (e.g.
 * "tb-k4c2/strict.op/mask", "tb-k4c1/strict/periodic/mask") and share no differences (no ".ds" / ".dx").  Graph replay and
 * the on-line tuner keep masked runs apart from uniform and mapped ones: gs_ctx_get_tuned / gs_ctx_set_tuned act on the
 * choices of the kernel set in force.  Ensembles ignore the mask; summaries include wall cells. */
int32_t gs_ctx_set_mask(gs_ctx *ctx, gs_field *mask);

/* Noise: a seeded, bit-reproducible stochastic term of the step.  While noise is attached, every step of gs_step / gs_run
 * is the reference step followed, per cell and species, by one increment drawn from a counter-based generator: a pure
 * function of (seed, step, global row, global column), so the bits do not depend on the kernel, the fusion depth, the
 * columns per lane, the slab count or the process count.  The definition, all words u32:
 *   Philox2x32-10, M = 0xD256D193, W = 0x9E3779B9.  One round:  (hi, lo) = M * c0 (the 64-bit product);
 *     (c0, c1) <- (hi ^ k ^ c1, lo).  Ten rounds; before every round but the first, k += W.
 *     philox(0, 0, 0) = (ff1dae59, 6cd10df2);  philox(ffffffff, ffffffff, ffffffff) = (2c3f628b, ab4fd7ad);
 *     philox(243f6a88, 85a308d3, 13198a2e) = (dd7ce038, f62a4c12)                       [(c0, c1, k) -> result]
 *   step key, formed on the host for the u64 seed and the u64 step index s:
 *     key(s) = philox(c0 = (u32)s, c1 = (u32)(s >> 32), k = (u32)seed)[0] ^ (u32)(seed >> 32)
 *   cell draw at global row r, global column c in step s:  (x0, x1) = philox(c0 = c, c1 = r, k = key(s));
 *     x0 is U's draw, x1 is V's.  Under the periodic rule a cell computed at a wrapped position uses the wrapped (r, c).
 *   value:  xi(x) = ((float)(int32_t)(x >> 8) - 8388608.0f) * 0x1p-23f  -- every operation exact in f32.
 *   step:   with (nu, nv) the reference step's outputs for the cell, every operation of the contract unchanged,
 *     out_u = nu + sigma_u * xi(x0),  out_v = nv + sigma_v * xi(x1):
 *     one rounded f32 multiply and one rounded f32 add per species in the context's float mode (GS_MATH_STRICT flushes a
 *     sub-normal product or sum), never contracted in either flavour -- GS_MATH_FUSED fuses only what it fuses without
 *     noise.  A species whose sigma is 0.0f is not touched at all: its value is nu bit for bit, -0 stays -0.
 * The increments are UNIFORM, not Gaussian: xi is uniform on the 2^24 multiples of 2^-23 in [-1, 1), variance 1/3, mean
 * -2^-24.  Over many steps only the variance sigma^2 / 3 per step matters (Euler-Maruyama in the weak sense).  Nothing is
 * clamped: additive noise can take V slightly below 0.
 *   step : the index of the next step the context executes.  It advances by one per time step that gs_step or gs_run
 *          enqueues on this context, whichever species they advance; gs_ctx_get_noise returns the current value.  A
 *          snapshot of the planes plus the saved gs_noise continues a run exactly; gs_ctx_set_noise with the same seed and
 *          an earlier step replays it.
 * gs_ctx_set_noise(ctx, NULL) detaches the noise.  Sigmas must be finite and >= 0: GS_ERR_INVALID otherwise.  Both sigmas
 * zero is legal and stays attached: the noise kernels run and give the uniform run's bits (the A/B for measuring cost).
 * Noise is the third kind of a context's per-cell data, one kind in force at a time: with a parameter map or a domain mask
 * attached the call returns GS_ERR_UNSUPPORTED, and gs_ctx_set_param_map / gs_ctx_set_mask refuse a context that has noise.
 * A pinned GS_KERNEL_WINDOW, _LDS or _TILE: GS_ERR_UNSUPPORTED.  use_graph = 1: GS_ERR_UNSUPPORTED (a replayed graph would
 * replay its step keys).  The call waits for enqueued work; in a multi-process run it is collective and every process
 * passes the same struct.  With noise, gs_run runs the marching kernel at every grid size, gs_step the streaming one and a
 * pinned GS_KERNEL_SIMPLE the simple one; their noise forms carry a "/noise" suffix in gs_ctx_info (e.g.
 * "tb-k4c2/strict.op/noise") and share no differences.  The on-line tuner keeps noise runs apart from the other kernel sets;
 * whatever it does, step s is computed with key(s).  Units at rest never apply.  Ensembles ignore the
 * context's noise; see gs_members_set_noise.
 *   gs_ctx_get_noise : *out = the struct in force with the current step (untouched when none is), *attached = 0 / 1. */
typedef struct gs_noise {
    float sigma_u, sigma_v;
    uint64_t seed;
    uint64_t step;
} gs_noise;
int32_t gs_ctx_set_noise(gs_ctx *ctx, const gs_noise *n);
int32_t gs_ctx_get_noise(const gs_ctx *ctx, gs_noise *out, int32_t *attached);

/* Concentration::default / zeros / ones (concentration/mod.rs:205-218) = create (+ fill).
 * `rows`, `cols` are the GLOBAL shape; every process passes the same values. */
int32_t gs_field_create(gs_ctx *ctx, gs_field **out, uint64_t rows, uint64_t cols);
int32_t gs_field_destroy(gs_ctx *ctx, gs_field *f);
int32_t gs_field_shape(const gs_field *f, uint64_t *rows, uint64_t *cols);
/* Rows [row0, row1) of the global grid that this process stores. */
int32_t gs_field_local_rows(const gs_field *f, uint64_t *row0, uint64_t *row1);
/* Concentration::raw_shape (mod.rs:223-228): local rows incl. 2 x 4 ghost rows per slab, row
 * pitch in f32. */
int32_t gs_field_raw_shape(const gs_field *f, uint64_t *raw_rows, uint64_t *pitch);

int32_t gs_field_fill(gs_ctx *ctx, gs_field *f, float value);
/* Concentration::fill_slice (mod.rs:230-243): global half-open ranges; rows outside this
 * process's slabs are skipped. */
int32_t gs_field_fill_slice(gs_ctx *ctx, gs_field *f, uint64_t r0, uint64_t r1, uint64_t c0,
                            uint64_t c1, float value);
/* Concentration::finalize (mod.rs:245-253): make the plane usable as a step input, i.e.
 * refresh ghost rows after fill / fill_slice / upload.  gs_step does it on demand. */
int32_t gs_field_finalize(gs_ctx *ctx, gs_field *f);
/* Dense row-major host <-> device copies of this process's rows (blocking).  `host` points
 * at local row 0, i.e. global row `row0` of gs_field_local_rows.  download =
 * Concentration::write_scalar_view (mod.rs:277-288). */
int32_t gs_field_upload(gs_ctx *ctx, gs_field *f, const float *host);
int32_t gs_field_download(gs_ctx *ctx, gs_field *f, float *host);
/* Device address of local slab `slab`'s row 0 (for zero-copy consumers); *pitch in f32. */
int32_t gs_field_device_ptr(const gs_field *f, int32_t slab, void **ptr, uint64_t *pitch,
                            uint64_t *slab_row0, uint64_t *slab_rows, int32_t *device);

/* Tell the library that the caller has written cells of `f` through gs_field_device_ptr (a zero-copy
 * producer): the copies of its boundary rows in the neighbouring slabs' ghost rows are stale, exactly as
 * after gs_field_upload.  The caller orders its writes before the next library call itself (the library's
 * streams do not know about them). */
int32_t gs_field_mark_written(gs_ctx *ctx, gs_field *f);

/* One time step: reads (in_u, in_v), writes (out_u, out_v).  Asynchronous.  The caller
 * flips its handles afterwards, as Species::flip does (concentration/mod.rs:88-92). */
int32_t gs_step(gs_ctx *ctx, gs_field *in_u, gs_field *in_v, gs_field *out_u, gs_field *out_v);

/* Simulate::perform_steps (compute/shared/src/lib.rs:48-58): `steps` steps ping-ponging
 * between slot 0 (u0, v0: input on entry) and slot 1.  *result_slot receives the slot that
 * holds the newest state (steps odd -> 1); the caller swaps its handles accordingly so that
 * "the input concentrations contain the final results" (:51-52).  Asynchronous.  The first runs on
 * a shape time a few candidate configurations (unit height, steps per pass, columns per lane) on
 * passes of the simulation itself -- nothing is recomputed.  A call with fewer than 64 steps still
 * to go never waits for those timings (it reads them in a later call); a longer one waits for each
 * phase, so that a long first run is tuned when it returns.  gs_options.no_tune (or pinning
 * rows_per_block) switches the tuning off. */
int32_t gs_run(gs_ctx *ctx, gs_field *u0, gs_field *v0, gs_field *u1, gs_field *v1,
               uint64_t steps, int32_t *result_slot);

/* Placement by measurement, for the planes of a large Species on a context with one slab per process (the host mirrors'
 * make_species call it for every Species of >= 2^26 cells unless told not to).  Where a hipMalloc lands in HBM is below
 * what a process controls, and it matters: the blocks lie in a few physical regions ("groups", runs of 2-30 consecutive
 * 1 GiB allocations; one large allocation is always inside one), and two planes of ONE group that a pass writes (and
 * reads) together are slow -- a pass that reads two 1 GiB blocks and writes them back takes 0.86-0.96 ms within a group,
 * 0.72-0.79 ms across groups, whatever the offsets, while every block alone reads and writes at the same rate from
 * every XCD (tools/ubench/hbm_kinds.hip; profiles/r06_placement.md).  Four planes of one group run the HBM-bound
 * single-step kernel at 0.58-0.65 of 8 TB/s, U's planes in one group and V's in another at 0.73-0.76, and the marching
 * kernel of gs_run gains 8-12 % at 16384^2.  This call times that pass (which leaves the blocks' contents alone) over
 * the pairs among the planes' four blocks (6 probes of 3 passes, 20 ms at 16384^2).  If each slot's (U, V) pair is as
 * fast as the fastest pair seen, and a slower pair has been seen, nothing moves and nothing is allocated.  Else it
 * draws blocks of the planes' size ONE AT A TIME -- at most `candidates` (1..124; the hosts' default is 12: at most
 * 12 GiB held for a moment at 16384^2) --, times each against every block held, stops as soon as two disjoint fast pairs
 * exist, moves the planes that have to move (device copies, one at a time: the planes KEEP THEIR CONTENTS, also when a
 * copy fails) and frees the rest.  A fresh box can hand out 16 and more consecutive blocks of one region: if `candidates`
 * draws do not settle it and MORE THAN HALF of the device's memory is free, the search goes on to 4 x `candidates` blocks
 * with one probe per block (planes of >= 512 MiB; GS_HIP_PLACE_DEEP=0 switches it off).  It waits for the context's work first and can come at any time.  first_ms / best_ms
 * (optional): mean time of the probe pass over the two slots' (U, V) pairs, before and after (0 when nothing was done). */
int32_t gs_fields_place(gs_ctx *ctx, gs_field *const planes[4], int32_t candidates, float *first_ms, float *best_ms);

/* Wait for everything enqueued on this context (all local devices and streams). */
int32_t gs_sync(gs_ctx *ctx);

/* Overlapped result download -- the analogue of ImageConcentration::write_scalar_view_after /
 * make_scalar_view_after (data/src/concentration/gpu/image/mod.rs:183-206), which `simulate`
 * uses so that the N steps and the download of the result are one asynchronous submission
 * (simulate/src/main.rs:99-106).
 *   gs_host_alloc / gs_host_free   page-locked host memory for the images
 *   gs_field_download_async        enqueue "copy this process's rows of `f` to `host`" behind
 *                                  the work already enqueued and return at once.  The plane is
 *                                  first densified into a device staging buffer, so steps
 *                                  enqueued afterwards are not held back by PCIe; `host` must
 *                                  stay valid until gs_download_wait / gs_sync.  It never waits: behind
 *                                  a persistent window launch (1080 x 1920 in long calls), which may
 *                                  still give up, the image is validated when it is waited for -- a
 *                                  launch that gave up is then run again and the image fetched again.
 *   gs_download_wait               wait for the downloads enqueued so far (not for later steps)
 *   gs_download_wait_but           ... for all but the newest `in_flight` (0 or 1) of them: with two images in flight
 *                                  (two staging buffers are used in turn) the host copy of one image overlaps the
 *                                  staging of the next and the hand-over of the one before: the PCIe link stays busy */
int32_t gs_host_alloc(void **out, uint64_t bytes);
int32_t gs_host_free(void *p);
int32_t gs_field_download_async(gs_ctx *ctx, gs_field *f, float *host);
int32_t gs_download_wait(gs_ctx *ctx);
int32_t gs_download_wait_but(gs_ctx *ctx, int32_t in_flight);

/* The per-pixel work of data-to-pics (data-to-pics/src/main.rs:139-144, ui/src/lib.rs:113-123): paint this
 * process's rows of `f` (the reference paints the V plane) into dense RGB8 [rows, cols, 3] through a
 * palette of n_colors RGB triples: pixel = palette[clamp(floor((double)(scale * value) * n_colors), 0,
 * n_colors - 1)], NaN -> entry 0 -- the rule of colorous' sequential gradients (the reference uses
 * colorous::INFERNO with scale = AMPLITUDE_SCALE = 1 / 0.5).  The palette is data: a binding passes the
 * 256 entries of the gradient it wants.  Blocking, like gs_field_download. */
int32_t gs_field_colormap(gs_ctx *ctx, gs_field *f, float scale, const uint8_t *palette_rgb, int32_t n_colors,
                          uint8_t *host_rgb);

/* Reduced result images: a plane averaged over factor x factor blocks ON THE DEVICE, so that only 1 / factor^2 of its bytes
 * are staged, copied and written -- what a live view, a monitoring loop and a long run at a large grid want of a result.
 *
 * Definition.  For a field of global shape [rows, cols] and an integer factor f, 1 <= f <= 64, the reduced image has shape
 * [ceil(rows / f), ceil(cols / f)], f32.  Pixel (R, C) covers the cells r in [R f, min((R + 1) f, rows)),
 * c in [C f, min((C + 1) f, cols)) (blocks are anchored at GLOBAL row 0 and column 0; edge blocks hold the cells that exist):
 *   1. row partial p_r: an f64 accumulator starting at +0.0 to which the block's cells of row r are added as f64 in
 *      ascending column order;
 *   2. block sum: an f64 accumulator starting at +0.0 to which p_r is added in ascending row order;
 *   3. pixel = (float)(block sum / (double)count), count = number of cells in the block, both roundings to nearest even.
 * Sub-normal cells count as what they are and a sub-normal result is kept.  Non-finite cells are not skipped: NaN and
 * infinities propagate by IEEE rules (a NaN pixel is any NaN).  The result is a function of the plane and f alone: the same
 * bits whatever the slab count, the process count, the step kernel that produced the plane, and whether the blocking or the
 * overlapped call fetched it.  factor == 1 is the plain call (gs_field_download, _download_async, _colormap): same bits, same
 * cost.
 *
 * Slabs.  A block never straddles two slabs: a context in which some slab -- local or, in a multi-process run, any rank's --
 * begins at a global row that is not a multiple of f refuses the call with GS_ERR_UNSUPPORTED and a message that names the
 * slab's first row and f.  The split is k * rows / S, so the verdict is a function of (rows, S, f) and every rank reaches the
 * same one without talking.  In a multi-process run each process receives its own output rows, [row0 / f, ceil(row1 / f))
 * of its rows [row0, row1), as the full-size calls hand it its own rows.
 *
 *   gs_field_reduced_shape           global reduced shape and this process's output rows [local_row0, local_row1) (each
 *                                    pointer may be null); the GS_ERR_UNSUPPORTED verdict without touching the device
 *   gs_field_download_reduced        blocking, like gs_field_download: waits for enqueued work (a persistent window
 *                                    launch that gave up is run again first), `host` holds the image on return
 *   gs_field_download_reduced_async  the overlapped form: gs_field_download_async with the reduction in the place of the
 *                                    staging copy.  Same two staging buffers (of which it needs 1 / f^2), same streams, same
 *                                    waits (gs_download_wait, gs_download_wait_but); full and reduced images may be mixed
 *                                    freely in one stream of calls.  Behind a persistent window launch that gives up the
 *                                    image is formed again from the replayed plane
 *   gs_field_colormap_reduced        gs_field_colormap's palette rule applied to the reduced image: dense RGB8
 *                                    [ceil(rows / f), ceil(cols / f), 3], this process's rows; blocking
 * factor outside 1..64, a null or foreign handle: GS_ERR_INVALID.  An empty field: GS_OK, nothing written. */
int32_t gs_field_reduced_shape(const gs_field *f, int32_t factor, uint64_t *rows, uint64_t *cols, uint64_t *local_row0,
                               uint64_t *local_row1);
int32_t gs_field_download_reduced(gs_ctx *ctx, gs_field *f, int32_t factor, float *host);
int32_t gs_field_download_reduced_async(gs_ctx *ctx, gs_field *f, int32_t factor, float *host);
int32_t gs_field_colormap_reduced(gs_ctx *ctx, gs_field *f, int32_t factor, float scale, const uint8_t *palette_rgb,
                                  int32_t n_colors, uint8_t *host_rgb);

/* Device-side stopwatch on the context's compute stream(s) (HIP events): start/stop
 * bracket enqueued work; elapsed is the maximum over local slabs, in milliseconds. */
int32_t gs_timer_start(gs_ctx *ctx);
int32_t gs_timer_stop(gs_ctx *ctx, float *elapsed_ms);

/* The configuration gs_run uses for slabs of `slab_rows` x `cols` cells: unit height, steps fused per
 * pass, columns per lane, full difference sharing (1 = on, 2 = off, 3 = across lanes too, as gs_options.share_taps; _set_ takes 0 as 3)
 * (zeros from _get_ when nothing was chosen yet).  Single-slab contexts find it
 * themselves (on-line tuning inside gs_run); a slab chain takes what it is given: one process tunes on a
 * single slab of the slab's shape, reads the result with _get_ and every process of the chain sets it
 * with _set_ -- all of them the same values, since the ghost-row exchange is fuse_steps rows deep
 * (grayscott_amd/dist.py: share_tuning). */
int32_t gs_ctx_get_tuned(const gs_ctx *ctx, uint64_t slab_rows, uint64_t cols, int32_t *rows_per_block,
                         int32_t *fuse_steps, int32_t *cols_per_lane, int32_t *share_taps);
int32_t gs_ctx_set_tuned(gs_ctx *ctx, uint64_t slab_rows, uint64_t cols, int32_t rows_per_block,
                         int32_t fuse_steps, int32_t cols_per_lane, int32_t share_taps);

/* What RCCL itself reports for this context's communicator (ncclCommCount / ncclCommUserRank /
 * ncclCommCuDevice): the number of ranks, this rank and its device; 0, -1, -1 for a single process. */
int32_t gs_ctx_comm_info(const gs_ctx *ctx, int32_t *rccl_ranks, int32_t *rccl_rank, int32_t *rccl_device);

/* Counters of a context since its creation, and -- on slab chains -- where the time of the passes timed
 * with gs_ctx_set_pass_timing went.  Not part of the reference's interface: what bench.py and the tests
 * read instead of inferring it from launch counts. */
typedef struct gs_stats {
    uint64_t passes;          /* passes over the planes enqueued (one pass advances 1..8 time steps)        */
    uint64_t steps;           /* time steps enqueued                                                       */
    uint64_t launches;        /* step-kernel launches (slab chains: boundary band + interior per slab)     */
    uint64_t ghost_refreshes; /* blocking ghost-row refreshes (slab chains: after fill / upload, or when a  *
                               * pass needs deeper ghost rows than the previous one left)                  */
    uint64_t timed_passes;    /* passes covered by the three sums below (the slowest local slab's)         */
    float halo_ms;            /* halo stream: boundary-band kernel + ghost-row exchange, summed             */
    float interior_ms;        /* compute stream: interior kernel, summed                                   */
    float halo_exposed_ms;    /* sum over passes of max(0, end of the halo stream's work - end of the      *
                               * interior kernel): what the exchange did NOT hide behind the interior      */
    float reserved;
    uint64_t window_fallbacks; /* persistent window launches that gave up (another kernel held compute units) and were  *
                                * run again by the marching kernel: 0 or 1, the context stays with the marching kernel  *
                                * afterwards; a timing that contains one measured the stall, not a rate               */
} gs_stats;
int32_t gs_ctx_stats(gs_ctx *ctx, gs_stats *out);
/* Time the next `passes` passes (0..4096; 0 = off) of every local slab of a slab chain with HIP events on
 * the halo and compute streams; gs_ctx_stats waits for them and reports the sums.  Waits for enqueued work. */
int32_t gs_ctx_set_pass_timing(gs_ctx *ctx, int32_t passes);
/* Units at rest.  (U, V) = (1.0f, +0.0f) is a fixed point of the update bit for bit, so a unit of the marching kernel --
 * a wave's rows x columns of a pass -- whose whole input window and whose output rows hold nothing else is not
 * recomputed by the full passes of a gs_run from the third on (single slab, one launch per pass, clipped or zero-halo
 * rule, strict math, finite parameters, no map, no mask, no graph; GS_HIP_QUIET_UNITS=0 when the context is created
 * switches it off).  The results are the same bits either way.  out[0] = units launched by the passes that took part,
 * out[1] = units among them that left without computing, out[2] = those passes, out[3] = the ones among them that could
 * skip (the third and later of their gs_run), all since the context was created.  Waits for enqueued work.
 * out[0] counts every unit.  out[1] counts what it always counted: the units with interior positions all around them -- no
 * unit position of the nine is on an edge of the grid.  The others are counted by gs_ctx_quiet_edge_stats. */
int32_t gs_ctx_quiet_stats(gs_ctx *ctx, uint64_t out[4]);
/* ... and the units on the grid's edges among them: the first and last strips of columns and the row chunks that touch the
 * grid's first or last rows, each half of such a position counting as a unit where the pass dispatched it as two halves.
 * Under the clipped rule they rest like any other unit (a neighbour outside the grid does not exist: no tap reads it);
 * under the zero-halo rule they never do (a halo of 0 next to U = 1 is a tap of -1), and neither do the interior units next
 * to them.  out[0] = units of edge positions launched by the passes that took part (included in gs_ctx_quiet_stats'
 * out[0]), out[1] = the ones among them that left without computing (by halves: a whole unit of an edge position that
 * leaves -- GS_HIP_EDGE_SPLIT=0, a chunk of one row -- counts as its two), out[2] = the interior units next to an edge position
 * that left without computing (neither is included in gs_ctx_quiet_stats' out[1]).  Waits for enqueued work. */
int32_t gs_ctx_quiet_edge_stats(gs_ctx *ctx, uint64_t out[3]);

/* Introspection for tests and the bench: name of the kernel variant last launched
 * ("tb-k4/strict@32x2" = 4 fused steps, strict math, tuned: 32-row units, 2 row bands; the periodic rule's kernels
 * carry "/periodic": "tb-k4c2/strict.op.dx/periodic@38x1") and the number of kernel launches so far. */
int32_t gs_ctx_info(const gs_ctx *ctx, char *kernel_name, size_t cap, uint64_t *launches);

/* Ensembles: `members` independent simulations of one shape rows x cols, advanced in shared launches -- a sweep over
 * (feed, kill), diffusion rates, dt or stencils.  An ensemble lives on a context of ONE slab in one process
 * (GS_ERR_UNSUPPORTED otherwise); every member has its own gs_params and its own U and V, the context's math and boundary
 * options apply to all of them.  After gs_ensemble_run(steps), member i is bit for bit what gs_run makes of a lone
 * Species with member i's parameters and initial state.  The ensemble owns its double buffer and tracks which slot
 * holds the newest state: callers never flip.  Host arrays are dense [count, rows, cols] f32.
 *   create        all members zero, every member with the context's parameters
 *   set_params    `count` = members (one entry per member) or 1 (the same for all); GS_MATH_FUSED refuses weights that
 *                 are not 0 or a power of two (GS_ERR_UNSUPPORTED), as gs_ctx_create does.  Waits for enqueued work.
 *   seed          Species::new's pattern (data/src/concentration/mod.rs:36-59) in every member
 *   upload        members [first, first + count); `u` or `v` may be NULL to leave that species as it is.  Blocking.
 *   download      species 0 = U, 1 = V of members [first, first + count).  Blocking.
 *   run           asynchronous, like gs_run (gs_sync waits).  Members of at most 4096 cells (8192 under the zero-halo
 *                 and periodic rules, and 160 KiB of LDS) stay in one workgroup's LDS for the whole call ("ensemble-resident"); larger
 *                 ones advance up to 8 steps per launch on LDS-resident windows ("ensemble-tile32x64" ...), with the
 *                 window and steps per launch chosen over the workgroups of the whole ensemble.  gs_ctx_info names it. */
typedef struct gs_ensemble gs_ensemble;
int32_t gs_ensemble_create(gs_ctx *ctx, gs_ensemble **out, uint64_t members, uint64_t rows, uint64_t cols);
int32_t gs_ensemble_destroy(gs_ctx *ctx, gs_ensemble *e);
int32_t gs_ensemble_shape(const gs_ensemble *e, uint64_t *members, uint64_t *rows, uint64_t *cols);
int32_t gs_ensemble_set_params(gs_ctx *ctx, gs_ensemble *e, const gs_params *params, uint64_t count);
int32_t gs_ensemble_seed(gs_ctx *ctx, gs_ensemble *e);
int32_t gs_ensemble_upload(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const float *u, const float *v);
int32_t gs_ensemble_download(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, int32_t species, float *host);
int32_t gs_ensemble_run(gs_ctx *ctx, gs_ensemble *e, uint64_t steps);

/* Active sets: members that have settled stop advancing.  Every member of an ensemble has an ACTIVE flag (set at creation)
 * and a STEP COUNT: the steps gs_ensemble_run has advanced it by since the ensemble was created.
 *   gs_members_set_active  active[i] != 0: member first + i is active, i < count; the other members keep their flags.
 *                          Blocking: it waits for enqueued work.  It touches neither parameters nor cells as seen through
 *                          the newest slot.
 *   gs_members_get_active  active[i] (0 or 1) and steps_taken[i] of member first + i, i < count, and *active_total: the
 *                          number of active members of the WHOLE ensemble.  Any of the three may be NULL, not all.  No device
 *                          work: steps that are enqueued count as taken.
 * Inactive means: gs_ensemble_run(steps) advances the active members only -- an inactive member keeps its bits and its step
 * count, whatever the number and parity of the runs; an active member is still bit for bit what gs_run makes of a lone
 * Species with its parameters and initial state after its OWN step count.  With no active member gs_ensemble_run is GS_OK
 * and launches nothing.  With a proper subset active it runs the listed forms of the ensemble kernels -- their workgroups
 * take their member from a device list of the active members' indices --, gs_ctx_info names them with a "/listed" suffix
 * ("ensemble-resident/strict.op/listed"), and the kernel form and its configuration are chosen for the members that run;
 * with every member active (again) it runs exactly what an ensemble without an active set runs.
 * What readers see: every call that reads the newest slot -- gs_ensemble_download, gs_members_summarize, gs_members_histogram,
 * gs_members_compare, gs_members_copy as source -- returns the held state of an inactive member.
 * What writers do: gs_ensemble_seed, gs_ensemble_upload, gs_ensemble_set_params and gs_members_copy (as destination) work on
 * inactive members as before, and the written state is what readers see afterwards and what the member holds from then on;
 * a reactivated member continues from it (no copy is made).  Step counts are neither copied by gs_members_copy nor reset by
 * anything.  The first gs_ensemble_run after members were retired, or written while inactive, waits for enqueued work and
 * copies those members into the ensemble's other slot (one launch) before it advances the rest.
 * GS_ERR_INVALID, all decided before any device work: a null or foreign handle, members outside the ensemble, a null
 * `active` (set_active), all three outputs null (get_active).  GS_ERR_UNSUPPORTED: set_active on an ensemble of more than
 * 2^31 members (the list holds 32-bit indices). */
int32_t gs_members_set_active(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const uint8_t *active);
int32_t gs_members_get_active(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, uint8_t *active, uint64_t *steps_taken,
                              uint64_t *active_total);

/* Noise of an ensemble: many realisations in shared launches.  Noise is attached to an ENSEMBLE, per member: every member
 * has its own gs_noise -- sigmas, seed and step counter; the context's noise (gs_ctx_set_noise) does not touch ensembles.
 * The generator, the step key, the draw, xi and the two operations per species are those defined under gs_ctx_set_noise, to
 * the bit: after any sequence of gs_ensemble_run calls, member i of an ensemble with noise is bit for bit what gs_run makes
 * of a lone Species on a context with member i's parameters, member i's initial state and member i's gs_noise attached,
 * after member i's own step count -- under all four boundary rules, in both math flavours, in both ensemble forms
 * (resident, windowed) and with or without an active set.
 *   gs_members_set_noise    noise[i] for member first + i, i < count, when entries == count; noise[0] for all of them when
 *                           entries == 1.  The first call attaches noise to the ensemble: members never named hold sigmas
 *                           0, seed 0 and step 0.  Later calls overwrite the named members only.  Blocking: it waits for
 *                           enqueued work.
 *   gs_members_get_noise    out[i] = member first + i's struct with its CURRENT step, *attached = 0 / 1 for the ensemble;
 *                           `out` is untouched when it is 0.  Either may be NULL, not both.  No device work: steps that are
 *                           enqueued count as taken, as in gs_members_get_active.
 *   gs_members_clear_noise  detaches: the next run launches exactly the kernels of an ensemble without noise.
 * Coordinates: a cell draws at its member-local (row, column); under the periodic rule a cell computed at a wrapped
 * position draws at the wrapped one.  Cells outside a member are zeros, unread or ring copies, as the rule says, and never
 * a source of noise.
 * Step counters: a member's counter starts at its gs_noise.step and advances by one per step THAT MEMBER takes -- a retired
 * member keeps its counter and goes on from it when it is reactivated.  The counter is u64 and wraps.  gs_members_copy
 * copies no noise, as it copies no step counts: a gs_members_copy into another ensemble plus the structs read back with
 * gs_members_get_noise continue a run exactly.
 * Zero sigmas: a member whose sigmas are both 0 has the bits of the plain run, a species whose sigma is 0 is not touched (-0
 * stays -0); the noise kernels run all the same (the A/B for measuring cost).  The multiply and the add are never
 * contracted in either flavour; GS_MATH_STRICT flushes sub-normal products and sums.
 * With noise attached gs_ensemble_run runs the noise forms of the two ensemble kernels, members of the same sizes in the
 * same form: gs_ctx_info names them with "/noise" behind the rule's suffix, and "/listed" behind that while a proper subset
 * of the members is active ("ensemble-resident/strict.op/noise", "ensemble-tile32x64/strict/periodic/noise/listed").  The
 * step key is formed on the device, once per step and member.
 * GS_ERR_INVALID, all decided before any device work: a null or foreign handle, members outside the ensemble, a null
 * `noise`, `entries` neither 1 nor `count`, a sigma that is negative or not finite (set_noise); both outputs null
 * (get_noise).  GS_ERR_UNSUPPORTED: set_noise on an ensemble of more than 2^31 members (the noise kernels take the list of
 * active members, which holds 32-bit indices).  Noise together with parameter maps or masks does not exist: ensembles have
 * neither. */
int32_t gs_members_set_noise(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const gs_noise *noise, uint64_t entries);
int32_t gs_members_get_noise(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, gs_noise *out, int32_t *attached);
int32_t gs_members_clear_noise(gs_ctx *ctx, gs_ensemble *e);

/* Summaries computed on the device: for one plane of the WHOLE global grid, the sum and sum of squares of its finite
 * cells, their minimum and maximum, and the count of non-finite cells (NaN, +-inf) -- without downloading the plane.
 *   gs_fields_summarize    out[i] for fields[i], i < n (1..4 fields of one shape, e.g. U and V of a Species): one wait for
 *                          enqueued work (as gs_field_download does: a persistent window launch that gave up is run again
 *                          first), one launch per slab, one exchange.  In a multi-process context the call is collective,
 *                          like gs_run, and every rank receives the summary of the global grid.
 *   gs_members_summarize  out[2 i] (U) and out[2 i + 1] (V) of members first + i, i < count, from the newest slot.
 * Both block and have no side effects (ghost rows, tuner, graphs and gs_stats are left as they are).  GS_ERR_INVALID: a
 * null or foreign handle, mixed shapes, n outside 1..4, members outside the ensemble.  An empty plane: sums +0, min +inf,
 * max -inf, nonfinite 0.
 * Fold order -- a function of (rows, cols) alone, so that the results are bit-reproducible whatever the slab count, the
 * process count or the step kernel, and a member's summary is bit for bit that of a lone Species in the same state:
 *   1. row partial: each of 64 lanes holds an f64 accumulator starting at +0.0; lane l adds, in this order, the cells at
 *      columns 256 k + 4 l + j for k = 0, 1, ... and j = 0..3 (x as f64; for sum_sq the product x * x formed in f64,
 *      which is exact).  A column >= cols or a non-finite cell adds nothing;
 *   2. lane combine: the 64 partials are halved repeatedly, p[0:32] + p[32:64], then p[0:16] + p[16:32], ... down to one;
 *   3. field fold: the row partials are added one after the other in f64, in ascending GLOBAL row order, from +0.0.
 * min and max are order-free (the sign of a zero extreme is not specified); sub-normal cells count as the values they
 * are (never flushed). */
typedef struct gs_summary {
    double sum;         /* of the finite cells, in the fold order above                   */
    double sum_sq;      /* of x * x over the finite cells (formed in f64: exact), same order */
    float min, max;     /* of the finite cells; +inf / -inf when there are none           */
    uint64_t nonfinite; /* NaN and +-inf cells                                            */
} gs_summary;           /* 32 bytes */
int32_t gs_fields_summarize(gs_ctx *ctx, gs_field *const *fields, int32_t n, gs_summary *out);
int32_t gs_members_summarize(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, gs_summary *out);

/* Histograms computed on the device: how the values of one plane of the WHOLE global grid are distributed over `bins`
 * (1..4096) equal bins of a range lo < hi (finite f32) -- without downloading the plane.  A result is bins + 3 unsigned
 * 64-bit counters: counts[0 .. bins), then below, above, nan.  Every cell x lands in exactly one of them:
 *   1. x is NaN            -> nan;
 *   2. x < lo (-inf too)   -> below;
 *   3. x > hi (+inf too)   -> above;
 *   4. otherwise           -> counts[b], b = min((int)t, bins - 1), t = (x - lo) * scale.
 * The subtraction and the multiplication are one f32 operation each, rounded to nearest even, never contracted; sub-normal
 * inputs and results are kept; the conversion truncates (t >= 0 here).  scale = (float)bins / (hi - lo) is formed once on
 * the host in f32: one subtraction, one division.  What follows:
 *   - the last bin is closed: x == hi counts in bin bins - 1 (U is exactly 1.0 over most of a fresh Species: [0, 1] holds it);
 *   - -0.0 with lo == 0 is in bin 0;
 *   - t is monotone in x, so every bin is an interval; its edges are where the formula steps: within rounding of
 *     lo + i (hi - lo) / bins, but not defined by that expression;
 *   - the counters sum to rows x cols;
 *   - counts are integers: the result is the same bits for any slab count, process count, step kernel or launch shape,
 *     and a member's is that of a lone Species in the same state;
 *   - this is the library's own rule, not numpy.histogram's, which bins in f64 and differs in cells next to an edge.
 *   gs_fields_histogram   out[i * (bins + 3) ...] for fields[i] with the range lo[i], hi[i], i < n (1..4 fields of one
 *                         shape; U and V live on different ranges): one wait for enqueued work (as gs_fields_summarize: a
 *                         persistent window launch that gave up is run again first), one launch per slab.  In a
 *                         multi-process context the call is collective, like gs_run, and every rank receives the counts
 *                         of the global grid.
 *   gs_members_histogram  out[(2 i + s) * (bins + 3) ...] for species s (0 = U with lo[0], hi[0]; 1 = V with lo[1], hi[1])
 *                         of member first + i, i < count, from the newest slot: one launch, one copy.
 * Both block and have no side effects (ghost rows, tuner, graphs and gs_stats are left as they are).  GS_ERR_INVALID, all
 * decided before any device work: lo or hi not finite, or lo >= hi; hi - lo or scale not a finite, normal, positive f32;
 * bins outside 1..4096; a null or foreign handle, mixed shapes, n outside 1..4, members outside the ensemble.  An empty
 * plane: GS_OK, every counter 0. */
int32_t gs_fields_histogram(gs_ctx *ctx, gs_field *const *fields, int32_t n, const float *lo, const float *hi, int32_t bins,
                            uint64_t *out);
int32_t gs_members_histogram(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const float lo[2], const float hi[2],
                             int32_t bins, uint64_t *out);

/* Morphology computed on the device: the bit-quad counts (Gray) of one plane of the WHOLE global grid after thresholding --
 * from which the area, the boundary length and the Euler number of the pattern follow exactly (the Minkowski functionals of
 * integral geometry: "spots, stripes or holes?") -- without downloading the plane.  For a plane x of R x C cells, a threshold
 * t and a sense `above`:
 *   - a cell is SET iff x > t (above != 0) or x < t (above == 0): one f32 comparison.  A NaN cell is never set, a cell equal
 *     to t is not set, infinities compare as they do, a sub-normal cell is the value it is (never flushed);
 *   - the binary image is padded with one ring of UNSET cells, under every boundary rule: a spot that crosses a periodic
 *     edge counts as two pieces (quads that wrap are not formed);
 *   - every 2 x 2 block of the padded image is a quad; its top-left corner runs over rows -1 .. R - 1 and columns
 *     -1 .. C - 1: (R + 1)(C + 1) quads.  A quad falls into one of six classes by its set cells, in this order in `quads`:
 *       Q0 none, Q1 one, Q2 two that share a side, Q3 three, Q4 four, QD two on a diagonal.
 *   The six counts sum to (R + 1)(C + 1).  An empty plane (R = 0 or C = 0): GS_OK, six zeros.
 * What the hosts derive, all exact integers:
 *   set cells                       A      = (Q1 + 2 Q2 + 2 QD + 3 Q3 + 4 Q4) / 4
 *   4-connected boundary length     P      = Q1 + Q2 + 2 QD + Q3   (cell sides between a set and an unset cell, the padding
 *                                                                   ring included)
 *   8-connected components - holes  euler8 = (Q1 - Q3 - 2 QD) / 4
 *   4-connected components - holes  euler4 = (Q1 - Q3 + 2 QD) / 4
 * Counts are integers and additive over any partition of the quads: the result is the same bits for any slab count, process
 * count, step kernel or launch shape, and a member's is that of a lone Species in the same state.
 *   gs_fields_morphology   out[i * nt + k] for fields[i] thresholded at thresholds[i * nt + k] with the sense above[i], i < n
 *                          (1..4 fields of one shape), k < nt (1..4 thresholds per field, all counted in one pass over the
 *                          plane): one wait for enqueued work (as gs_fields_summarize: a persistent window launch that gave up
 *                          is run again first), one launch per slab.  The row above a slab's first row is staged from the
 *                          slab (or process) above into a buffer of its own: ghost rows are never read.  In a multi-process
 *                          context the call is collective, like gs_run, and every rank receives the counts of the global grid.
 *   gs_members_morphology  out[(2 i + s) * nt + k] for species s (0 = U with thresholds[k] and above[0]; 1 = V with
 *                          thresholds[nt + k] and above[1]) of member first + i, i < count, from the newest slot: one launch,
 *                          one copy.  A member never sees its neighbours' rows.
 * Both block and have no side effects (ghost rows, tuner, graphs and gs_stats are left as they are).  GS_ERR_INVALID: a null
 * argument, nt outside 1..4 or a NaN threshold -- decided before any handle is looked at --, a null or foreign handle, mixed
 * shapes, n outside 1..4, members outside the ensemble. */
typedef struct gs_morphology {
    uint64_t quads[6]; /* Q0, Q1, Q2, Q3, Q4, QD */
} gs_morphology;       /* 48 bytes */
int32_t gs_fields_morphology(gs_ctx *ctx, gs_field *const *fields, int32_t n, const float *thresholds, const int32_t *above,
                             int32_t nt, gs_morphology *out);
int32_t gs_members_morphology(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const float *thresholds,
                              const int32_t above[2], int32_t nt, gs_morphology *out);

/* Regional observables computed on the device: the summary and the bit-quad counts of every REGION of one plane of the global
 * grid -- which part of a parameter map's grid grew spots, which stripes, which died, which blew up -- without downloading
 * the plane.  A region shape (rh, rw) cuts the global grid of R x C cells into RR = ceil(R / rh) by RC = ceil(C / rw) regions:
 * region (i, j), of index i * RC + j, holds rows [i rh, min((i + 1) rh, R)) and columns [j rw, min((j + 1) rw, C)).  The last
 * row and column of regions may be ragged; they are kept, never dropped.
 * The rule that defines every result: a region's result is, bit for bit, what gs_fields_summarize / gs_fields_morphology
 * return for a field that holds exactly that region's cells.
 *   - summary: the fold order above with columns counted from the region's FIRST column -- lane l adds the region's columns
 *     256 k + 4 l + j, the halving lane combine follows, then the region's rows are added in ascending order from +0.0.  min,
 *     max, nonfinite, sub-normal cells and the sign of a zero extreme: as for the whole grid.
 *   - morphology: the region's thresholded image is padded with its OWN ring of unset cells -- a region never sees its
 *     neighbours' cells, as an ensemble member never sees its neighbours' rows.  A region of h x w cells has (h + 1)(w + 1)
 *     quads in the six classes, which sum to that; the set rule is morphology's (NaN and equal-to-threshold cells unset).
 *     The regions do not partition the quads of the global grid.
 * Results are the same bits for any slab count, process count, step kernel or launch shape and do not depend on the
 * boundary rule; with a domain mask attached wall cells count, as in the whole-grid calls.
 *   gs_region_grid               *rr = RR and *rc = RC for a grid of rows x cols cells, or the refusal of a region shape.
 *                                Pure: no handle, no device.
 *   gs_fields_region_summaries   out[p * RR RC + i RC + j] for region (i, j) of fields[p], p < n (1..4 fields of one shape).
 *   gs_fields_region_morphology  out[(p * RR RC + i RC + j) * nt + k] for region (i, j) of fields[p] thresholded at
 *                                thresholds[p * nt + k] with the sense above[p], k < nt (1..4 thresholds per field, all counted
 *                                in one pass over the plane); Q0 is the host's complement, as for the whole grid.
 * Both wait once for enqueued work (as gs_fields_summarize: a persistent window launch that gave up is run again first), read
 * every plane once with one launch per slab, block, and have no side effects (ghost rows, tuner, graphs and gs_stats are
 * left as they are).  In a multi-process context they are collective, like gs_run, and every rank receives every region.
 * Limits, all decided before any device work -- GS_ERR_INVALID: rw not a multiple of 4 or below 16 (a lane's four columns
 * never straddle two regions); rh < 1; RR RC > GS_REGIONS_MAX (a cap on result memory: 128 MiB of summaries per plane); a
 * null argument, nt outside 1..4 or a NaN threshold -- decided before any handle is looked at --; a null or foreign handle,
 * mixed shapes, n outside 1..4.  GS_ERR_UNSUPPORTED, on every rank alike: a context of several slabs or processes in which
 * some slab begins at a row that is no multiple of rh (as for gs_field_download_reduced: a region lies inside one slab, no
 * ghost row is read and no row is staged).  An empty plane: GS_OK, nothing is written. */
#define GS_REGIONS_MAX (1u << 22)
int32_t gs_region_grid(uint64_t rows, uint64_t cols, int32_t rh, int32_t rw, uint64_t *rr, uint64_t *rc);
int32_t gs_fields_region_summaries(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw, gs_summary *out);
int32_t gs_fields_region_morphology(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw,
                                    const float *thresholds, const int32_t *above, int32_t nt, gs_morphology *out);

/* Regional two-point correlations: the pair counts of gs_fields_correlation (below) of every region of the same region grid
 * -- how far apart the spots or stripes of each part of a parameter map's grid are; the whole-grid counts of such a grid
 * are a blend that belongs to no region.
 *   gs_fields_region_correlation  out[((((p * RR + i) * RC + j) * nt + t) * 4 + k) * (L + 1) + d] is, bit for bit, what
 *                                 gs_fields_correlation returns for a field that holds region (i, j)'s cells alone, for
 *                                 direction k, lag d, and fields[p] thresholded at thresholds[p * nt + t] with the sense
 *                                 above[p], L = max_lag.
 * The set rule and the four unit steps are the whole-grid correlation's.  A region's border is a wall: a pair whose two
 * cells lie in different regions is never formed, under every boundary rule.  A lag that does not fit the region, a ragged
 * one included, counts 0; d = 0 is the region's area for all four k.  The number of pairs that exist in a region of h x w
 * cells, N_k(d) = max(h - d dr, 0) max(w - d |dc|, 0), is the hosts' to compute.  The regions do not partition the pairs of
 * the global grid.  With a domain mask attached wall cells count.
 * The call follows its two twins above: one wait for enqueued work, one launch per slab, blocking, no side effects (ghost
 * rows, tuner, graphs and gs_stats are left as they are), collective in a multi-process context with every rank receiving
 * every region; an empty plane: GS_OK, nothing is written.  GS_ERR_INVALID, decided in this order: a null argument; rh or
 * rw refused by gs_region_grid; nt outside 1..4; a NaN threshold; max_lag outside 1..64 -- all before any handle is looked
 * at --; a null or foreign handle, mixed shapes, n outside 1..4; RR RC > GS_REGIONS_MAX; RR RC nt 4 (L + 1) >
 * GS_REGION_PAIRS_MAX counters per field (a cap on result memory: 256 MiB per field).  GS_ERR_UNSUPPORTED, on every rank
 * alike: some slab begins at a row that is no multiple of rh, as above -- a region lies inside one slab, so nothing is staged
 * and no ghost row is read.
 * Not done: regions of ensemble members; pairs wrapped under the periodic rule; lags beyond 64; regions that straddle slabs. */
#define GS_REGION_PAIRS_MAX (1u << 25)
int32_t gs_fields_region_correlation(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw,
                                     const float *thresholds, const int32_t *above, int32_t nt, int32_t max_lag, uint64_t *out);

/* Regional histograms: the histogram of gs_fields_histogram (above) of every region of the same region grid -- what
 * fraction of each part of a parameter map's grid lies above any x chosen after the run, its median and quantiles, and
 * whether it is bimodal ("half spots, half background") where a summary's mean and variance cannot tell.
 *   gs_fields_region_histogram  out[((p * RR + i) * RC + j) * (bins + 3) + s] is slot s -- counts[0 .. bins), then below,
 *                               above, nan -- of region (i, j) of fields[p] and, bit for bit, what gs_fields_histogram
 *                               returns for a field that holds that region's cells alone, with the range lo[p], hi[p] and
 *                               the same bins.
 * The binning rule is the whole-grid histogram's, word for word: scale formed once on the host in f32, the subtraction and
 * the multiplication one f32 operation each, sub-normal cells and products kept, the last bin closed, -0.0 with lo == 0 in
 * bin 0.  A region's bins + 3 counters sum to its number of cells, ragged regions in the last row and column of the region
 * grid included; over all regions every slot sums to the whole-grid histogram's slot, because the regions partition the
 * cells.  Counts are integers: the result is the same bits for any slab count, process count, step kernel or launch shape
 * and does not depend on the boundary rule; with a domain mask attached wall cells count.
 * The call follows its three twins above: one wait for enqueued work, one launch per slab, blocking, no side effects (ghost
 * rows, tuner, graphs and gs_stats are left as they are), collective in a multi-process context with every rank receiving
 * every region; an empty plane: GS_OK, nothing is written.  GS_ERR_INVALID, decided in this order: a null argument; rh or
 * rw refused by gs_region_grid; bins outside 1..4096; the range refusals of gs_fields_histogram (lo or hi not finite,
 * lo >= hi, hi - lo or scale not a finite, normal, positive f32) for fields 0 .. n - 1 when n is within 1..4 -- all before
 * any handle is looked at --; a null or foreign handle, mixed shapes, n outside 1..4; RR RC > GS_REGIONS_MAX; RR RC
 * (bins + 3) > GS_REGION_HIST_MAX counters per field (a cap on result memory: 256 MiB per field).  GS_ERR_UNSUPPORTED, on
 * every rank alike: some slab begins at a row that is no multiple of rh, as above.
 * Not done: regions of ensemble members; regions that straddle slabs. */
#define GS_REGION_HIST_MAX (1u << 25)
int32_t gs_fields_region_histogram(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw, const float *lo,
                                   const float *hi, int32_t bins, uint64_t *out);

/* Two-point correlations computed on the device: the two-point probability function of one plane of the WHOLE global grid
 * after thresholding -- for a lag vector, the number of cell pairs that far apart which are both set; from it the pattern's
 * wavelength and the direction of its stripes follow ("how far apart are the spots?") -- without downloading the plane.  For
 * a plane x of R x C cells, a threshold t, a sense `above` and a largest lag L, 1 <= L <= 64:
 *   - a cell is SET by morphology's rule: iff x > t (above != 0) or x < t (above == 0), one f32 comparison.  A NaN cell is
 *     never set, a cell equal to t is not set, infinities compare as they do, a sub-normal cell is the value it is (never
 *     flushed);
 *   - four unit steps e_k = (dr, dc):  k = 0: (0, 1) along a row;  k = 1: (1, 0) down a column;  k = 2: (1, 1) the diagonal;
 *     k = 3: (1, -1) the anti-diagonal;
 *   - pairs[k][d], d = 0 .. L, is the number of unordered cell pairs {p, p + d e_k} with both cells inside the grid and both
 *     set.  d = 0 is the number of set cells, the same for all four k: morphology's area A.  Pairs NEVER wrap, under every
 *     boundary rule, as morphology's quads never do: a pair across a periodic edge is not formed.  A lag that does not fit
 *     the grid counts 0.
 * The number of pairs that exist, N_k(d) = max(R - d dr, 0) max(C - d |dc|, 0), is geometry: the hosts compute it -- and from
 * both S2_k(d) = pairs / N, the autocovariance S2 - (A / (R C))^2, its first minimum (half the wavelength) and the maximum
 * after it (the wavelength) --, the device does not.  An empty plane (R = 0 or C = 0): GS_OK, all zeros.
 * Counts are integers and additive over any partition of the pairs: the result is the same bits for any slab count, process
 * count, step kernel or launch shape, and a member's is that of a lone Species in the same state.
 *   gs_fields_correlation   out[((i * nt + j) * 4 + k) * (L + 1) + d] for fields[i] thresholded at thresholds[i * nt + j] with
 *                           the sense above[i], i < n (1..4 fields of one shape), j < nt (1..4 thresholds per field, all
 *                           counted in one pass over the plane), L = max_lag: one wait for enqueued work (as
 *                           gs_fields_summarize: a persistent window launch that gave up is run again first), one launch per
 *                           slab.  A pair belongs to its lower row; the min(L, r0) rows above a slab's first row r0 are staged
 *                           from the slab (or process) above into a buffer of its own: ghost rows are never read.  A context
 *                           of more than one slab in which some slab -- any rank's -- holds fewer than L rows:
 *                           GS_ERR_UNSUPPORTED, on every rank alike.  In a multi-process context the call is collective, like
 *                           gs_run, and every rank receives the counts of the global grid.
 *   gs_members_correlation  the same layout with i = 2 m + s for species s (0 = U with thresholds[j] and above[0]; 1 = V with
 *                           thresholds[nt + j] and above[1]) of member first + m, m < count, from the newest slot: one launch,
 *                           one copy.  A member is a plane of its own: nothing is above it, its neighbours' rows are never seen.
 * Both block and have no side effects (ghost rows, tuner, graphs and gs_stats are left as they are).  GS_ERR_INVALID: a null
 * argument, nt outside 1..4, a NaN threshold or max_lag outside 1..64 -- decided in this order before any handle is looked
 * at --, a null or foreign handle, mixed shapes, n outside 1..4, members outside the ensemble.
 * Not done: pairs wrapped under the periodic rule; the full 2-D lag window and lags beyond 64; real-valued autocorrelation;
 * cross-correlation of U with V; slabs shorter than L. */
int32_t gs_fields_correlation(gs_ctx *ctx, gs_field *const *fields, int32_t n, const float *thresholds, const int32_t *above,
                              int32_t nt, int32_t max_lag, uint64_t *out);
int32_t gs_members_correlation(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const float *thresholds,
                               const int32_t above[2], int32_t nt, int32_t max_lag, uint64_t *out);

/* Power spectra computed on the device: the tile-averaged structure factor of one plane of the WHOLE global grid -- from it the
 * pattern's wavelength with sub-cell resolution and the orientation of stripes at any angle, with no threshold -- without
 * downloading the plane.  For a plane x of R x C cells, a tile size T of 16, 32, 64 or 128 and window = 0 (none) or 1
 * (periodic Hann):
 *   - TILES are T x T cells, do not overlap and are anchored at global row 0 and column 0: band b is rows [b T, (b + 1) T),
 *     tile (b, j) columns [j T, (j + 1) T) of band b.  Only tiles wholly inside the grid exist, floor(R / T) floor(C / T) of
 *     them; the remaining rows and columns are not looked at.  Nothing wraps, under any boundary rule.
 *   - TABLES, formed by the host in f64 and rounded to f32, handed out by gs_spectrum_tables (which needs no device):
 *     h[j] = 0.5 - 0.5 cos(2 pi j / T), j < T, and W[k] = (cos(2 pi k / T), -sin(2 pi k / T)), k < T / 2.
 *   - PER TILE, every f32 operation rounded on its own, no fused multiply-add:
 *       1. a tile that holds a NaN or an infinity adds nothing and counts as skipped;
 *       2. the mean: the cells added as f64, each row halved repeatedly -- p[0:T/2] + p[T/2:T], and so on down to one value --,
 *          the T row sums halved likewise, m = (float)(sum / (double)(T T));
 *       3. y = x - m in f32 and, with the window, y = (y h[r]) h[c];
 *       4. every row, as complex numbers with zero imaginary part, through a radix-2 decimation-in-time transform: the input
 *          permuted by bit reversal, then log2 T stages with half-sizes h = 1, 2, 4, ...; a butterfly with a = X[i],
 *          b = X[i + h] and w = W[(i mod h) T / (2 h)] forms t = (b.re w.re - b.im w.im, b.re w.im + b.im w.re), then
 *          X[i] = a + t and X[i + h] = a - t;
 *       5. columns 0 .. T/2 of the result through the same transform along the rows' axis;
 *       6. p[kr][kc] = re re + im im in f32, kr < T, kc <= T/2.
 *   - THE FOLD, a function of (R, C, T) alone: a segment is up to 16 consecutive tiles [16 s, 16 s + 16) of one band, and its
 *     record adds its tiles' p, as f64, one after another in ascending tile order from +0.0; a band's sum adds its segments'
 *     records in ascending order from +0.0; the plane's result adds the band sums in ascending global band order from +0.0.
 * The result is power[T][T/2 + 1] as f64, the raw sums -- the hosts do all normalisation (the mean over the tiles used, the
 * window's energy, the radial average) --, and tiles[2] = {used, skipped}.  Sub-normal values are kept; overflow inside a
 * tile propagates by IEEE rules.  A grid smaller than T on a side: GS_OK, all zeros.  The bits are the same for any slab
 * count, process count or step kernel, and a member's are those of a lone Species in the same state.
 *   gs_spectrum_tables   window[T] and twiddle[T / 2 pairs (re, im)] as above; either may be null.
 *   gs_fields_spectrum   power[(i T + kr) (T/2 + 1) + kc] and tiles[2 i ..] for fields[i], i < n (1..4 fields of one shape):
 *                        one wait for enqueued work (as gs_fields_summarize), per slab one launch over its segments and one
 *                        that adds them per band; the host adds the bands.  A context in which some slab -- any rank's --
 *                        begins at a row that is not a multiple of T: GS_ERR_UNSUPPORTED, on every rank alike.  In a
 *                        multi-process context the call is collective, like gs_run, and every rank receives the global result.
 *   gs_members_spectrum  the same layout with i = 2 m + s for species s of member first + m, m < count, from the newest slot:
 *                        one launch over every member's segments.  Retired members are read like any other.
 * Both block and have no side effects (ghost rows, tuner, graphs and gs_stats are left as they are).  GS_ERR_INVALID: a tile
 * or window outside the sets above or a null output -- decided before any handle is looked at --, a null or foreign handle,
 * mixed shapes, n outside 1..4, members outside the ensemble.
 * Not done: the cross-spectrum of U with V; overlapping tiles; tiles that wrap.
 * (For per-region spectra see gs_fields_region_spectrum, below.) */
int32_t gs_spectrum_tables(int32_t tile, float *window, float *twiddle);
int32_t gs_fields_spectrum(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t tile, int32_t window, double *power,
                           uint64_t *tiles);
int32_t gs_members_spectrum(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, int32_t tile, int32_t window,
                            double *power, uint64_t *tiles);

/* Connected components computed on the device: how many spots one plane of the WHOLE global grid has after thresholding, and
 * how large they are -- what the bit quads cannot say, which give only components - holes -- without downloading the plane.
 * For a plane x of R x C cells, a threshold t, a sense `above` and a connectivity of 4 or 8:
 *   - a cell is SET by morphology's rule: iff x > t (above != 0) or x < t (above == 0), one f32 comparison.  A NaN cell is
 *     never set, a cell equal to t is not set, infinities compare as they do, a sub-normal cell is the value it is (never
 *     flushed);
 *   - two set cells are neighbours when they share a side, under connectivity 8 also when they share a corner; a component is
 *     a largest set of set cells joined by chains of neighbours.  Components NEVER wrap, under every boundary rule, as
 *     morphology's quads and correlation's pairs never do: a spot across a periodic edge counts as two;
 *   - the result counts the components, adds up and bins their sizes (cells) and names the largest.  An empty plane (R = 0 or
 *     C = 0): GS_OK, all zeros.
 * What the hosts derive: the mean size set_cells / components, the largest's share largest / set_cells, and with
 * morphology's Euler number of the same threshold and sense the holes: components - euler8 (connectivity 8) or - euler4 (4).
 * All fields are integers, and the same bits for any slab count, process count, step kernel or launch shape; a member's
 * result is that of a lone Species in the same state.
 *   gs_fields_components   out[i * nt + k] for fields[i] thresholded at thresholds[i * nt + k] with the sense above[i], i < n
 *                          (1..4 fields of one shape), k < nt (1..4 thresholds per field): one wait for enqueued work (as
 *                          gs_fields_summarize: a persistent window launch that gave up is run again first); then every
 *                          (field, threshold) is labelled one after the other, slab by slab on the slab's compute stream.  A
 *                          slab labels its own rows as if it were alone and hands the (root, size) of its first and last row
 *                          to the host, which joins the components that meet across the seams; ghost rows are never read.  In
 *                          a multi-process context the call is collective, like gs_run: every rank's seam rows and counters
 *                          travel to every rank, and every rank does the same merge.
 *   gs_members_components  out[(2 i + s) * nt + k] for species s (0 = U with thresholds[k] and above[0]; 1 = V with
 *                          thresholds[nt + k] and above[1]) of member first + i, i < count, from the newest slot (a retired
 *                          member: its held state).  A member is a plane of its own: it never joins its neighbours' rows.
 * Label memory: a u32 parent and a u32 size per cell, 8 bytes per cell of the slab (2 GiB at 16384 x 16384) or of the batch of
 * members being labelled, allocated for the call and freed before it returns; every (plane, threshold) is labelled in the
 * same memory.  Members are labelled in batches of as many whole members as fit GS_COMPONENTS_BATCH_BYTES of label memory (at
 * least one).
 * Both block and have no side effects (ghost rows, tuner, graphs and gs_stats are left as they are).  GS_ERR_INVALID, decided
 * in this order before any handle is looked at: a null argument, nt outside 1..4, a NaN threshold, a connectivity that is
 * neither 4 nor 8; then a null or foreign handle, mixed shapes, n outside 1..4, members outside the ensemble.
 * GS_ERR_UNSUPPORTED: a slab (or a member) of 2^32 cells or more -- labels are 32-bit.  GS_ERR_NOMEM: the label memory cannot
 * be had; nothing is changed.  In a multi-process context the ranks agree on that verdict before anything else travels: if
 * one rank cannot have its memory, every rank returns GS_ERR_NOMEM.
 * Not done: components wrapped under the periodic rule; label planes for the caller.  (Centroids and bounding boxes: the
 * component lists below.) */
#define GS_COMPONENTS_BATCH_BYTES (256u << 20)
typedef struct gs_components {
    uint64_t components;  /* connected components of set cells                                   */
    uint64_t set_cells;   /* sum of their sizes: morphology's area A                             */
    uint64_t largest;     /* cells of the largest one; 0 when there is none                      */
    uint64_t by_size[32]; /* by_size[b]: components with 2^b <= size < 2^(b+1); b = 31 also takes */
} gs_components;          /*             every larger one.  280 bytes                            */
int32_t gs_fields_components(gs_ctx *ctx, gs_field *const *fields, int32_t n, const float *thresholds, const int32_t *above,
                             int32_t nt, int32_t connectivity, gs_components *out);
int32_t gs_members_components(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, const float *thresholds,
                              const int32_t above[2], int32_t nt, int32_t connectivity, gs_components *out);

/* Regional connected components: the result of gs_fields_components of every region of the region grid of the regional
 * observables above (gs_region_grid) -- how many spots each part of a parameter map's grid holds, how large they are and
 * whether one component percolates its region (largest / set_cells), which a region's Euler number (components - holes)
 * cannot say.  A whole-grid call on a mapped grid blends the regions: the spots of neighbouring regions join across borders.
 *   gs_fields_region_components  out[((p * RR + i) * RC + j) * nt + k] is the result of region (i, j) of fields[p]
 *                                thresholded at thresholds[p * nt + k] with the sense above[p] and, bit for bit, what
 *                                gs_fields_components returns for a field that holds that region's cells alone, with the
 *                                same threshold, sense and connectivity.
 * A region's border is a WALL: two set cells in different regions are never neighbours, neither across a side nor across a
 * corner, under every boundary rule; a spot that straddles a border counts once in every region it touches.  So over the
 * regions set_cells sums to the whole grid's set_cells, the sum of components is at least the whole grid's, and with
 * rh >= R and rw >= C (one region) the result is gs_fields_components' own.  The set rule is morphology's, word for word (a NaN
 * cell and a cell equal to the threshold are not set, a sub-normal cell is the value it is); with a domain mask attached
 * wall cells count.  All counters are integers: the same bits for any slab count, process count, step kernel or launch
 * shape.
 * A slab is labelled in place as gs_fields_components labels it, in label memory of 8 bytes per cell of the slab that lives
 * for the call alone, with the regions' borders as walls; every component adds itself to the counters of its region.  A
 * region lies inside one slab, so nothing is joined on the host.
 * The call follows its four twins above: one wait for enqueued work (a window launch that gave up is run again first),
 * blocking, no side effects (ghost rows, tuner, graphs and gs_stats are left as they are), collective in a multi-process
 * context with every rank receiving every region; an empty plane: GS_OK, nothing is written.  GS_ERR_INVALID, decided in
 * this order: a null argument; rh or rw refused by gs_region_grid; nt outside 1..4; a NaN threshold; a connectivity that is
 * neither 4 nor 8 -- all before any handle is looked at --; a null or foreign handle, mixed shapes, n outside 1..4; RR RC >
 * GS_REGIONS_MAX; RR RC nt > GS_REGION_COMPONENTS_MAX records per field (a cap on result memory: 280 MiB per field).
 * GS_ERR_UNSUPPORTED, on every rank alike: some slab begins at a row that is no multiple of rh, as above; a slab of 2^32
 * cells or more.  GS_ERR_NOMEM: as gs_fields_components returns it; in a multi-process context the ranks agree on it before
 * anything else travels.
 * Not done: regions of ensemble members; regions that straddle slabs; regional component lists. */
#define GS_REGION_COMPONENTS_MAX (1u << 20)
int32_t gs_fields_region_components(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw,
                                    const float *thresholds, const int32_t *above, int32_t nt, int32_t connectivity,
                                    gs_components *out);

/* Component lists computed on the device: WHERE the spots of one plane of the WHOLE global grid are after thresholding -- one
 * record per connected component with its size, the sums of its cells' coordinates (the centroid), its first cell and its
 * bounding box -- without downloading the plane: whether a spot pattern is a lattice (distances between centroids), whether
 * the spots move from one sample to the next, how elongated a component is, which ones touch the edge of the domain.
 * For a plane x of R x C cells, a threshold t, a sense `above`, a connectivity of 4 or 8 and a min_size >= 1:
 *   - cells are SET and joined into components exactly by the rule of gs_fields_components: a NaN cell is never set, a cell
 *     equal to t is not set, a sub-normal cell is the value it is, and components NEVER wrap, under every boundary rule;
 *   - every component of at least min_size cells is LISTED as one gs_component_record.  Rows of a field are rows of the whole
 *     global grid, rows of a member are the member's own.  The centroid is (sum_row / size, sum_col / size); the first cell
 *     is the component's first in row-major order;
 *   - within a plane the records are in ascending (first_row, first_col) order -- the order in which a row-major labelling
 *     (scipy.ndimage.label) numbers components.
 * The result is integers only: the same bits for any slab count, step kernel or launch shape, and for a member and a lone
 * Species in the same state.  With min_size = 1 the list agrees with gs_fields_components for the same arguments: the number
 * of records is `components`, the sizes add up to `set_cells`, their maximum is `largest`, their floor(log2) bins are `by_size`.
 * An empty plane (R = 0 or C = 0, or no cell set): GS_OK and a list without records.
 *   gs_field_component_list    one plane; the list has 1 plane.  One wait for enqueued work (as gs_fields_components), then
 *                              slab by slab on the slab's compute stream: the labelling of gs_fields_components, then the
 *                              components to list are counted -- in a slab chain those that touch a slab's first or last row
 *                              are listed whatever their size, because min_size can only be applied after the seam merge --,
 *                              the count is read back once, the records are written in first-cell order and every set cell
 *                              adds its coordinates to its record (integer atomics, one set per run of cells).  The host
 *                              makes the rows global, joins the records that meet across the seams (sizes and sums added, the
 *                              boxes united, the first cell the smallest), applies min_size and orders by first cell; ghost
 *                              rows are never read.
 *   gs_members_component_list  species (0 = U, 1 = V) of members first .. first + count - 1 from the newest slot (a retired
 *                              member: its held state); the list has `count` planes.  A member is a plane of its own: it never
 *                              joins its neighbours' rows.  Members are labelled in the batches of gs_members_components.
 *   gs_component_list_view     *planes, and the records of plane i: records[offsets[i] .. offsets[i + 1]); offsets has
 *                              planes + 1 entries.  The pointers stay valid until the list is destroyed.
 *   gs_component_list_destroy  frees the list; NULL: GS_OK.  A list is host memory owned by the library and independent of the
 *                              context: it may outlive it.
 * Label memory: as for gs_fields_components, 8 bytes per cell of the slab or batch -- the u32 size of a root is replaced by
 * its record's index once the record holds the size --, in a slab chain 1 bit per cell more (the marks of the components that
 * touch a seam row), and 48 bytes per record; all allocated for the call and freed before it returns.  One u32 per 256 cells of
 * the slab's scratch buffer holds the counts.
 * Both calls block like gs_fields_components (one wait for enqueued work, then the slabs' compute streams) and have no side
 * effects (ghost rows, tuner, graphs and gs_stats are left as they are).  GS_ERR_INVALID, decided in this order: a null
 * argument (ctx, out), a NaN threshold, a connectivity that is neither 4 nor 8, min_size == 0, a species outside 0..1 --
 * all before any handle is looked at --; then a null or foreign handle, members outside the ensemble.  GS_ERR_UNSUPPORTED: a
 * slab or a batch of members of 2^32 cells or more; a grid for which a sum could overflow, rows * rows * cols or
 * rows * cols * cols >= 2^64; a multi-process context (world > 1) -- every rank reaches that verdict alone, before anything
 * is allocated or sent: exchanging record lists of variable length between ranks is a follow-up.  GS_ERR_NOMEM: label or
 * record memory cannot be had; nothing is changed and no list is returned.  On any refusal *out is left as it was.
 * Not done: multi-process contexts; components wrapped under the periodic rule; label planes for the caller;
 * intensity-weighted centroids or any float accumulation; several thresholds or fields in one call.  (What became of the
 * spots between two states: gs_fields_match below.) */
typedef struct gs_component_record {
    uint64_t size;                               /* cells                                                              */
    uint64_t sum_row, sum_col;                   /* sums of the cells' row / column indices: centroid = sum / size    */
    uint32_t first_row, first_col;               /* its first cell in row-major order                                  */
    uint32_t row_min, row_max, col_min, col_max; /* bounding box, inclusive                                            */
} gs_component_record;                           /* 48 bytes, all integers */
typedef struct gs_component_list gs_component_list; /* host memory owned by the library, independent of the context */
int32_t gs_field_component_list(gs_ctx *ctx, gs_field *f, float threshold, int32_t above, int32_t connectivity, uint64_t min_size,
                                gs_component_list **out);
int32_t gs_members_component_list(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, int32_t species, float threshold,
                                  int32_t above, int32_t connectivity, uint64_t min_size, gs_component_list **out);
int32_t gs_component_list_view(const gs_component_list *list, uint64_t *planes, const uint64_t **offsets,
                               const gs_component_record **records);
int32_t gs_component_list_destroy(gs_component_list *list);

/* Component matching computed on the device: WHAT BECAME of the spots between two states -- which ones continued, split,
 * merged, were born or died, and how far the continuing ones moved -- without downloading either plane.  Two planes of one
 * shape, `before` (a snapshot's plane, say: gs_fields_copy) and `after`, and ONE rule for both: threshold, above, connectivity
 * 4 or 8, min_size >= 1, exactly as in gs_field_component_list (a NaN cell is never set, a cell equal to the threshold is not
 * set, a sub-normal cell is the value it is, components never wrap).
 *   - the match holds the component list of `before` and that of `after`: each equals, record for record, what
 *     gs_field_component_list (gs_members_component_list) returns for that plane and rule;
 *   - an OVERLAP is (before, after, cells): the index of a record in before's list within its plane, the index of a record in
 *     after's list, and cells >= 1, the number of grid cells set in both planes that belong to both components;
 *   - every pair of listed components that shares at least one cell appears exactly once; within a plane the overlaps are in
 *     ascending (before, after) order.  A component below min_size is in neither list and in no overlap;
 *   - with min_size 1 the cells of all overlaps add up to the number of cells set in both planes; the overlaps of one record
 *     add up to at most its size.  before == after (the same handle) is allowed: its overlaps are (i, i, size_i).
 * Integers only: the same bits for any slab count, step kernel or launch shape, and for a member and a lone Species.
 *   gs_fields_match          one pair of planes of this context and one shape; the match has 1 plane.  One wait for enqueued
 *                            work, then slab by slab on the slab's compute stream: `before` labelled and counted, `after`
 *                            labelled and counted, each in label memory of its own; the PIECES -- the cells set in both --
 *                            labelled from the two label arrays under the same connectivity (a connected piece lies inside
 *                            exactly one component of each plane) and counted; the three counts are read back once; the
 *                            records are written and one overlap per piece, which names its two records through the piece's
 *                            first cell.  The host makes rows and indices global, joins what crosses the seams as the lists
 *                            do, drops the pairs of which a partner fell below min_size, sorts, and adds the cells of equal
 *                            pairs: two pieces of one pair, and pieces cut by a seam, become one overlap.
 *   gs_members_match         species (0 = U, 1 = V) of member first + i of `after` against member first + i of `before`, i <
 *                            count, each from its ensemble's newest slot (a retired member: its held state) -- the pairing of
 *                            gs_members_compare; the match has `count` planes.  Both ensembles belong to this context and
 *                            have one shape and member count; before == after is allowed.  Members go in batches of whole
 *                            members such that each of the three labellings stays within GS_COMPONENTS_BATCH_BYTES.
 *   gs_component_match_view  the two lists -- ordinary gs_component_lists OWNED BY THE MATCH: gs_component_list_view works
 *                            on them, they die with the match and must not be destroyed --, *planes, and the overlaps of
 *                            plane i: overlaps[offsets[i] .. offsets[i + 1]); offsets has planes + 1 entries.  The pointers
 *                            stay valid until the match is destroyed.
 *   gs_component_match_destroy  frees the match and its lists; NULL: GS_OK.  Host memory owned by the library, independent of
 *                            the context: it may outlive it.
 * Label memory: 24 bytes per cell of the slab or batch (three labellings of 8), in a slab chain 1 bit per cell more for each
 * of the two lists, 48 bytes per record and 16 per piece; all allocated for the call and freed before it returns, however it
 * returns.  Three u32 per 256 cells of the slab's scratch buffer hold the counts.
 * Both calls block like the list calls (one wait for enqueued work, then the slabs' compute streams) and have no side effects
 * (ghost rows, tuner, graphs and gs_stats are left as they are).  GS_ERR_INVALID, decided in this order: a null argument (ctx,
 * out), a NaN threshold, a connectivity that is neither 4 nor 8, min_size == 0, a species outside 0..1 -- all before any
 * handle is looked at --; then a null or foreign handle, planes of different shapes, members outside the ensemble.
 * GS_ERR_UNSUPPORTED: a multi-process context (world > 1) -- every rank reaches that verdict alone, before anything is
 * allocated or sent --; a slab or a batch of members of 2^32 cells or more; the lists' sum-overflow shapes.  GS_ERR_NOMEM:
 * label or record memory cannot be had; nothing is changed and no match is returned.  On any refusal *out is left as it was.
 * Not done: multi-process contexts; wrapped components; matching by distance where nothing overlaps; tracks over more than
 * two states; float-weighted overlaps. */
typedef struct gs_component_overlap {
    uint32_t before, after; /* record indices within the plane's two lists      */
    uint64_t cells;         /* cells set in both planes that belong to both     */
} gs_component_overlap;     /* 16 bytes */
typedef struct gs_component_match gs_component_match; /* host memory owned by the library, independent of the context */
int32_t gs_fields_match(gs_ctx *ctx, gs_field *before, gs_field *after, float threshold, int32_t above, int32_t connectivity,
                        uint64_t min_size, gs_component_match **out);
int32_t gs_members_match(gs_ctx *ctx, gs_ensemble *before, gs_ensemble *after, uint64_t first, uint64_t count, int32_t species,
                         float threshold, int32_t above, int32_t connectivity, uint64_t min_size, gs_component_match **out);
int32_t gs_component_match_view(const gs_component_match *match, const gs_component_list **before, const gs_component_list **after,
                                uint64_t *planes, const uint64_t **offsets, const gs_component_overlap **overlaps);
int32_t gs_component_match_destroy(gs_component_match *match);

/* Two states compared on the device: how far one plane of the WHOLE global grid is from another of the same shape -- "has
 * this run stopped changing?" -- without downloading either, and the device copies that give a state to compare with
 * (snapshots) or to go back to (restores).
 *
 * The difference.  Per cell, d = (double)a - (double)b: ONE f64 subtraction of the two f32 cells, rounded to nearest even
 * (exact unless the exponents lie more than about 29 binades apart).  |d| is exact; d * d is one f64 multiplication, which
 * cannot overflow for f32 inputs.  Sub-normal cells count as the values they are (never flushed).
 * Comparable cells.  A cell is comparable when a AND b are finite there.  Any other cell (NaN or +-inf in either) counts in
 * `nonfinite` and adds +0.0 to the sums and nothing to the maximum.
 * `differing` compares the cells' 32-bit patterns, over EVERY cell, comparable or not: differing == 0 means that the two
 * planes are memcmp-equal over their cells; +0 against -0 differs (with d = 0); two NaNs of one bit pattern do not differ,
 * two of different payloads do.
 * Fold order -- exactly the summaries', a function of (rows, cols) alone, so that the results are bit-reproducible whatever
 * the slab count, the process count, the step kernel or the call form, and a member's result is bit for bit that of two
 * lone Species in the same states:
 *   1. row partial: each of 64 lanes holds an f64 accumulator starting at +0.0; lane l adds, in this order, |d| (for
 *      sum_sq: d * d) of the cells at columns 256 k + 4 l + j for k = 0, 1, ... and j = 0..3.  A column >= cols or a cell
 *      that is not comparable adds nothing;
 *   2. lane combine: the 64 partials are halved repeatedly, p[0:32] + p[32:64], then p[0:16] + p[16:32], ... down to one;
 *   3. field fold: the row partials are added one after the other in f64, in ascending GLOBAL row order, from +0.0.
 * max_abs and the two counts are order-free.
 *   gs_fields_compare   out[i] for the pair (a[i], b[i]), i < n (1..4 pairs, all planes of one shape on this context, e.g. a
 *                       Species' U and V against a snapshot's).  a[i] == b[i] is allowed: all zeros.  One wait for enqueued
 *                       work (as gs_fields_summarize: a persistent window launch that gave up is run again first), one
 *                       launch per slab, one exchange.  In a multi-process context the call is collective, like gs_run,
 *                       and every rank receives the result of the global grid.
 *   gs_members_compare  out[2 i] (U) and out[2 i + 1] (V): member first + i of `e` against member first + i of `ref`, i <
 *                       count, each ensemble's newest slot.  `ref` is an ensemble of the same context, shape and member
 *                       count (e itself is allowed: all zeros).
 * Both block and have no side effects (ghost rows, tuner, graphs and gs_stats are left as they are).  An empty plane: all
 * zeros.
 *   gs_fields_copy      dst[i] receives the cells of src[i], i < n (1..4), device to device on the slabs' compute streams,
 *                       in the order of i.  Blocking (it waits for enqueued work first, then for the copies).  dst[i] is
 *                       left exactly as gs_field_upload leaves a plane: its ghost rows count as stale and the next gs_step /
 *                       gs_run (or gs_field_finalize) refreshes them, so a run that follows is right under every boundary
 *                       rule and slab layout.  In a multi-process context every process copies its own rows.
 *   gs_members_copy     members [first, first + count) of `src`'s newest slot into the same members of `dst`'s newest slot;
 *                       the other members, both parameter tables and src stay as they are.  Blocking.
 * GS_ERR_INVALID, all decided before any device work: a null or foreign handle, mixed shapes, n outside 1..4, members
 * outside the ensemble, ensembles of different shapes or member counts, dst[i] == src[i] (or dst == src), a field named
 * twice in dst. */
typedef struct gs_change {
    double   sum_abs;    /* sum of |d| over the comparable cells, in the summaries' fold order      */
    double   sum_sq;     /* sum of d * d over the same cells, same order                            */
    double   max_abs;    /* largest |d|; +0.0 when no cell is comparable                            */
    uint64_t differing;  /* cells whose 32 bits differ -- ALL cells, non-finite ones included       */
    uint64_t nonfinite;  /* cells where a or b is NaN or +-inf (they add nothing to the sums / max) */
} gs_change;             /* 40 bytes */
int32_t gs_fields_compare(gs_ctx *ctx, gs_field *const *a, gs_field *const *b, int32_t n, gs_change *out);
int32_t gs_members_compare(gs_ctx *ctx, gs_ensemble *e, gs_ensemble *ref, uint64_t first, uint64_t count, gs_change *out);
int32_t gs_fields_copy(gs_ctx *ctx, gs_field *const *dst, gs_field *const *src, int32_t n);
int32_t gs_members_copy(gs_ctx *ctx, gs_ensemble *dst, gs_ensemble *src, uint64_t first, uint64_t count);

/* Regional state comparison: the change of every REGION of the region grid of gs_region_grid (above) between two planes of one
 * shape -- which part of a parameter map's grid is steady, which pulsates, which is chaotic; the whole-grid comparison of such
 * a grid blends them into one number that belongs to none -- without downloading either plane.
 * The rule that defines every result is the regional family's: a region's result is, bit for bit, what gs_fields_compare
 * returns for two fields that hold exactly that region's cells.  That is: d = (double)a - (double)b, comparable cells,
 * `differing` and `nonfinite` as defined above; the summaries' fold order with columns counted from the region's FIRST
 * column -- lane l adds the region's columns 256 k + 4 l + j --; the halving lane combine, in which the lanes past the
 * region hold +0.0; the region's rows added in ascending order from +0.0.  max_abs and the two counts are order-free.
 * Ragged last rows and columns of regions are kept.  The results are the same bits for any slab count, process count, step
 * kernel, launch shape or route (below) and do not depend on the boundary rule; with a domain mask attached wall cells count.
 *   gs_fields_region_compare  out[p * RR RC + i RC + j] is the change of region (i, j) of the pair (a[p], b[p]), p < n (1..4
 *                             pairs, all planes of one shape on this context).  a[p] == b[p] is allowed: all zeros.
 * The call waits once for enqueued work (as gs_fields_summarize: a persistent window launch that gave up is run again first),
 * blocks, and has no side effects (ghost rows, tuner, graphs and gs_stats are left as they are).  In a multi-process context
 * it is collective, like gs_run, and every rank receives every region.  An empty plane: GS_OK, nothing is written.
 * Two routes compute the same bits, and the library chooses per slab from the slab's shape, the region shape and the device's
 * compute-unit count alone:
 *   wave     a wave takes a whole region (several narrow ones side by side in 256 columns) and adds its rows in registers:
 *            no memory but the result.  Chosen for many small regions.
 *   records  a wave takes a band of 16 rows of a region and leaves a 16-byte record per (row, region column); a second launch
 *            adds every region's records in row order.  Chosen where a wave per region would leave the device underfilled:
 *            a region at least 32 rows high AND fewer wave-route waves -- rows of the region grid x ceil(RC / s), s = the
 *            regions that fit side by side in 256 columns, 1 from rw = 256 -- than 4 per compute unit (one per SIMD: with
 *            that many the wave route measures faster, profiles/region_change.md).  Record memory, rows x RC x 16 bytes per pair and slab, comes from the context's
 *            scratch buffer; where one slab's would exceed GS_REGION_CHANGE_RECORDS_MAX bytes the call takes the wave route.
 * The environment variable GS_HIP_REGION_CHANGE_ROUTE, read at every call, forces a route for tests and measurements:
 * `records` (still subject to that cap), `wave`; unset or empty: the library's choice; anything else: GS_ERR_INVALID.
 * Refusals, all decided before any device work -- GS_ERR_INVALID, in this order: a null argument; an rh or rw that
 * gs_region_grid refuses (both decided before any handle is looked at); a null or foreign handle, mixed shapes, n outside
 * 1..4; RR RC > GS_REGIONS_MAX.  GS_ERR_UNSUPPORTED, on every rank alike: a context of several slabs or processes in which
 * some slab begins at a row that is no multiple of rh (a region lies inside one slab).
 * Not done: regions of ensemble members; regions that straddle slabs; ending a run early on the regions' verdict. */
#define GS_REGION_CHANGE_RECORDS_MAX (1ull << 28)
int32_t gs_fields_region_compare(gs_ctx *ctx, gs_field *const *a, gs_field *const *b, int32_t n, int32_t rh, int32_t rw,
                                 gs_change *out);

/* Regional power spectra: the tile-averaged structure factor of gs_fields_spectrum (above) of every REGION of the region grid
 * of gs_region_grid -- the wavelength, with sub-cell resolution and no threshold, and the orientation and anisotropy of the
 * stripes of each part of a parameter map's grid; the whole-grid spectrum of such a grid is a blend that belongs to no region.
 * For a region shape (rh, rw) that gs_region_grid accepts, a tile T of 16, 32, 64 or 128 and window 0 or 1, the rule is the
 * regional family's: a region's result is, bit for bit, what gs_fields_spectrum returns for a field that holds exactly that
 * region's cells.  That is:
 *   - tiles are anchored at the region's first row and first column; a region of h x w cells has floor(h / T) floor(w / T)
 *     tiles, its remaining rows and columns are not looked at (a NaN there changes nothing);
 *   - a tile with a cell that is not finite is skipped and counted, in its own region only;
 *   - the arithmetic per tile is gs_fields_spectrum's, word for word, with the same tables;
 *   - the fold is per region: a segment is up to 16 consecutive tiles of one band of the region, counted from the region's
 *     first tile, and its record adds its tiles' power in ascending tile order from +0.0; a band's sum adds its segments in
 *     ascending order from +0.0; the region's result adds its band sums in ascending order from +0.0;
 *   - a region in which no tile fits -- a ragged last region, or rh < T or rw < T -- gets zeros and {0, 0};
 *   - a region's border is a wall for tiles: no tile straddles two regions.  rh and rw need not be multiples of T.
 * The bits are the same for any slab count, process count, step kernel or launch shape and do not depend on the boundary
 * rule; with a domain mask attached wall cells count.  Where rh and rw are multiples of T the regions partition the whole
 * grid's tiles: the counts add up to gs_fields_spectrum's exactly, the power only to rounding (the fold orders differ).
 *   gs_fields_region_spectrum  power[(((p RR + i) RC + j) T + kr) (T/2 + 1) + kc], the raw f64 sums, and
 *                              tiles[((p RR + i) RC + j) 2 + {0: used, 1: skipped}] for region (i, j) of fields[p], p < n
 *                              (1..4 fields of one shape).
 * The call follows its regional twins: one wait for enqueued work (as gs_fields_summarize), per slab one launch over the
 * regions' segments and one that adds them per region -- the device finishes every region, the host adds nothing --, blocking,
 * no side effects (ghost rows, tuner, graphs and gs_stats are left as they are), collective in a multi-process context with
 * every rank receiving every region; an empty plane: GS_OK, nothing is written.  GS_ERR_INVALID, decided in this order: a null
 * output; a tile or window outside the sets above; rh or rw refused by gs_region_grid -- these three before any handle is
 * looked at --; a null or foreign handle, mixed shapes, n outside 1..4; RR RC > GS_REGIONS_MAX; RR RC (T (T/2 + 1) + 2) >
 * GS_REGION_SPECTRUM_MAX result words per field (a cap on result memory: 256 MiB per field); the words of segment records
 * over the n fields -- n times the sum over the regions of (bands of the region) (segments of a band of the region)
 * (T (T/2 + 1) + 2), computed from the global shape alone, so that every rank and every slab count reaches the same verdict
 * -- > GS_REGION_SPECTRUM_RECORDS_MAX (a cap on scratch memory: 1 GiB).  GS_ERR_UNSUPPORTED, on every rank alike: some slab
 * begins at a row that is no multiple of rh -- a region lies inside one slab, so nothing is staged and no ghost row is read;
 * there is no condition on T at the seams.
 * Not done: regions of ensemble members; regions that straddle slabs; overlapping tiles. */
#define GS_REGION_SPECTRUM_MAX (1u << 25)
#define GS_REGION_SPECTRUM_RECORDS_MAX (1ull << 27)
int32_t gs_fields_region_spectrum(gs_ctx *ctx, gs_field *const *fields, int32_t n, int32_t rh, int32_t rw, int32_t tile,
                                  int32_t window, double *power, uint64_t *tiles);

/* Time statistics formed on the device: per-cell accumulators over the SAMPLES of a run -- is a cell steady, pulsating or
 * chaotic (variance), what does the time-averaged field look like (mean), where has a spot been (maximum), when did the front
 * arrive (first crossing of a threshold), for what share of the time was a cell inside a spot (occupancy) -- without
 * downloading a frame.  A gs_time_stats follows 1..4 planes of one shape; each selected GROUP keeps accumulator planes per
 * plane, and one call adds one sample x of every cell, in this order:
 *   GS_TSTAT_SUM        sum (f64, reset +0.0):        sum = sum + (double)x
 *   GS_TSTAT_SQUARES    squares (f64, reset +0.0):    squares = squares + (double)x * (double)x   (the product is exact in f64)
 *   GS_TSTAT_EXTREMES   min, max (f32, reset +inf, -inf):   min = x < min ? x : min;  max = x > max ? x : max
 *   GS_TSTAT_CROSSINGS  set_count (u32, reset 0), first_stamp (u32, reset 0xffffffff): if x is SET by morphology's rule against
 *                       the plane's one threshold and sense (x > t, or x < t; one f32 comparison): set_count += 1, and
 *                       first_stamp = stamp where it still holds 0xffffffff
 * What follows: a NaN sample never replaces an extreme and is never set, but NaN and +-inf propagate into sum and squares --
 * the visible sign of a blow-up; a zero never replaces an extreme zero of the other sign (the comparisons are strict); a
 * sub-normal sample counts as the value it is; both sums are plain sequential f64 additions per cell, so any host restates
 * them bit for bit (the sign and payload of a NaN are not specified).  Every cell is independent: the accumulators are the
 * same bits for any slab count, process count, boundary rule or launch shape, and a member's are those of a lone Species
 * sampled in the same states.
 * Result planes (`which`), computed in f64 with every operation rounded once and converted to f32 at the end; n = samples:
 *   GS_TSTAT_MEAN       (float)(sum / n)
 *   GS_TSTAT_VARIANCE   d = squares / n - (sum / n) * (sum / n);  (float)(d > 0 ? d : 0), a NaN d stays NaN
 *   GS_TSTAT_MIN, _MAX  the accumulator
 *   GS_TSTAT_OCCUPANCY  (float)((double)set_count / n)
 *   GS_TSTAT_ARRIVAL    (float)first_stamp, -1.0f where the cell was never set
 * (no standard deviation is formed on the device: the hosts take the square root of what they read).
 *   gs_time_stats_create      accumulators for n planes of rows x cols cells (the GLOBAL shape of the fields it will follow),
 *                             one set per slab on that slab's device, rows of the fields' pitch, at their reset values.
 *                             thresholds[n] and above[n] (above[i] != 0: set above the threshold) are needed with
 *                             GS_TSTAT_CROSSINGS and ignored without.  No rank ever exchanges anything: the object works in
 *                             every context that has fields, with a parameter map or a domain mask attached too.
 *   gs_time_stats_accumulate  one sample of fields[0 .. n) (this context's, of the object's shape), stamped `stamp` (any u32
 *                             but 0xffffffff; the hosts pass the step count): waits for enqueued work as the other
 *                             observables do (a persistent window launch that gave up is run again first), enqueues one launch
 *                             per slab on its compute stream and returns.  The fields, their ghost rows, the tuner, the graphs
 *                             and gs_stats are left as they are.
 *   gs_time_stats_samples     *n = samples since creation or the last reset.
 *   gs_time_stats_result      result plane `which` of plane `plane` into `out` (this context's, of the object's shape), whose
 *                             ghost rows go stale as after gs_fields_copy: an ordinary field for every observable, reduced
 *                             download and colour map.
 *   gs_time_stats_download    raw accumulator `raw` of plane `plane` as dense [rows, cols] of its own type (f64, f32 or u32)
 *                             with the row coverage of gs_field_download: this process's rows.
 *   gs_time_stats_reset       back to the reset values, samples = 0.
 * result, download, reset and destroy wait for the enqueued samples before they act.  The object's memory is owned by its
 * context: gs_time_stats_destroy frees it early, gs_ctx_destroy frees whatever is left, and a handle is dead once its context is.
 * Ensembles: planes 0 / 1 = U / V of members [first, first + count) of an ensemble shaped like `like`, sampled from the newest
 * slot whether active or retired (a retired member repeats its state).
 *   gs_members_time_stats_create      thresholds[2] / above[2]: U's, V's.
 *   gs_members_time_stats_accumulate  one sample of the object's members of `e` (this context's, shaped like `like`).
 *   gs_members_time_stats_result      host[i * rows * cols ...] = result plane `which` of species `species` of member first + i.
 * samples, download (dense [count * rows, cols]), reset and destroy are the calls above.
 * GS_ERR_INVALID, decided before anything is allocated or launched: a null argument; groups 0 or with unknown bits;
 * GS_TSTAT_CROSSINGS without thresholds, or a NaN threshold; n outside 1..4; fields of another context or shape, or another
 * count than the object's; stamp == 0xffffffff; a `which` or `raw` whose group is not selected, or a plane outside the
 * object's; a result before the first sample; members outside the ensemble; an object of the other form.  An ensemble on a
 * context that refuses ensembles: that context's own error (GS_ERR_UNSUPPORTED).  An allocation failure: GS_ERR_NOMEM (or
 * GS_ERR_HIP), and nothing is left behind. */
#define GS_TSTAT_SUM 1u
#define GS_TSTAT_SQUARES 2u
#define GS_TSTAT_EXTREMES 4u
#define GS_TSTAT_CROSSINGS 8u
enum { GS_TSTAT_MEAN = 0, GS_TSTAT_VARIANCE = 1, GS_TSTAT_MIN = 2, GS_TSTAT_MAX = 3, GS_TSTAT_OCCUPANCY = 4, GS_TSTAT_ARRIVAL = 5 };
enum { GS_TSTAT_RAW_SUM = 0, GS_TSTAT_RAW_SQUARES = 1, GS_TSTAT_RAW_MIN = 2, GS_TSTAT_RAW_MAX = 3, GS_TSTAT_RAW_SET_COUNT = 4,
       GS_TSTAT_RAW_FIRST_STAMP = 5 };
typedef struct gs_time_stats gs_time_stats; /* device memory owned by the context */
int32_t gs_time_stats_create(gs_ctx *ctx, gs_time_stats **out, uint64_t rows, uint64_t cols, int32_t n, uint32_t groups,
                             const float *thresholds, const int32_t *above);
int32_t gs_time_stats_destroy(gs_ctx *ctx, gs_time_stats *ts);
int32_t gs_time_stats_reset(gs_ctx *ctx, gs_time_stats *ts);
int32_t gs_time_stats_accumulate(gs_ctx *ctx, gs_time_stats *ts, gs_field *const *fields, int32_t n, uint32_t stamp);
int32_t gs_time_stats_samples(const gs_time_stats *ts, uint64_t *n);
int32_t gs_time_stats_result(gs_ctx *ctx, gs_time_stats *ts, int32_t plane, int32_t which, gs_field *out);
int32_t gs_time_stats_download(gs_ctx *ctx, gs_time_stats *ts, int32_t plane, int32_t raw, void *host);
int32_t gs_members_time_stats_create(gs_ctx *ctx, gs_time_stats **out, gs_ensemble *like, uint64_t first, uint64_t count,
                                     uint32_t groups, const float thresholds[2], const int32_t above[2]);
int32_t gs_members_time_stats_accumulate(gs_ctx *ctx, gs_time_stats *ts, gs_ensemble *e, uint32_t stamp);
int32_t gs_members_time_stats_result(gs_ctx *ctx, gs_time_stats *ts, int32_t species, int32_t which, float *host);

/* Bundle statistics: per-cell statistics ACROSS ensemble members, formed on the device in one pass -- the ensemble average
 * of R realisations of one parameter point (mean), the spread between them (variance), the envelope (min, max) and the
 * probability that a cell lies inside a spot, P(V > t) (occupancy) -- without downloading a member.
 * Members [first, first + count) of `e` form count / span BUNDLES: bundle b holds members first + b span + j, j < span.
 * For every bundle, species (U, V) and cell the accumulators are those of the time statistics above, member j in the place
 * of sample j, visited in ascending j:
 *   sum (f64, from +0.0):        sum = sum + (double)x
 *   squares (f64, from +0.0):    squares = squares + (double)x * (double)x
 *   min, max (f32, from +inf, -inf):   min = x < min ? x : min;  max = x > max ? x : max   (strict: a NaN never replaces an
 *                                extreme, nor does a zero one of the other sign)
 *   set_count (u32, from 0):     + 1 where x is SET by morphology's rule against the species' threshold and sense (x > t, or
 *                                x < t; one f32 comparison)
 * Both sums are plain sequential f64 additions in member order, and that order is the contract: a span is never split over
 * lanes, waves or launches and added up again.  A sub-normal value counts as the value it is.
 * Result planes use the GS_TSTAT_* codes and the formulas of gs_time_stats_result with n = span -- GS_TSTAT_MEAN, _VARIANCE,
 * _MIN, _MAX, _OCCUPANCY; each in f64 with every operation rounded once, converted to f32 at the end.  GS_TSTAT_ARRIVAL has
 * no meaning across members.  It follows: a bundle's result is bit for bit (the sign and payload of a NaN aside) the time
 * statistics of a lone Species, or of a one-member ensemble, sampled through the bundle's members' states in ascending order.
 *   gs_members_bundle_stats  which[0 .. n): n distinct result codes, n in 1..5.  Result which[i] of bundle b is written into
 *                            member out_first + b of out[i]: its U plane from the members' U, its V plane from their V.
 *                            It is written as gs_members_copy writes a member: into the newest slot, and an inactive member
 *                            of out[i] is mirrored into its other slot before out[i]'s next run.  Active flags, step counts,
 *                            parameters and noise of out[i] are untouched, and its other members keep their bits: out[i] is
 *                            an ordinary ensemble for every observable above.  thresholds[2] / above[2] are U's and V's;
 *                            they are needed with GS_TSTAT_OCCUPANCY and ignored (may be null) without it.  Members are
 *                            read from the newest slot whether active or retired, as the time statistics read them.
 * The call waits for enqueued work as the other member observables do, blocks, and has no side effects on the tuner, the
 * graphs or gs_stats.  count == 0: GS_OK, nothing is written.
 * GS_ERR_INVALID, decided in this order before anything is launched: a null argument; span == 0, or count no multiple of
 * span; members outside `e`; n outside 1..5; an unknown or repeated code, or GS_TSTAT_ARRIVAL; the occupancy without
 * thresholds, or a NaN threshold; an out[i] that is null, `e` itself, named twice, of another context or shape, or with
 * fewer than out_first + count / span members.  A context that refuses ensembles: that context's own error
 * (GS_ERR_UNSUPPORTED).
 * Not done: bundles of members that are not consecutive; weights per member; a bundle's accumulators for the caller; medians
 * and other quantiles.  One bundle of tiny members with a huge span is one lane per four cells by contract, and is slow: the
 * parallelism is cells x bundles, never the span. */
int32_t gs_members_bundle_stats(gs_ctx *ctx, gs_ensemble *e, uint64_t first, uint64_t count, uint64_t span, const int32_t *which,
                                int32_t n, const float thresholds[2], const int32_t above[2], gs_ensemble *const *out,
                                uint64_t out_first);

/* Measurement hook, not for bindings (tools/rccl_under_load.py): the ghost-row exchange's transport on ONE GPU while the
 * caller keeps the chip busy or idle.  mode 0: a one-rank RCCL communicator, `messages` ncclSend / ncclRecv pairs of
 * `floats` f32 to itself in one group; mode 1: the same bytes as device-to-device copies (the in-process chain's route);
 * both on a high-priority stream created like a slab's halo stream.  _run enqueues one exchange and waits for it:
 * host_ms from the first enqueue to the end of the wait, device_ms between events around it on its stream. */
typedef struct gs_exchange_probe gs_exchange_probe;
int32_t gs_debug_exchange_probe_create(int32_t device, int32_t mode, int32_t messages, uint64_t floats, gs_exchange_probe **out);
int32_t gs_debug_exchange_probe_run(gs_exchange_probe *p, float *host_ms, float *device_ms);
int32_t gs_debug_exchange_probe_destroy(gs_exchange_probe *p);
/* Introspection for the bench and the tests, not for bindings: what gs_fields_place has done on this context so far --
 * pair probes timed and extra blocks drawn (each of the planes' size; all freed or handed to planes by now). */
int32_t gs_debug_place_stats(const gs_ctx *ctx, uint64_t *probes, uint64_t *blocks_drawn);
/* Test hook, not for bindings: the key of the table that remembers on which (device, kernel entry) more than 64 KB
 * of dynamic LDS were opted into -- 1 when (device, slot, bytes) is new (and is recorded), 0 when a launch on that
 * device would skip the opt-in, -1 for a bad slot (tests/test_capi_cpu.py). */
int32_t gs_debug_dyn_lds_key(int32_t device, int32_t slot, int32_t bytes);
/* Test hook, not for bindings: the tiling GS_KERNEL_WINDOW would use for a grid on a device of `compute_units` CUs (no
 * device needed).  Returns the number of windows (0: the grid is not one round of windows) and writes up to cap_windows
 * descriptors of 6 + 14 int32 each: first owned row, first owned column, owned rows, owned columns, window rows in use,
 * number of neighbours, neighbour indices. */
int32_t gs_debug_window_plan(uint64_t rows, uint64_t cols, int32_t compute_units, int32_t boundary, int32_t cheap_edge_kinds,
                             int32_t window_rows, int32_t k, int32_t *out, int32_t cap_windows, int32_t *rows_per_wave, int32_t *k_out);

#ifdef __cplusplus
}
#endif
#endif /* GS_HIP_H */
