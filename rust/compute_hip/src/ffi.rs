//! `extern "C"` view of include/gs_hip.h (ABI version 4).  Field order and widths must match
//! the header exactly; `tests/test_capi_cpu.py::test_struct_layouts` pins the C side.
#![allow(non_camel_case_types)]

use std::os::raw::{c_char, c_void};

pub const GS_OK: i32 = 0;
pub const GS_UNIQUE_ID_BYTES: usize = 128;

#[repr(C)]
#[derive(Copy, Clone, Debug)]
pub struct gs_params {
    pub w: [[f32; 3]; 3],
    pub du: f32,
    pub dv: f32,
    pub feed: f32,
    pub kill: f32,
    pub dt: f32,
}

#[repr(C)]
#[derive(Copy, Clone, Debug, Default)]
pub struct gs_options {
    pub math: i32,
    pub kernel: i32,
    pub rows_per_block: i32,
    pub fuse_steps: i32,
    pub use_graph: i32,
    pub pitch_pad: i32,
    pub split: i32,
    pub general_kernels: i32,
    pub cols_per_lane: i32,
    pub boundary: i32,
    pub no_tune: i32,
    pub tile_shape: i32,
    pub share_taps: i32,
    pub reserved: [i32; 3],
}

#[repr(C)]
pub struct gs_ctx {
    _private: [u8; 0],
}
#[repr(C)]
pub struct gs_field {
    _private: [u8; 0],
}
#[repr(C)]
pub struct gs_ensemble {
    _private: [u8; 0],
}

/// A component list owned by the library (of a `gs_component_match` here: it dies with the match).
#[repr(C)]
pub struct gs_component_list {
    _private: [u8; 0],
}
/// What `gs_fields_match` / `gs_members_match` return: host memory owned by the library.
#[repr(C)]
pub struct gs_component_match {
    _private: [u8; 0],
}

/// Time statistics (include/gs_hip.h): per-cell accumulators over the samples of a run; device memory.
#[repr(C)]
pub struct gs_time_stats {
    _private: [u8; 0],
}
/// The groups of accumulators a `gs_time_stats` keeps (a sum of these) ...
pub const GS_TSTAT_SUM: u32 = 1;
pub const GS_TSTAT_SQUARES: u32 = 2;
pub const GS_TSTAT_EXTREMES: u32 = 4;
pub const GS_TSTAT_CROSSINGS: u32 = 8;
/// ... its result planes (`which`) ...
pub const GS_TSTAT_MEAN: i32 = 0;
pub const GS_TSTAT_VARIANCE: i32 = 1;
pub const GS_TSTAT_MIN: i32 = 2;
pub const GS_TSTAT_MAX: i32 = 3;
pub const GS_TSTAT_OCCUPANCY: i32 = 4;
pub const GS_TSTAT_ARRIVAL: i32 = 5;
/// ... and its raw accumulators (`raw`): f64, f64, f32, f32, u32, u32.
pub const GS_TSTAT_RAW_SUM: i32 = 0;
pub const GS_TSTAT_RAW_SQUARES: i32 = 1;
pub const GS_TSTAT_RAW_MIN: i32 = 2;
pub const GS_TSTAT_RAW_MAX: i32 = 3;
pub const GS_TSTAT_RAW_SET_COUNT: i32 = 4;
pub const GS_TSTAT_RAW_FIRST_STAMP: i32 = 5;

/// A before-record and an after-record of a match that share `cells` grid cells (16 bytes).
#[repr(C)]
#[derive(Copy, Clone, Debug, Default, PartialEq, Eq)]
pub struct gs_component_overlap {
    pub before: u32,
    pub after: u32,
    pub cells: u64,
}

/// The noise term of a context (include/gs_hip.h: gs_ctx_set_noise): sigmas, seed, index of the next step (24 bytes).
#[repr(C)]
#[derive(Clone, Copy, Debug, PartialEq)]
pub struct gs_noise {
    pub sigma_u: f32,
    pub sigma_v: f32,
    pub seed: u64,
    pub step: u64,
}

/// A plane's summary computed on the device (32 bytes; fold order in include/gs_hip.h).
#[repr(C)]
#[derive(Copy, Clone, Debug, Default)]
pub struct gs_summary {
    pub sum: f64,
    pub sum_sq: f64,
    pub min: f32,
    pub max: f32,
    pub nonfinite: u64,
}

/// `gs_morphology` (include/gs_hip.h): the bit-quad counts of one thresholded plane or region -- Q0, Q1, Q2, Q3, Q4, QD.  48 bytes.
#[repr(C)]
#[derive(Copy, Clone, Debug, Default)]
pub struct gs_morphology {
    pub quads: [u64; 6],
}

/// `GS_REGIONS_MAX` (include/gs_hip.h): the most regions a region shape may cut a grid into.
pub const GS_REGIONS_MAX: u64 = 1 << 22;
/// `GS_REGION_HIST_MAX` (include/gs_hip.h): the most counters per field one regional histogram call returns.
pub const GS_REGION_HIST_MAX: u64 = 1 << 25;
/// `GS_REGION_SPECTRUM_MAX` (include/gs_hip.h): the most result words per field one regional spectrum call returns.
pub const GS_REGION_SPECTRUM_MAX: u64 = 1 << 25;
/// `GS_REGION_SPECTRUM_RECORDS_MAX` (include/gs_hip.h): the most segment-record words over the fields of one such call.
pub const GS_REGION_SPECTRUM_RECORDS_MAX: u64 = 1 << 27;

/// `gs_change` (include/gs_hip.h): how far one plane is from another -- sums of |d| and d * d and the largest |d| over the
/// cells finite in both (d = a - b in f64), cells whose bits differ, cells not finite in either.  40 bytes.
#[repr(C)]
#[derive(Copy, Clone, Debug, Default)]
pub struct gs_change {
    pub sum_abs: f64,
    pub sum_sq: f64,
    pub max_abs: f64,
    pub differing: u64,
    pub nonfinite: u64,
}

extern "C" {
    pub fn gs_abi_version() -> i32;
    pub fn gs_last_error() -> *const c_char;
    pub fn gs_default_options(out: *mut gs_options);
    pub fn gs_get_unique_id(out128: *mut c_void) -> i32;
    pub fn gs_ctx_create(
        out: *mut *mut gs_ctx,
        params: *const gs_params,
        opts: *const gs_options,
        device_ids: *const i32,
        n_local: i32,
        rank: i32,
        world: i32,
        unique_id: *const c_void,
    ) -> i32;
    pub fn gs_ctx_destroy(ctx: *mut gs_ctx) -> i32;
    pub fn gs_ctx_set_param_map(ctx: *mut gs_ctx, feed: *mut gs_field, kill: *mut gs_field) -> i32;
    pub fn gs_ctx_set_mask(ctx: *mut gs_ctx, mask: *mut gs_field) -> i32;
    pub fn gs_ctx_set_noise(ctx: *mut gs_ctx, n: *const gs_noise) -> i32;
    pub fn gs_ctx_get_noise(ctx: *const gs_ctx, out: *mut gs_noise, attached: *mut i32) -> i32;
    pub fn gs_field_create(ctx: *mut gs_ctx, out: *mut *mut gs_field, rows: u64, cols: u64) -> i32;
    pub fn gs_field_destroy(ctx: *mut gs_ctx, f: *mut gs_field) -> i32;
    pub fn gs_field_raw_shape(f: *const gs_field, raw_rows: *mut u64, pitch: *mut u64) -> i32;
    pub fn gs_field_fill(ctx: *mut gs_ctx, f: *mut gs_field, value: f32) -> i32;
    pub fn gs_fields_place(
        ctx: *mut gs_ctx,
        planes: *const *mut gs_field,
        candidates: i32,
        first_ms: *mut f32,
        best_ms: *mut f32,
    ) -> i32;
    pub fn gs_field_fill_slice(
        ctx: *mut gs_ctx,
        f: *mut gs_field,
        r0: u64,
        r1: u64,
        c0: u64,
        c1: u64,
        value: f32,
    ) -> i32;
    pub fn gs_field_finalize(ctx: *mut gs_ctx, f: *mut gs_field) -> i32;
    pub fn gs_field_download(ctx: *mut gs_ctx, f: *mut gs_field, host: *mut f32) -> i32;
    pub fn gs_step(
        ctx: *mut gs_ctx,
        in_u: *mut gs_field,
        in_v: *mut gs_field,
        out_u: *mut gs_field,
        out_v: *mut gs_field,
    ) -> i32;
    pub fn gs_run(
        ctx: *mut gs_ctx,
        u0: *mut gs_field,
        v0: *mut gs_field,
        u1: *mut gs_field,
        v1: *mut gs_field,
        steps: u64,
        result_slot: *mut i32,
    ) -> i32;
    pub fn gs_sync(ctx: *mut gs_ctx) -> i32;
    pub fn gs_field_download_async(ctx: *mut gs_ctx, f: *mut gs_field, host: *mut f32) -> i32;
    pub fn gs_download_wait(ctx: *mut gs_ctx) -> i32;
    pub fn gs_download_wait_but(ctx: *mut gs_ctx, in_flight: i32) -> i32;
    pub fn gs_field_colormap(
        ctx: *mut gs_ctx,
        f: *mut gs_field,
        scale: f32,
        palette_rgb: *const u8,
        n_colors: i32,
        host_rgb: *mut u8,
    ) -> i32;
    // reduced result images: the plane averaged over factor x factor blocks on the device (gs_hip.h)
    pub fn gs_field_reduced_shape(
        f: *const gs_field,
        factor: i32,
        rows: *mut u64,
        cols: *mut u64,
        local_row0: *mut u64,
        local_row1: *mut u64,
    ) -> i32;
    pub fn gs_field_download_reduced(ctx: *mut gs_ctx, f: *mut gs_field, factor: i32, host: *mut f32) -> i32;
    pub fn gs_field_download_reduced_async(ctx: *mut gs_ctx, f: *mut gs_field, factor: i32, host: *mut f32) -> i32;
    pub fn gs_field_colormap_reduced(
        ctx: *mut gs_ctx,
        f: *mut gs_field,
        factor: i32,
        scale: f32,
        palette_rgb: *const u8,
        n_colors: i32,
        host_rgb: *mut u8,
    ) -> i32;
    pub fn gs_fields_summarize(ctx: *mut gs_ctx, fields: *const *mut gs_field, n: i32, out: *mut gs_summary) -> i32;
    pub fn gs_members_summarize(
        ctx: *mut gs_ctx,
        e: *mut gs_ensemble,
        first: u64,
        count: u64,
        out: *mut gs_summary,
    ) -> i32;
    /// Power spectra (gs_hip.h): the window `h[tile]` and the `tile / 2` twiddles as (re, im) pairs; pure.
    pub fn gs_spectrum_tables(tile: i32, window: *mut f32, twiddle: *mut f32) -> i32;
    /// `power[n][tile][tile / 2 + 1]` raw f64 sums over whole tiles and `tiles[n][2]` = {used, skipped}; `window`: 0 none, 1 Hann.
    pub fn gs_fields_spectrum(
        ctx: *mut gs_ctx,
        fields: *const *mut gs_field,
        n: i32,
        tile: i32,
        window: i32,
        power: *mut f64,
        tiles: *mut u64,
    ) -> i32;
    /// The same layout with index 2 m + s for species s of member `first + m`.
    pub fn gs_members_spectrum(
        ctx: *mut gs_ctx,
        e: *mut gs_ensemble,
        first: u64,
        count: u64,
        tile: i32,
        window: i32,
        power: *mut f64,
        tiles: *mut u64,
    ) -> i32;
    /// Regional observables (gs_hip.h): `rr` x `rc` regions of `rh` x `rw` cells cut a grid of `rows` x `cols`; pure.
    pub fn gs_region_grid(rows: u64, cols: u64, rh: i32, rw: i32, rr: *mut u64, rc: *mut u64) -> i32;
    /// `out`: n x rr x rc records, region (i, j) of `fields[p]` at `p * rr * rc + i * rc + j`.
    pub fn gs_fields_region_summaries(
        ctx: *mut gs_ctx,
        fields: *const *mut gs_field,
        n: i32,
        rh: i32,
        rw: i32,
        out: *mut gs_summary,
    ) -> i32;
    /// `thresholds`: n x nt, `above`: n senses; `out`: n x rr x rc x nt records.
    pub fn gs_fields_region_morphology(
        ctx: *mut gs_ctx,
        fields: *const *mut gs_field,
        n: i32,
        rh: i32,
        rw: i32,
        thresholds: *const f32,
        above: *const i32,
        nt: i32,
        out: *mut gs_morphology,
    ) -> i32;
    /// `thresholds`: n x nt, `above`: n senses; `out`: n x rr x rc x nt x 4 x (max_lag + 1) pair counts, a region's border
    /// being a wall for pairs.
    pub fn gs_fields_region_correlation(
        ctx: *mut gs_ctx,
        fields: *const *mut gs_field,
        n: i32,
        rh: i32,
        rw: i32,
        thresholds: *const f32,
        above: *const i32,
        nt: i32,
        max_lag: i32,
        out: *mut u64,
    ) -> i32;
    /// `lo`, `hi`: n ranges; `out`: n x rr x rc x (bins + 3) counters -- counts, below, above, nan of every region,
    /// at most `GS_REGION_HIST_MAX` per field.
    pub fn gs_fields_region_histogram(
        ctx: *mut gs_ctx,
        fields: *const *mut gs_field,
        n: i32,
        rh: i32,
        rw: i32,
        lo: *const f32,
        hi: *const f32,
        bins: i32,
        out: *mut u64,
    ) -> i32;
    /// `power`: n x rr x rc x tile x (tile / 2 + 1) raw f64 sums, `tiles`: n x rr x rc x 2 counts {used, skipped} -- the
    /// spectrum of every region's cells alone, at most `GS_REGION_SPECTRUM_MAX` words per field.
    pub fn gs_fields_region_spectrum(
        ctx: *mut gs_ctx,
        fields: *const *mut gs_field,
        n: i32,
        rh: i32,
        rw: i32,
        tile: i32,
        window: i32,
        power: *mut f64,
        tiles: *mut u64,
    ) -> i32;
    /// Pair i: `a[i]` against `b[i]`, n = 1..4 pairs of one shape; `out`: n records.
    pub fn gs_fields_compare(
        ctx: *mut gs_ctx,
        a: *const *mut gs_field,
        b: *const *mut gs_field,
        n: i32,
        out: *mut gs_change,
    ) -> i32;
    /// `out`: n x RR x RC records: the change of every region of rh x rw cells of a[p] against b[p].
    pub fn gs_fields_region_compare(
        ctx: *mut gs_ctx,
        a: *const *mut gs_field,
        b: *const *mut gs_field,
        n: i32,
        rh: i32,
        rw: i32,
        out: *mut gs_change,
    ) -> i32;
    /// `out`: count x 2 records (U, V) of members first + i of `e` against the same members of `reference`.
    pub fn gs_members_compare(
        ctx: *mut gs_ctx,
        e: *mut gs_ensemble,
        reference: *mut gs_ensemble,
        first: u64,
        count: u64,
        out: *mut gs_change,
    ) -> i32;
    /// Device copies: `dst[i]` receives the cells of `src[i]` (snapshots and restores); blocking.
    pub fn gs_fields_copy(ctx: *mut gs_ctx, dst: *const *mut gs_field, src: *const *mut gs_field, n: i32) -> i32;
    pub fn gs_members_copy(ctx: *mut gs_ctx, dst: *mut gs_ensemble, src: *mut gs_ensemble, first: u64, count: u64) -> i32;
    /// `out`: n x (bins + 3) counters -- counts[bins], below, above, nan -- by the rule of include/gs_hip.h.
    pub fn gs_fields_histogram(
        ctx: *mut gs_ctx,
        fields: *const *mut gs_field,
        n: i32,
        lo: *const f32,
        hi: *const f32,
        bins: i32,
        out: *mut u64,
    ) -> i32;
    /// `lo`, `hi`: two values each (U, V); `out`: count x 2 x (bins + 3) counters.
    pub fn gs_members_histogram(
        ctx: *mut gs_ctx,
        e: *mut gs_ensemble,
        first: u64,
        count: u64,
        lo: *const f32,
        hi: *const f32,
        bins: i32,
        out: *mut u64,
    ) -> i32;
    /// What became of the components of `before` in `after` (two planes of one shape, one rule): `out` receives a match.
    pub fn gs_fields_match(
        ctx: *mut gs_ctx,
        before: *mut gs_field,
        after: *mut gs_field,
        threshold: f32,
        above: i32,
        connectivity: i32,
        min_size: u64,
        out: *mut *mut gs_component_match,
    ) -> i32;
    /// Member first + i of `after` against member first + i of `before`; the match has `count` planes.
    pub fn gs_members_match(
        ctx: *mut gs_ctx,
        before: *mut gs_ensemble,
        after: *mut gs_ensemble,
        first: u64,
        count: u64,
        species: i32,
        threshold: f32,
        above: i32,
        connectivity: i32,
        min_size: u64,
        out: *mut *mut gs_component_match,
    ) -> i32;
    /// The two lists (owned by the match), the planes, `planes + 1` offsets and the overlaps; valid until the match is destroyed.
    pub fn gs_component_match_view(
        m: *const gs_component_match,
        before: *mut *const gs_component_list,
        after: *mut *const gs_component_list,
        planes: *mut u64,
        offsets: *mut *const u64,
        overlaps: *mut *const gs_component_overlap,
    ) -> i32;
    /// Null: `GS_OK`.
    pub fn gs_component_match_destroy(m: *mut gs_component_match) -> i32;
    /// Accumulators for `n` (1..4) planes of `rows` x `cols` cells; `thresholds[n]` / `above[n]` with `GS_TSTAT_CROSSINGS`.
    pub fn gs_time_stats_create(
        ctx: *mut gs_ctx,
        out: *mut *mut gs_time_stats,
        rows: u64,
        cols: u64,
        n: i32,
        groups: u32,
        thresholds: *const f32,
        above: *const i32,
    ) -> i32;
    /// Null: `GS_OK`.
    pub fn gs_time_stats_destroy(ctx: *mut gs_ctx, ts: *mut gs_time_stats) -> i32;
    pub fn gs_time_stats_reset(ctx: *mut gs_ctx, ts: *mut gs_time_stats) -> i32;
    /// One sample of `fields[0 .. n)`, stamped `stamp` (any u32 but 0xffffffff): enqueued, not waited for.
    pub fn gs_time_stats_accumulate(ctx: *mut gs_ctx, ts: *mut gs_time_stats, fields: *const *mut gs_field, n: i32, stamp: u32) -> i32;
    pub fn gs_time_stats_samples(ts: *const gs_time_stats, n: *mut u64) -> i32;
    /// Result plane `which` of plane `plane` into `out`, a field of the same shape.
    pub fn gs_time_stats_result(ctx: *mut gs_ctx, ts: *mut gs_time_stats, plane: i32, which: i32, out: *mut gs_field) -> i32;
    /// Raw accumulator `raw` of plane `plane`: dense rows of this process, of the accumulator's own type.
    pub fn gs_time_stats_download(ctx: *mut gs_ctx, ts: *mut gs_time_stats, plane: i32, raw: i32, host: *mut c_void) -> i32;
    /// Planes 0 / 1 = U / V of members `[first, first + count)` of an ensemble shaped like `like`.
    pub fn gs_members_time_stats_create(
        ctx: *mut gs_ctx,
        out: *mut *mut gs_time_stats,
        like: *mut gs_ensemble,
        first: u64,
        count: u64,
        groups: u32,
        thresholds: *const f32,
        above: *const i32,
    ) -> i32;
    pub fn gs_members_time_stats_accumulate(ctx: *mut gs_ctx, ts: *mut gs_time_stats, e: *mut gs_ensemble, stamp: u32) -> i32;
    /// `host[count, rows, cols]`: result plane `which` of species `species` of every member.
    pub fn gs_members_time_stats_result(ctx: *mut gs_ctx, ts: *mut gs_time_stats, species: i32, which: i32, host: *mut f32) -> i32;
    /// Per-cell statistics across members: every run of `span` members of `[first, first + count)` is a bundle, and result
    /// `which[i]` (`GS_TSTAT_MEAN` .. `GS_TSTAT_OCCUPANCY`) of bundle `b` is written into member `out_first + b` of `out[i]`.
    /// `thresholds[2]` / `above[2]` (U's, V's) are needed with the occupancy and may be null without it.
    pub fn gs_members_bundle_stats(
        ctx: *mut gs_ctx,
        e: *mut gs_ensemble,
        first: u64,
        count: u64,
        span: u64,
        which: *const i32,
        n: i32,
        thresholds: *const f32,
        above: *const i32,
        out: *const *mut gs_ensemble,
        out_first: u64,
    ) -> i32;
}
