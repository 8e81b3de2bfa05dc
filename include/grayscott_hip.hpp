// grayscott_hip.hpp -- header-only C++17 mirror of the reference's backend interface over the
// C ABI (gs_hip.h).  Same names, argument meaning and error behaviour as the Rust items:
//
//   gs::Parameters        data/src/parameters.rs:13-33, Default :72-83
//   gs::HipConcentration  Concentration trait, data/src/concentration/mod.rs:198-296
//   gs::Evolving/Species  data/src/concentration/mod.rs:17-187 (Species::new :36-59)
//   gs::Simulation        SimulateBase/SimulateCreate/Simulate, compute/shared/src/lib.rs:19-58
//
// Errors: a non-zero gs_status becomes gs::HipError (the Rust shim's HipError); programming
// errors that panic in the reference (shape mismatch in write_scalar_view,
// concentration/mod.rs:291-295) throw std::logic_error.
#pragma once
#include "gs_hip.h"

#include <array>
#include <cmath>
#include <cstddef>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

namespace gs {

using Precision = float; // data/src/lib.rs:11

struct HipError : std::runtime_error {
    int32_t code;
    HipError(int32_t c, const std::string &m)
        : std::runtime_error("gs_hip error " + std::to_string(c) + ": " + m), code(c) {}
};

inline void check(int32_t status)
{
    if (status != GS_OK) throw HipError(status, gs_last_error());
}

// What became of the components of one thresholded plane between two states (gs_fields_match): the two states' component
// lists and, in ascending (before, after) order, every pair of records that shares a cell with the number of shared cells.
struct ComponentMatch {
    std::vector<gs_component_record> before, after;
    std::vector<gs_component_overlap> overlaps;
};

namespace detail {
// The planes of a gs_component_match copied out, one ComponentMatch per plane; the match is destroyed at once, its lists with it.
inline std::vector<ComponentMatch> take_component_matches(gs_component_match *match)
{
    const gs_component_list *lists[2] = {nullptr, nullptr};
    uint64_t planes = 0, list_planes = 0;
    const uint64_t *offsets = nullptr, *list_offsets = nullptr;
    const gs_component_overlap *overlaps = nullptr;
    const gs_component_record *records = nullptr;
    int32_t status = gs_component_match_view(match, &lists[0], &lists[1], &planes, &offsets, &overlaps);
    std::vector<ComponentMatch> out((std::size_t)(status == GS_OK ? planes : 0));
    for (uint64_t i = 0; status == GS_OK && i < planes; ++i) out[i].overlaps.assign(overlaps + offsets[i], overlaps + offsets[i + 1]);
    for (int k = 0; status == GS_OK && k < 2; ++k) {
        status = gs_component_list_view(lists[k], &list_planes, &list_offsets, &records);
        for (uint64_t i = 0; status == GS_OK && i < planes; ++i)
            (k ? out[i].after : out[i].before).assign(records + list_offsets[i], records + list_offsets[i + 1]);
    }
    gs_component_match_destroy(match);
    check(status);
    return out;
}
// The planes of a gs_component_list copied out, one vector of records per plane; the list is destroyed at once.
inline std::vector<std::vector<gs_component_record>> take_component_lists(gs_component_list *list)
{
    uint64_t planes = 0;
    const uint64_t *offsets = nullptr;
    const gs_component_record *records = nullptr;
    const int32_t status = gs_component_list_view(list, &planes, &offsets, &records);
    std::vector<std::vector<gs_component_record>> out;
    if (status == GS_OK)
        for (uint64_t i = 0; i < planes; ++i) out.emplace_back(records + offsets[i], records + offsets[i + 1]);
    gs_component_list_destroy(list);
    check(status);
    return out;
}
// U's thresholds, then V's -- the C ABI's order for (U, V) -- or the refusal when their numbers differ.
inline std::vector<float> uv_thresholds(const std::vector<float> &u_thresholds, const std::vector<float> &v_thresholds)
{
    if (u_thresholds.size() != v_thresholds.size())
        throw HipError(GS_ERR_INVALID, "the same number of thresholds for U and V");
    std::vector<float> t(u_thresholds);
    t.insert(t.end(), v_thresholds.begin(), v_thresholds.end());
    return t;
}
// The cells of region (i, j) of a grid of rows x cols cells cut into regions of rh x rw: fewer in a ragged last row or column.
inline uint64_t region_cells(uint64_t rows, uint64_t cols, int32_t rh, int32_t rw, uint64_t i, uint64_t j)
{
    const uint64_t h = rows - i * (uint64_t)rh, w = cols - j * (uint64_t)rw;
    return (h < (uint64_t)rh ? h : (uint64_t)rh) * (w < (uint64_t)rw ? w : (uint64_t)rw);
}
} // namespace detail

// A plane's summary computed on the device (gs_summary): sum, sum of squares, min and max of its finite cells (fold order
// of gs_hip.h: bit-reproducible), the count of its non-finite cells, and `size`, its number of cells.
struct Summary {
    double sum = 0.0, sum_sq = 0.0;
    float min = 0.0f, max = 0.0f;
    uint64_t nonfinite = 0, size = 0;
    static Summary from_c(const gs_summary &s, uint64_t size)
    {
        return Summary{s.sum, s.sum_sq, s.min, s.max, s.nonfinite, size};
    }
    uint64_t cells() const { return size - nonfinite; } // the finite ones
    double mean() const { return cells() ? sum / (double)cells() : std::nan(""); }
    double std() const
    {
        if (!cells()) return std::nan("");
        const double m = mean(), var = sum_sq / (double)cells() - m * m;
        return var > 0.0 ? std::sqrt(var) : 0.0;
    }
};

// How far one plane is from another of the same shape, computed on the device (gs_change, gs_hip.h): with d = a - b formed
// in f64 per cell, the sums of |d| and d * d (the summaries' fold order: bit-reproducible) and the largest |d| over the
// comparable cells -- those finite in both planes --, the cells whose 32 bits differ (all cells), the cells not finite in
// either plane, and `cells`, the planes' number of cells.
struct Change {
    double sum_abs = 0.0, sum_sq = 0.0, max_abs = 0.0;
    uint64_t differing = 0, nonfinite = 0, cells = 0;
    static Change from_c(const gs_change &c, uint64_t cells)
    {
        return Change{c.sum_abs, c.sum_sq, c.max_abs, c.differing, c.nonfinite, cells};
    }
    uint64_t comparable() const { return cells - nonfinite; }
    bool equal() const { return differing == 0; } // the same bits in every cell
    double mean_abs() const { return comparable() ? sum_abs / (double)comparable() : std::nan(""); }
    double rms() const { return comparable() ? std::sqrt(sum_sq / (double)comparable()) : std::nan(""); }
};

// A plane's histogram computed on the device (gs_fields_histogram; the binning rule is gs_hip.h's): `counts[i]` cells in
// bin i of `counts.size()` equal bins of [lo, hi] (the last one closed), `below` / `above` the range, `nan`; `size` = the
// plane's number of cells = the sum of all of them.
struct Histogram {
    std::vector<uint64_t> counts;
    uint64_t below = 0, above = 0, nan = 0;
    float lo = 0.0f, hi = 0.0f;
    uint64_t size = 0;
    // from bins + 3 counters as the C ABI writes them
    static Histogram from_c(const uint64_t *c, int32_t bins, float lo, float hi, uint64_t size)
    {
        Histogram h;
        h.counts.assign(c, c + bins);
        h.below = c[bins];
        h.above = c[bins + 1];
        h.nan = c[bins + 2];
        h.lo = lo;
        h.hi = hi;
        h.size = size;
        return h;
    }
    uint64_t in_range() const
    {
        uint64_t n = 0;
        for (uint64_t c : counts) n += c;
        return n;
    }
};

// The bit-quad counts of one thresholded plane, counted on the device (gs_fields_morphology; the rule is gs_hip.h's): a cell
// is set when it is above `threshold` (`above`) or below it, the image is padded with one ring of unset cells, and `quads`
// counts its (rows + 1)(cols + 1) 2 x 2 blocks by class: Q0, Q1, Q2, Q3, Q4, QD.  What follows is exact.
struct Morphology {
    std::array<uint64_t, 6> quads{};
    float threshold = 0.0f;
    bool above = true;
    uint64_t cells = 0;
    static Morphology from_c(const gs_morphology &m, float threshold, bool above, uint64_t cells)
    {
        Morphology o;
        for (std::size_t i = 0; i < 6; ++i) o.quads[i] = m.quads[i];
        o.threshold = threshold;
        o.above = above;
        o.cells = cells;
        return o;
    }
    // set cells
    uint64_t area() const { return (quads[1] + 2 * quads[2] + 2 * quads[5] + 3 * quads[3] + 4 * quads[4]) / 4; }
    double area_fraction() const { return cells ? (double)area() / (double)cells : std::nan(""); }
    // cell sides between a set and an unset cell (4-connected boundary length), the padding ring included
    uint64_t perimeter() const { return quads[1] + quads[2] + 2 * quads[5] + quads[3]; }
    // components minus holes under 4- and 8-connectivity
    int64_t euler4() const { return ((int64_t)quads[1] - (int64_t)quads[3] + 2 * (int64_t)quads[5]) / 4; }
    int64_t euler8() const { return ((int64_t)quads[1] - (int64_t)quads[3] - 2 * (int64_t)quads[5]) / 4; }
};

// The results of every region of one plane (gs_fields_region_summaries, gs_fields_region_morphology; the rules are gs_hip.h's):
// a region shape (rh, rw) cuts the plane into rr x rc regions, ragged ones at the lower and right edge kept, and `at(i, j)` is
// bit for bit the whole-grid result of a plane that holds region (i, j)'s cells alone.
template <typename T> struct Regions {
    uint64_t rr = 0, rc = 0;
    int32_t rh = 0, rw = 0;
    std::vector<T> results; // rr * rc, region (i, j) at i * rc + j
    const T &at(uint64_t i, uint64_t j) const { return results.at((std::size_t)(i * rc + j)); }
};
using RegionSummaries = Regions<Summary>;
using RegionMorphology = Regions<Morphology>; // of one threshold

// The connected components of one thresholded plane, labelled on the device (gs_fields_components; the rule is gs_hip.h's): a
// cell is set by Morphology's rule, set cells are neighbours across a side or, under connectivity 8, also across a corner;
// components never wrap.  by_size[b] counts the components of 2^b <= size < 2^(b+1) cells (the last bin takes every larger
// one).  All exact integers.
struct Components {
    uint64_t count = 0, set_cells = 0, largest = 0;
    std::array<uint64_t, 32> by_size{};
    float threshold = 0.0f;
    bool above = true;
    int32_t connectivity = 8;
    static Components from_c(const gs_components &c, float threshold, bool above, int32_t connectivity)
    {
        Components o;
        o.count = c.components;
        o.set_cells = c.set_cells;
        o.largest = c.largest;
        for (std::size_t b = 0; b < 32; ++b) o.by_size[b] = c.by_size[b];
        o.threshold = threshold;
        o.above = above;
        o.connectivity = connectivity;
        return o;
    }
    double mean_size() const { return count ? (double)set_cells / (double)count : std::nan(""); }
    double largest_fraction() const { return set_cells ? (double)largest / (double)set_cells : std::nan(""); }
    // holes of the pattern: components minus the Euler number of the same connectivity, from a Morphology of the same plane,
    // threshold and sense (another threshold or sense is refused)
    int64_t holes(const Morphology &m) const
    {
        if (m.threshold != threshold || m.above != above)
            throw HipError(GS_ERR_INVALID, "a Morphology of another threshold or sense");
        return (int64_t)count - (connectivity == 8 ? m.euler8() : m.euler4());
    }
};
// (gs_fields_region_components): `at(i, j)` is the Components of region (i, j)'s cells alone -- a region's border is a wall
using RegionComponents = Regions<Components>; // of one threshold
// (gs_fields_region_compare): `at(i, j)` is the Change of two planes that hold region (i, j)'s cells alone, `cells` the region's
struct RegionChange : Regions<Change> {
    // per region: no comparable cell moved by more than tol, and every cell is comparable
    std::vector<bool> steady(double tol) const
    {
        std::vector<bool> out;
        for (const Change &c : results) out.push_back(c.max_abs <= tol && c.nonfinite == 0);
        return out;
    }
};

// The two-point pair counts of one thresholded plane, counted on the device (gs_fields_correlation; the rule is gs_hip.h's):
// pairs[k][d] is the number of cell pairs {p, p + d e_k}, d = 0 .. max_lag, inside the grid with both cells set, for the unit
// steps e_0 = (0, 1), e_1 = (1, 0), e_2 = (1, 1), e_3 = (1, -1).  Pairs never wrap.  What follows is computed from the integers.
struct Correlation {
    std::array<std::vector<uint64_t>, 4> pairs;
    float threshold = 0.0f;
    bool above = true;
    uint64_t rows = 0, cols = 0;
    // `c`: [4][max_lag + 1], the layout of gs_fields_correlation for one plane and threshold
    static Correlation from_c(const uint64_t *c, int32_t max_lag, float threshold, bool above, uint64_t rows, uint64_t cols)
    {
        Correlation o;
        for (std::size_t k = 0; k < 4; ++k) o.pairs[k].assign(c + k * (std::size_t)(max_lag + 1), c + (k + 1) * (std::size_t)(max_lag + 1));
        o.threshold = threshold;
        o.above = above;
        o.rows = rows;
        o.cols = cols;
        return o;
    }
    int32_t max_lag() const { return (int32_t)pairs[0].size() - 1; }
    uint64_t pairs_set(std::size_t k, std::size_t d) const { return pairs[k][d]; }
    // the pairs {p, p + d e_k} that exist inside the grid: geometry
    uint64_t pairs_total(std::size_t k, std::size_t d) const
    {
        const uint64_t dr = k == 0 ? 0 : d, dc = k == 1 ? 0 : d;
        return (rows > dr ? rows - dr : 0) * (cols > dc ? cols - dc : 0);
    }
    // set cells over cells
    double fraction() const { return rows * cols != 0 ? (double)pairs[0][0] / (double)(rows * cols) : std::nan(""); }
    // the two-point probability: set pairs over pairs; NaN where no pair exists
    double s2(std::size_t k, std::size_t d) const
    {
        const uint64_t total = pairs_total(k, d);
        return total ? (double)pairs[k][d] / (double)total : std::nan("");
    }
    double autocovariance(std::size_t k, std::size_t d) const { return s2(k, d) - fraction() * fraction(); }
    // the length of d e_k in cells
    double distance(std::size_t k, std::size_t d) const { return (double)d * (k < 2 ? 1.0 : std::sqrt(2.0)); }
};

// The tile-averaged power spectrum of one plane, summed on the device (gs_fields_spectrum; the rule is gs_hip.h's):
// raw[kr * (tile / 2 + 1) + kc] is the sum over the whole tile x tile tiles that hold only finite cells of
// |FFT2(window (tile - its mean))|^2, kr < tile, kc <= tile / 2; tiles_used and tiles_skipped count those tiles and the ones
// left out.  What follows is computed from these sums; frequencies are in cycles per cell.
struct Spectrum {
    std::vector<double> raw;
    int32_t tile = 0, window = 0; // window: 0 none, 1 periodic Hann
    uint64_t tiles_used = 0, tiles_skipped = 0;
    // `p`: [tile][tile / 2 + 1], `t`: {used, skipped} -- the layout of gs_fields_spectrum for one plane
    static Spectrum from_c(const double *p, const uint64_t *t, int32_t tile, int32_t window)
    {
        Spectrum o;
        o.raw.assign(p, p + (std::size_t)tile * (std::size_t)(tile / 2 + 1));
        o.tile = tile;
        o.window = window;
        o.tiles_used = t[0];
        o.tiles_skipped = t[1];
        return o;
    }
    std::size_t bins() const { return (std::size_t)tile * (std::size_t)(tile / 2 + 1); }
    // the sum of (h_r h_c)^2 over a tile: tile^2 without a window
    double window_energy() const
    {
        if (!window) return (double)tile * (double)tile;
        double e = 0.0;
        for (int32_t j = 0; j < tile; ++j) {
            const double h = 0.5 - 0.5 * std::cos(2.0 * 3.14159265358979323846 * (double)j / (double)tile);
            e += h * h;
        }
        return e * e;
    }
    // the mean over the tiles used, divided by the window's energy; NaN without a tile
    double power(std::size_t kr, std::size_t kc) const
    {
        return tiles_used ? raw[kr * (std::size_t)(tile / 2 + 1) + kc] / ((double)tiles_used * window_energy()) : std::nan("");
    }
    // S(|k|) on rings 0 .. tile / 2: ring round(tile sqrt(f_r^2 + f_c^2)), a bin weighing 2 for 0 < kc < tile / 2, else 1; bins
    // beyond the last ring are dropped
    std::vector<double> radial() const
    {
        const std::size_t half = (std::size_t)tile / 2;
        std::vector<double> sum(half + 1, 0.0), weight(half + 1, 0.0);
        for (std::size_t kr = 0; kr < (std::size_t)tile; ++kr)
            for (std::size_t kc = 0; kc <= half; ++kc) {
                const double fr = (kr < half ? (double)kr : (double)kr - (double)tile), fc = (double)kc;
                const std::size_t ring = (std::size_t)std::nearbyint(std::sqrt(fr * fr + fc * fc));
                if (ring > half) continue;
                const double w = kc > 0 && kc < half ? 2.0 : 1.0;
                sum[ring] += w * power(kr, kc);
                weight[ring] += w;
            }
        for (std::size_t k = 0; k <= half; ++k) sum[k] /= weight[k];
        return sum;
    }
    // the pattern's wavenumber in cycles per cell: the largest ring among 1 .. tile / 2 - 1, refined by a parabola through its
    // neighbours; NaN for a flat spectrum (or none at all)
    double peak_wavenumber() const
    {
        const std::vector<double> s = radial();
        const std::size_t half = (std::size_t)tile / 2;
        std::size_t k = 1;
        double lo = s[1], hi = s[1];
        for (std::size_t i = 0; i <= half; ++i)
            if (!std::isfinite(s[i])) return std::nan("");
        for (std::size_t i = 1; i < half; ++i) {
            if (s[i] > hi) {
                hi = s[i];
                k = i;
            }
            if (s[i] < lo) lo = s[i];
        }
        if (!(hi > lo)) return std::nan("");
        const double bend = s[k - 1] - 2.0 * s[k] + s[k + 1];
        double shift = bend < 0.0 ? 0.5 * (s[k - 1] - s[k + 1]) / bend : 0.0;
        shift = shift < -0.5 ? -0.5 : (shift > 0.5 ? 0.5 : shift);
        return ((double)k + shift) / (double)tile;
    }
    // cells per period
    double wavelength() const { return 1.0 / peak_wavenumber(); }
};

// of one threshold (gs_fields_region_correlation): `at(i, j)` has region (i, j)'s own rows and cols, a pair across a region
// border is never formed
using RegionCorrelation = Regions<Correlation>;
// (gs_fields_region_histogram): `at(i, j)` is the Histogram of region (i, j)'s cells alone, its `size` the region's own cells
using RegionHistogram = Regions<Histogram>;
// (gs_fields_region_spectrum): `at(i, j)` is the Spectrum of region (i, j)'s cells alone, tiles anchored at the region's first
// row and column; a region in which no tile fits has zeros and no tiles
using RegionSpectrum = Regions<Spectrum>;

struct Parameters {
    std::array<std::array<Precision, 3>, 3> weights{{{0.25f, 0.5f, 0.25f}, {0.5f, 0.0f, 0.5f}, {0.25f, 0.5f, 0.25f}}};
    Precision diffusion_rate_u = 0.1f, diffusion_rate_v = 0.05f;
    Precision feed_rate = 0.014f, kill_rate = 0.054f, time_step = 1.0f;

    // the reference's compile-time stencil choices (data/Cargo.toml:28-58, parameters.rs:91-122) as
    // run-time values: "oono-puri" (default), "5points", "patrakarttunen", "pretty"
    static Parameters with_stencil(const std::string &name)
    {
        Parameters p;
        if (name == "5points") p.weights = {{{0.f, 1.f, 0.f}, {1.f, 0.f, 1.f}, {0.f, 1.f, 0.f}}};
        else if (name == "patrakarttunen") {
            const Precision a = 1.0f / 6.0f, b = 4.0f / 6.0f;
            p.weights = {{{a, b, a}, {b, 0.f, b}, {a, b, a}}};
        } else if (name == "pretty") p.weights = {{{1.f, 1.f, 1.f}, {1.f, 1.f, 1.f}, {1.f, 1.f, 1.f}}};
        else if (name != "oono-puri") throw std::invalid_argument("unknown stencil " + name);
        return p;
    }

    gs_params to_c() const
    {
        gs_params p;
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) p.w[i][j] = weights[i][j];
        p.du = diffusion_rate_u;
        p.dv = diffusion_rate_v;
        p.feed = feed_rate;
        p.kill = kill_rate;
        p.dt = time_step;
        return p;
    }
};

// Backend CLI arguments (every field defaulted, compute/shared/src/lib.rs:20-25).
struct HipArgs {
    std::vector<int32_t> devices{0};
    int32_t math = GS_MATH_STRICT, kernel = GS_KERNEL_AUTO, rows_per_block = 0, fuse_steps = 0, cols_per_lane = 0;
    // boundary: any gs_boundary of gs_hip.h, GS_BOUNDARY_PERIODIC (one device, one process) and GS_BOUNDARY_NEUMANN included
    int32_t boundary = GS_BOUNDARY_CLIPPED, no_tune = 0, share_taps = 0, general_kernels = 0;
    // not a gs_options field: the most extra blocks gs_fields_place may draw when make_species places a Species by
    // measurement -- every Species of >= 2^26 cells on a context with one slab (0 = planes as hipMalloc hands them out)
    int32_t place_candidates = 12;
};

// Concentration::Context: owner of the gs_ctx.
class HipContext {
  public:
    HipContext(const Parameters &params, const HipArgs &args)
    {
        gs_params p = params.to_c();
        gs_options o;
        gs_default_options(&o);
        o.math = args.math;
        o.kernel = args.kernel;
        o.rows_per_block = args.rows_per_block;
        o.fuse_steps = args.fuse_steps;
        o.cols_per_lane = args.cols_per_lane;
        o.boundary = args.boundary;
        o.no_tune = args.no_tune;
        o.share_taps = args.share_taps;
        o.general_kernels = args.general_kernels;
        check(gs_ctx_create(&ctx_, &p, &o, args.devices.data(), (int32_t)args.devices.size(), 0, 1, nullptr));
        place_candidates_ = args.devices.size() == 1 ? args.place_candidates : 0;
    }
    ~HipContext() { gs_ctx_destroy(ctx_); }
    int32_t place_candidates() const { return place_candidates_; }
    HipContext(const HipContext &) = delete;
    HipContext &operator=(const HipContext &) = delete;
    gs_ctx *get() const { return ctx_; }
    void sync() const { check(gs_sync(ctx_)); }
    // waits for the asynchronous downloads enqueued so far (not for later steps)
    void download_wait() const { check(gs_download_wait(ctx_)); }
    // ... for all but the newest `in_flight` (0 or 1): two images on their way, the PCIe link never idles between them
    void download_wait_but(int32_t in_flight) const { check(gs_download_wait_but(ctx_, in_flight)); }
    // counters of the context (passes, steps, launches, blocking ghost refreshes) and, on slab chains, the
    // halo-stream / interior times of the passes timed with set_pass_timing (gs_ctx_stats)
    gs_stats stats() const
    {
        gs_stats st;
        check(gs_ctx_stats(ctx_, &st));
        return st;
    }
    void set_pass_timing(int32_t passes) const { check(gs_ctx_set_pass_timing(ctx_, passes)); }


  private:
    gs_ctx *ctx_ = nullptr;
    int32_t place_candidates_ = 0;
};
using Context = std::shared_ptr<HipContext>;

using Shape = std::array<std::size_t, 2>;
using Range = std::pair<std::size_t, std::size_t>; // half-open, like Rust's Range<usize>

class HipConcentration {
  public:
    static HipConcentration default_(Context &c, Shape s) { return HipConcentration(c, s); }
    static HipConcentration zeros(Context &c, Shape s) { return HipConcentration(c, s); }
    static HipConcentration ones(Context &c, Shape s)
    {
        HipConcentration x(c, s);
        check(gs_field_fill(c->get(), x.f_, 1.0f));
        return x;
    }
    HipConcentration(HipConcentration &&o) noexcept : ctx_(std::move(o.ctx_)), f_(o.f_), shape_(o.shape_) { o.f_ = nullptr; }
    HipConcentration &operator=(HipConcentration &&o) noexcept
    {
        std::swap(ctx_, o.ctx_);
        std::swap(f_, o.f_);
        std::swap(shape_, o.shape_);
        return *this;
    }
    ~HipConcentration()
    {
        if (f_) gs_field_destroy(ctx_->get(), f_);
    }
    Shape shape() const { return shape_; }
    Shape raw_shape() const
    {
        uint64_t r = 0, p = 0;
        check(gs_field_raw_shape(f_, &r, &p));
        return {(std::size_t)r, (std::size_t)p};
    }
    void fill_slice(Context &c, std::array<Range, 2> slice, Precision value)
    {
        check(gs_field_fill_slice(c->get(), f_, slice[0].first, slice[0].second, slice[1].first,
                                  slice[1].second, value));
    }
    void finalize(Context &c) { check(gs_field_finalize(c->get(), f_)); }
    // make_scalar_view: owned dense copy [rows * cols]
    std::vector<Precision> make_scalar_view(Context &c)
    {
        std::vector<Precision> out(shape_[0] * shape_[1]);
        check(gs_field_download(c->get(), f_, out.data()));
        return out;
    }
    // write_scalar_view: the target must have exactly this table's shape (validate_write)
    void write_scalar_view(Context &c, Precision *target, Shape target_shape)
    {
        if (target_shape != shape_) throw std::logic_error("write_scalar_view: target shape mismatch");
        check(gs_field_download(c->get(), f_, target));
    }
    // write_scalar_view_after (data/src/concentration/gpu/image/mod.rs:196-206): enqueue the
    // download behind the steps already enqueued; `target` (ideally from PinnedImage) is valid
    // after HipContext::download_wait()
    void write_scalar_view_after(Context &c, Precision *target, Shape target_shape)
    {
        if (target_shape != shape_) throw std::logic_error("write_scalar_view_after: target shape mismatch");
        check(gs_field_download_async(c->get(), f_, target));
    }
    // Reduced result images (gs_hip.h: gs_field_download_reduced): the plane averaged over reduce x reduce blocks on the
    // device.  reduced_shape: this process's rows of the image x its columns (throws HipError for a factor outside 1..64
    // and for a slab chain whose slabs do not begin at multiples of the factor).
    Shape reduced_shape(int32_t reduce) const
    {
        uint64_t cols = 0, r0 = 0, r1 = 0;
        check(gs_field_reduced_shape(f_, reduce, nullptr, &cols, &r0, &r1));
        return Shape{(std::size_t)(r1 - r0), (std::size_t)cols};
    }
    std::vector<Precision> make_scalar_view(Context &c, int32_t reduce)
    {
        const Shape s = reduced_shape(reduce);
        std::vector<Precision> out(s[0] * s[1]);
        check(gs_field_download_reduced(c->get(), f_, reduce, out.data()));
        return out;
    }
    void write_scalar_view(Context &c, Precision *target, Shape target_shape, int32_t reduce)
    {
        if (target_shape != reduced_shape(reduce)) throw std::logic_error("write_scalar_view: target shape mismatch");
        check(gs_field_download_reduced(c->get(), f_, reduce, target));
    }
    void write_scalar_view_after(Context &c, Precision *target, Shape target_shape, int32_t reduce)
    {
        if (target_shape != reduced_shape(reduce)) throw std::logic_error("write_scalar_view_after: target shape mismatch");
        check(gs_field_download_reduced_async(c->get(), f_, reduce, target));
    }
    // gs_field_colormap_reduced: RGB8 [reduced rows, reduced cols, 3] through a palette of n_colors RGB triples
    std::vector<uint8_t> colormap(Context &c, const uint8_t *palette_rgb, int32_t n_colors, float scale, int32_t reduce)
    {
        const Shape s = reduced_shape(reduce);
        std::vector<uint8_t> out(s[0] * s[1] * 3);
        check(gs_field_colormap_reduced(c->get(), f_, reduce, scale, palette_rgb, n_colors, out.data()));
        return out;
    }
    gs_field *raw() const { return f_; }
    // a zero-copy producer wrote cells through gs_field_device_ptr: ghost rows of neighbouring slabs are stale
    void mark_written(Context &c) { check(gs_field_mark_written(c->get(), f_)); }

  private:
    HipConcentration(Context &c, Shape s) : ctx_(c), shape_(s)
    {
        check(gs_field_create(c->get(), &f_, s[0], s[1]));
    }
    Context ctx_;
    gs_field *f_ = nullptr;
    Shape shape_{};
};

// Page-locked host image for overlapped downloads (gs_host_alloc / gs_host_free).
class PinnedImage {
  public:
    explicit PinnedImage(Shape s) : shape_(s)
    {
        void *p = nullptr;
        check(gs_host_alloc(&p, (uint64_t)s[0] * s[1] * sizeof(Precision)));
        data_ = static_cast<Precision *>(p);
    }
    ~PinnedImage() { gs_host_free(data_); }
    PinnedImage(const PinnedImage &) = delete;
    PinnedImage &operator=(const PinnedImage &) = delete;
    Precision *data() { return data_; }
    const Precision *data() const { return data_; }
    Shape shape() const { return shape_; }

  private:
    Precision *data_ = nullptr;
    Shape shape_;
};

// Pair of concentrations, slot 0 = input, slot 1 = output (concentration/mod.rs:140-187).
class Evolving {
  public:
    static Evolving zeros_out(Context &c, Shape s)
    {
        return Evolving(HipConcentration::default_(c, s), HipConcentration::zeros(c, s));
    }
    static Evolving ones_out(Context &c, Shape s)
    {
        return Evolving(HipConcentration::default_(c, s), HipConcentration::ones(c, s));
    }
    HipConcentration &in() { return pair_[0]; }
    HipConcentration &out() { return pair_[1]; }
    Shape shape() const { return pair_[0].shape(); }
    void flip(Context &c)
    {
        pair_[1].finalize(c);
        std::swap(pair_[0], pair_[1]);
    }
    void swap_slots() { std::swap(pair_[0], pair_[1]); }

  private:
    Evolving(HipConcentration a, HipConcentration b) : pair_{std::move(a), std::move(b)} {}
    std::array<HipConcentration, 2> pair_;
};

class Species;

// A state of a Species kept on the device: one U and one V plane of its own, filled by a device copy (gs_fields_copy) of the
// species' current in-planes.  Made by Species::snapshot; Species::change_since compares with it, Species::restore goes
// back to it.
class Snapshot {
  public:
    inline void update(Species &species); // take the species' current state (blocking)
    HipConcentration &u() { return u_; }
    HipConcentration &v() { return v_; }

  private:
    friend class Species;
    Snapshot(Context &c, Shape s) : context_(c), u_(HipConcentration::default_(c, s)), v_(HipConcentration::default_(c, s)) {}
    Context context_;
    HipConcentration u_, v_;
};

class Species {
  public:
    // Species::new (concentration/mod.rs:36-59)
    static Species new_(Context context, Shape shape)
    {
        Evolving u = Evolving::ones_out(context, shape);
        Evolving v = Evolving::zeros_out(context, shape);
        const std::size_t num_range[2] = {7, 8}, frac = 16, row_shift = 4;
        std::array<Range, 2> center;
        for (int i = 0; i < 2; ++i) {
            const std::size_t shift = (i == 0) ? row_shift : 0;
            auto edge = [&](int j) {
                const std::size_t x = shape[i] * num_range[j] / frac;
                return x > shift ? x - shift : 0; // saturating_sub
            };
            center[i] = {edge(0), edge(1)};
        }
        u.out().fill_slice(context, center, 0.0f);
        v.out().fill_slice(context, center, 1.0f);
        Species s(std::move(context), std::move(u), std::move(v));
        s.flip();
        return s;
    }
    Context &context() { return context_; }
    Shape shape() const { return u_.shape(); }
    // placement by measurement (gs_fields_place; not in the reference): U's and V's planes are given blocks of different
    // physical regions of HBM (at most `candidates` extra blocks drawn); planes that move keep their contents
    void place(int32_t candidates)
    {
        gs_field *planes[4] = {u_.in().raw(), v_.in().raw(), u_.out().raw(), v_.out().raw()};
        check(gs_fields_place(context_->get(), planes, candidates, nullptr, nullptr));
    }
    void flip()
    {
        u_.flip(context_);
        v_.flip(context_);
    }
    Evolving &u() { return u_; }
    Evolving &v() { return v_; }
    // (U, V) summaries of the current state over the whole global grid, in one call (gs_fields_summarize; blocking,
    // collective in a multi-process context)
    std::pair<Summary, Summary> summary()
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        gs_summary out[2];
        check(gs_fields_summarize(context_->get(), planes, 2, out));
        const Shape s = shape();
        return {Summary::from_c(out[0], s[0] * s[1]), Summary::from_c(out[1], s[0] * s[1])};
    }
    // (U, V) histograms of the current state over the whole global grid, in one call (gs_fields_histogram; blocking,
    // collective in a multi-process context): `bins` equal bins of u_range for U and of v_range for V
    std::pair<Histogram, Histogram> histogram(int32_t bins = 256, std::array<float, 2> u_range = {0.0f, 1.0f},
                                              std::array<float, 2> v_range = {0.0f, 0.5f})
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        const float lo[2] = {u_range[0], v_range[0]}, hi[2] = {u_range[1], v_range[1]};
        std::vector<uint64_t> out(2 * (std::size_t)(bins > 0 ? bins + 3 : 3));
        check(gs_fields_histogram(context_->get(), planes, 2, lo, hi, bins, out.data()));
        const Shape s = shape();
        return {Histogram::from_c(out.data(), bins, lo[0], hi[0], s[0] * s[1]),
                Histogram::from_c(out.data() + bins + 3, bins, lo[1], hi[1], s[0] * s[1])};
    }
    // (U, V) bit-quad counts of the current state over the whole global grid, in one call (gs_fields_morphology; blocking,
    // collective in a multi-process context): one Morphology per threshold (1..4 per species, the same number for both), U
    // set where it is below its thresholds and V where it is above, unless the senses say otherwise
    std::pair<std::vector<Morphology>, std::vector<Morphology>> morphology(const std::vector<float> &v_thresholds,
                                                                           const std::vector<float> &u_thresholds,
                                                                           bool v_above = true, bool u_above = false)
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        const std::size_t nt = v_thresholds.size();
        const std::vector<float> t = detail::uv_thresholds(u_thresholds, v_thresholds);
        const int32_t sense[2] = {u_above ? 1 : 0, v_above ? 1 : 0};
        std::vector<gs_morphology> out(2 * nt + 1);
        check(gs_fields_morphology(context_->get(), planes, 2, t.data(), sense, (int32_t)nt, out.data()));
        const Shape s = shape();
        std::pair<std::vector<Morphology>, std::vector<Morphology>> uv;
        for (std::size_t k = 0; k < nt; ++k) {
            uv.first.push_back(Morphology::from_c(out[k], t[k], u_above, s[0] * s[1]));
            uv.second.push_back(Morphology::from_c(out[nt + k], t[nt + k], v_above, s[0] * s[1]));
        }
        return uv;
    }
    // (U, V) summaries of every region of rh x rw cells of the current state, in one call (gs_fields_region_summaries;
    // blocking, collective in a multi-process context)
    std::pair<RegionSummaries, RegionSummaries> region_summaries(int32_t rh, int32_t rw)
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        const Shape s = shape();
        uint64_t rr = 0, rc = 0;
        check(gs_region_grid(s[0], s[1], rh, rw, &rr, &rc));
        const std::size_t regions = (std::size_t)(rr * rc);
        std::vector<gs_summary> out(2 * regions + 1);
        check(gs_fields_region_summaries(context_->get(), planes, 2, rh, rw, out.data()));
        std::pair<RegionSummaries, RegionSummaries> uv;
        RegionSummaries *both[2] = {&uv.first, &uv.second};
        for (std::size_t p = 0; p < 2; ++p) {
            *both[p] = RegionSummaries{rr, rc, rh, rw, {}};
            for (std::size_t r = 0; r < regions; ++r)
                both[p]->results.push_back(Summary::from_c(out[p * regions + r], detail::region_cells(s[0], s[1], rh, rw, r / rc, r % rc)));
        }
        return uv;
    }
    // (U, V) bit-quad counts of every region of rh x rw cells of the current state, in one call (gs_fields_region_morphology;
    // blocking, collective in a multi-process context): one RegionMorphology per threshold, thresholds and senses as for
    // morphology()
    std::pair<std::vector<RegionMorphology>, std::vector<RegionMorphology>> region_morphology(int32_t rh, int32_t rw,
                                                                                              const std::vector<float> &v_thresholds,
                                                                                              const std::vector<float> &u_thresholds,
                                                                                              bool v_above = true, bool u_above = false)
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        const std::size_t nt = v_thresholds.size();
        const std::vector<float> t = detail::uv_thresholds(u_thresholds, v_thresholds);
        const int32_t sense[2] = {u_above ? 1 : 0, v_above ? 1 : 0};
        const Shape s = shape();
        uint64_t rr = 0, rc = 0;
        check(gs_region_grid(s[0], s[1], rh, rw, &rr, &rc));
        const std::size_t regions = (std::size_t)(rr * rc);
        std::vector<gs_morphology> out(2 * regions * nt + 1);
        check(gs_fields_region_morphology(context_->get(), planes, 2, rh, rw, t.data(), sense, (int32_t)nt, out.data()));
        std::pair<std::vector<RegionMorphology>, std::vector<RegionMorphology>> uv;
        std::vector<RegionMorphology> *both[2] = {&uv.first, &uv.second};
        for (std::size_t p = 0; p < 2; ++p)
            for (std::size_t k = 0; k < nt; ++k) {
                RegionMorphology m{rr, rc, rh, rw, {}};
                for (std::size_t r = 0; r < regions; ++r)
                    m.results.push_back(Morphology::from_c(out[(p * regions + r) * nt + k], t[p * nt + k], p ? v_above : u_above,
                                                           detail::region_cells(s[0], s[1], rh, rw, r / rc, r % rc)));
                both[p]->push_back(std::move(m));
            }
        return uv;
    }
    // (U, V) connected components of the current state over the whole global grid, in one call (gs_fields_components; blocking,
    // collective in a multi-process context): one Components per threshold (1..4 per species, the same number for both), U set
    // where it is below its thresholds and V where it is above, as morphology() has it; connectivity 4 or 8
    std::pair<std::vector<Components>, std::vector<Components>> components(const std::vector<float> &v_thresholds,
                                                                           const std::vector<float> &u_thresholds,
                                                                           int32_t connectivity = 8)
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        const std::size_t nt = v_thresholds.size();
        const std::vector<float> t = detail::uv_thresholds(u_thresholds, v_thresholds);
        const int32_t sense[2] = {0, 1};
        std::vector<gs_components> out(2 * nt + 1);
        check(gs_fields_components(context_->get(), planes, 2, t.data(), sense, (int32_t)nt, connectivity, out.data()));
        std::pair<std::vector<Components>, std::vector<Components>> uv;
        for (std::size_t k = 0; k < nt; ++k) {
            uv.first.push_back(Components::from_c(out[k], t[k], false, connectivity));
            uv.second.push_back(Components::from_c(out[nt + k], t[nt + k], true, connectivity));
        }
        return uv;
    }
    // (U, V) connected components of every region of rh x rw cells of the current state, in one call
    // (gs_fields_region_components; blocking, collective in a multi-process context): one RegionComponents per threshold,
    // thresholds and senses as for region_morphology(), a region's border being a wall; connectivity 4 or 8
    std::pair<std::vector<RegionComponents>, std::vector<RegionComponents>> region_components(int32_t rh, int32_t rw,
                                                                                              const std::vector<float> &v_thresholds,
                                                                                              const std::vector<float> &u_thresholds,
                                                                                              bool v_above = true, bool u_above = false,
                                                                                              int32_t connectivity = 8)
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        const std::size_t nt = v_thresholds.size();
        const std::vector<float> t = detail::uv_thresholds(u_thresholds, v_thresholds);
        const int32_t sense[2] = {u_above ? 1 : 0, v_above ? 1 : 0};
        const Shape s = shape();
        uint64_t rr = 0, rc = 0;
        check(gs_region_grid(s[0], s[1], rh, rw, &rr, &rc));
        const std::size_t regions = (std::size_t)(rr * rc);
        std::vector<gs_components> out(2 * regions * nt + 1);
        check(gs_fields_region_components(context_->get(), planes, 2, rh, rw, t.data(), sense, (int32_t)nt, connectivity, out.data()));
        std::pair<std::vector<RegionComponents>, std::vector<RegionComponents>> uv;
        std::vector<RegionComponents> *both[2] = {&uv.first, &uv.second};
        for (std::size_t p = 0; p < 2; ++p)
            for (std::size_t k = 0; k < nt; ++k) {
                RegionComponents c{rr, rc, rh, rw, {}};
                for (std::size_t r = 0; r < regions; ++r)
                    c.results.push_back(Components::from_c(out[(p * regions + r) * nt + k], t[p * nt + k], p ? v_above : u_above,
                                                           connectivity));
                both[p]->push_back(std::move(c));
            }
        return uv;
    }
    // where the spots are: one record per connected component of at least min_size cells of species (0 = U, 1 = V) of the
    // current state thresholded at `threshold`, over the whole global grid, in ascending order of the first cell
    // (gs_field_component_list; blocking, single-process contexts)
    std::vector<gs_component_record> component_list(float threshold = 0.25f, int32_t species = 1, bool above = true,
                                                    int32_t connectivity = 8, uint64_t min_size = 1)
    {
        if (species != 0 && species != 1) throw HipError(GS_ERR_INVALID, "species must be 0 (U) or 1 (V)");
        gs_component_list *list = nullptr;
        check(gs_field_component_list(context_->get(), species ? v_.in().raw() : u_.in().raw(), threshold, above ? 1 : 0,
                                      connectivity, min_size, &list));
        return detail::take_component_lists(list).at(0);
    }
    // what became of the spots since the snapshot: the component lists of species (0 = U, 1 = V) in the snapshot and in the
    // current state under one rule, and the overlaps of their components (gs_fields_match; blocking, single-process contexts)
    ComponentMatch match_since(Snapshot &snap, float threshold = 0.25f, int32_t species = 1, bool above = true,
                               int32_t connectivity = 8, uint64_t min_size = 1)
    {
        if (species != 0 && species != 1) throw HipError(GS_ERR_INVALID, "species must be 0 (U) or 1 (V)");
        gs_component_match *match = nullptr;
        check(gs_fields_match(context_->get(), species ? snap.v().raw() : snap.u().raw(), species ? v_.in().raw() : u_.in().raw(),
                              threshold, above ? 1 : 0, connectivity, min_size, &match));
        return detail::take_component_matches(match).at(0);
    }
    // (U, V) two-point pair counts of the current state over the whole global grid, in one call (gs_fields_correlation;
    // blocking, collective in a multi-process context): one Correlation per threshold (1..4 per species, the same number for
    // both), lags 0 .. max_lag (1..64), U set where it is below its thresholds and V where it is above, unless the senses say
    // otherwise
    std::pair<std::vector<Correlation>, std::vector<Correlation>> correlation(const std::vector<float> &v_thresholds,
                                                                             const std::vector<float> &u_thresholds,
                                                                             int32_t max_lag = 32, bool v_above = true,
                                                                             bool u_above = false)
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        const std::size_t nt = v_thresholds.size(), lags = max_lag >= 1 && max_lag <= 64 ? (std::size_t)max_lag + 1 : 1;
        const std::vector<float> t = detail::uv_thresholds(u_thresholds, v_thresholds);
        const int32_t sense[2] = {u_above ? 1 : 0, v_above ? 1 : 0};
        std::vector<uint64_t> out(2 * nt * 4 * lags + 1);
        check(gs_fields_correlation(context_->get(), planes, 2, t.data(), sense, (int32_t)nt, max_lag, out.data()));
        const Shape s = shape();
        std::pair<std::vector<Correlation>, std::vector<Correlation>> uv;
        for (std::size_t k = 0; k < nt; ++k) {
            uv.first.push_back(Correlation::from_c(out.data() + k * 4 * lags, max_lag, t[k], u_above, s[0], s[1]));
            uv.second.push_back(Correlation::from_c(out.data() + (nt + k) * 4 * lags, max_lag, t[nt + k], v_above, s[0], s[1]));
        }
        return uv;
    }
    // (U, V) tile-averaged power spectra of the current state over the whole global grid, in one call (gs_fields_spectrum;
    // blocking, collective in a multi-process context): tiles of `tile` (16, 32, 64, 128) cells a side, with the periodic Hann
    // window unless `hann` is false
    std::pair<Spectrum, Spectrum> spectrum(int32_t tile = 64, bool hann = true)
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        const std::size_t t = tile == 16 || tile == 32 || tile == 64 || tile == 128 ? (std::size_t)tile : 16;
        const std::size_t bins = t * (t / 2 + 1); // (a refused tile: the call returns before it writes)
        std::vector<double> power(2 * bins);
        uint64_t tiles[4] = {0, 0, 0, 0};
        check(gs_fields_spectrum(context_->get(), planes, 2, tile, hann ? 1 : 0, power.data(), tiles));
        return {Spectrum::from_c(power.data(), tiles, tile, hann ? 1 : 0), Spectrum::from_c(power.data() + bins, tiles + 2, tile, hann ? 1 : 0)};
    }
    // (U, V) two-point pair counts of every region of rh x rw cells of the current state, in one call
    // (gs_fields_region_correlation; blocking, collective in a multi-process context): one RegionCorrelation per threshold, a
    // region's border being a wall for pairs; thresholds, lags and senses as for correlation()
    std::pair<std::vector<RegionCorrelation>, std::vector<RegionCorrelation>> region_correlation(int32_t rh, int32_t rw,
                                                                                                 const std::vector<float> &v_thresholds,
                                                                                                 const std::vector<float> &u_thresholds,
                                                                                                 int32_t max_lag = 32, bool v_above = true,
                                                                                                 bool u_above = false)
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        const std::size_t nt = v_thresholds.size(), lags = max_lag >= 1 && max_lag <= 64 ? (std::size_t)max_lag + 1 : 1;
        const std::vector<float> t = detail::uv_thresholds(u_thresholds, v_thresholds);
        const int32_t sense[2] = {u_above ? 1 : 0, v_above ? 1 : 0};
        const Shape s = shape();
        uint64_t rr = 0, rc = 0;
        check(gs_region_grid(s[0], s[1], rh, rw, &rr, &rc));
        // (a result over the cap is refused by the call; nothing that large is allocated for it)
        const std::size_t regions = rr * rc * nt * 4 * lags <= (uint64_t)GS_REGION_PAIRS_MAX ? (std::size_t)(rr * rc) : 0;
        std::vector<uint64_t> out(2 * regions * nt * 4 * lags + 1);
        check(gs_fields_region_correlation(context_->get(), planes, 2, rh, rw, t.data(), sense, (int32_t)nt, max_lag, out.data()));
        std::pair<std::vector<RegionCorrelation>, std::vector<RegionCorrelation>> uv;
        std::vector<RegionCorrelation> *both[2] = {&uv.first, &uv.second};
        for (std::size_t p = 0; p < 2; ++p)
            for (std::size_t k = 0; k < nt; ++k) {
                RegionCorrelation c{rr, rc, rh, rw, {}};
                for (std::size_t r = 0; r < regions; ++r) {
                    const uint64_t h = detail::region_cells(s[0], 1, rh, 1, r / rc, 0), w = detail::region_cells(1, s[1], 1, rw, 0, r % rc);
                    c.results.push_back(Correlation::from_c(out.data() + ((p * regions + r) * nt + k) * 4 * lags, max_lag, t[p * nt + k],
                                                            p ? v_above : u_above, h, w));
                }
                both[p]->push_back(std::move(c));
            }
        return uv;
    }
    // (U, V) histograms of every region of rh x rw cells of the current state, in one call (gs_fields_region_histogram;
    // blocking, collective in a multi-process context): `bins` equal bins of u_range for U and of v_range for V
    std::pair<RegionHistogram, RegionHistogram> region_histogram(int32_t rh, int32_t rw, int32_t bins = 256,
                                                                 std::array<float, 2> u_range = {0.0f, 1.0f},
                                                                 std::array<float, 2> v_range = {0.0f, 1.0f})
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        const float lo[2] = {u_range[0], v_range[0]}, hi[2] = {u_range[1], v_range[1]};
        const std::size_t each = bins >= 1 && bins <= 4096 ? (std::size_t)bins + 3 : 3;
        const Shape s = shape();
        uint64_t rr = 0, rc = 0;
        check(gs_region_grid(s[0], s[1], rh, rw, &rr, &rc));
        // (a result over the cap is refused by the call; nothing that large is allocated for it)
        const std::size_t regions = rr * rc * each <= (uint64_t)GS_REGION_HIST_MAX ? (std::size_t)(rr * rc) : 0;
        std::vector<uint64_t> out(2 * regions * each + 1);
        check(gs_fields_region_histogram(context_->get(), planes, 2, rh, rw, lo, hi, bins, out.data()));
        std::pair<RegionHistogram, RegionHistogram> uv;
        RegionHistogram *both[2] = {&uv.first, &uv.second};
        for (std::size_t p = 0; p < 2; ++p) {
            *both[p] = RegionHistogram{rr, rc, rh, rw, {}};
            for (std::size_t r = 0; r < regions; ++r)
                both[p]->results.push_back(Histogram::from_c(out.data() + (p * regions + r) * each, bins, lo[p], hi[p],
                                                             detail::region_cells(s[0], s[1], rh, rw, r / rc, r % rc)));
        }
        return uv;
    }
    // (U, V) tile-averaged power spectra of every region of rh x rw cells of the current state, in one call
    // (gs_fields_region_spectrum; blocking, collective in a multi-process context): tile and window as for spectrum()
    std::pair<RegionSpectrum, RegionSpectrum> region_spectrum(int32_t rh, int32_t rw, int32_t tile = 64, bool hann = true)
    {
        gs_field *planes[2] = {u_.in().raw(), v_.in().raw()};
        const std::size_t t = tile == 16 || tile == 32 || tile == 64 || tile == 128 ? (std::size_t)tile : 16;
        const std::size_t bins = t * (t / 2 + 1); // (a refused tile: the call returns before it writes)
        const Shape s = shape();
        uint64_t rr = 0, rc = 0;
        check(gs_region_grid(s[0], s[1], rh, rw, &rr, &rc));
        // (a result over the cap is refused by the call; nothing that large is allocated for it)
        const std::size_t regions = rr * rc * (bins + 2) <= (uint64_t)GS_REGION_SPECTRUM_MAX ? (std::size_t)(rr * rc) : 0;
        std::vector<double> power(2 * regions * bins + 1);
        std::vector<uint64_t> tiles(4 * regions + 1);
        check(gs_fields_region_spectrum(context_->get(), planes, 2, rh, rw, tile, hann ? 1 : 0, power.data(), tiles.data()));
        std::pair<RegionSpectrum, RegionSpectrum> uv;
        RegionSpectrum *both[2] = {&uv.first, &uv.second};
        for (std::size_t p = 0; p < 2; ++p) {
            *both[p] = RegionSpectrum{rr, rc, rh, rw, {}};
            for (std::size_t r = 0; r < regions; ++r)
                both[p]->results.push_back(Spectrum::from_c(power.data() + (p * regions + r) * bins, tiles.data() + 2 * (p * regions + r),
                                                            tile, hann ? 1 : 0));
        }
        return uv;
    }
    // the current state copied into planes of its own on the device (gs_fields_copy; blocking)
    Snapshot snapshot()
    {
        Snapshot s(context_, shape());
        s.update(*this);
        return s;
    }
    // (U, V): how far the current state is from the snapshot (current minus snapshot), in one call (gs_fields_compare;
    // blocking, collective in a multi-process context)
    std::pair<Change, Change> change_since(Snapshot &snap)
    {
        gs_field *a[2] = {u_.in().raw(), v_.in().raw()}, *b[2] = {snap.u().raw(), snap.v().raw()};
        gs_change out[2];
        check(gs_fields_compare(context_->get(), a, b, 2, out));
        const Shape s = shape();
        return {Change::from_c(out[0], s[0] * s[1]), Change::from_c(out[1], s[0] * s[1])};
    }
    // (U, V): how far every region of rh x rw cells of the current state is from the same region of the snapshot (current
    // minus snapshot), in one call (gs_fields_region_compare; blocking, collective in a multi-process context)
    std::pair<RegionChange, RegionChange> region_changes_since(const Snapshot &snap, int32_t rh, int32_t rw)
    {
        gs_field *a[2] = {u_.in().raw(), v_.in().raw()}, *b[2] = {snap.u_.raw(), snap.v_.raw()};
        const Shape s = shape();
        uint64_t rr = 0, rc = 0;
        check(gs_region_grid(s[0], s[1], rh, rw, &rr, &rc));
        const std::size_t regions = (std::size_t)(rr * rc);
        std::vector<gs_change> out(2 * regions + 1);
        check(gs_fields_region_compare(context_->get(), a, b, 2, rh, rw, out.data()));
        std::pair<RegionChange, RegionChange> uv;
        RegionChange *both[2] = {&uv.first, &uv.second};
        for (std::size_t p = 0; p < 2; ++p) {
            both[p]->rr = rr;
            both[p]->rc = rc;
            both[p]->rh = rh;
            both[p]->rw = rw;
            for (std::size_t r = 0; r < regions; ++r)
                both[p]->results.push_back(Change::from_c(out[p * regions + r], detail::region_cells(s[0], s[1], rh, rw, r / rc, r % rc)));
        }
        return uv;
    }
    // go back to the snapshot: its planes are copied into the current in-planes (gs_fields_copy; blocking), and the next
    // perform_steps continues from the snapshot's bits
    void restore(Snapshot &snap)
    {
        gs_field *dst[2] = {u_.in().raw(), v_.in().raw()}, *src[2] = {snap.u().raw(), snap.v().raw()};
        check(gs_fields_copy(context_->get(), dst, src, 2));
    }
    std::vector<Precision> make_result_view() { return v_.in().make_scalar_view(context_); }
    void write_result_view(Precision *target, Shape target_shape)
    {
        v_.in().write_scalar_view(context_, target, target_shape);
    }
    void write_result_view_after(PinnedImage &image)
    {
        v_.in().write_scalar_view_after(context_, image.data(), image.shape());
    }

  private:
    Species(Context c, Evolving u, Evolving v) : context_(std::move(c)), u_(std::move(u)), v_(std::move(v)) {}
    Context context_;
    Evolving u_, v_;
};

inline void Snapshot::update(Species &species)
{
    gs_field *dst[2] = {u_.raw(), v_.raw()}, *src[2] = {species.u().in().raw(), species.v().in().raw()};
    check(gs_fields_copy(context_->get(), dst, src, 2));
}

// Ensemble (gs_ensemble_*): `members` independent grids of one shape on one context, each with its own Parameters and its
// own U and V; member i evolves bit for bit as a lone Species with its parameters would.  The ensemble tracks its current
// slot itself.  Host arrays are dense [count, rows, cols].
class Ensemble {
  public:
    // members with params[i] each (params.size() == members) or params[0] for all (params.size() == 1); seeded with
    // Species::new's pattern when `seed`, else zeros
    Ensemble(Context ctx, std::size_t members, Shape shape, const std::vector<Parameters> &params, bool seed = true)
        : ctx_(std::move(ctx)), members_(members), shape_(shape)
    {
        check(gs_ensemble_create(ctx_->get(), &e_, members, shape[0], shape[1]));
        try {
            set_params(params);
            if (seed) check(gs_ensemble_seed(ctx_->get(), e_));
        } catch (...) {
            gs_ensemble_destroy(ctx_->get(), e_);
            throw;
        }
    }
    ~Ensemble()
    {
        if (e_) gs_ensemble_destroy(ctx_->get(), e_);
    }
    Ensemble(const Ensemble &) = delete;
    Ensemble &operator=(const Ensemble &) = delete;
    Ensemble(Ensemble &&o) noexcept : ctx_(std::move(o.ctx_)), e_(o.e_), members_(o.members_), shape_(o.shape_) { o.e_ = nullptr; }

    std::size_t members() const { return members_; }
    Shape shape() const { return shape_; }
    gs_ensemble *raw() const { return e_; }
    const Context &context() const { return ctx_; }
    void set_params(const std::vector<Parameters> &params)
    {
        std::vector<gs_params> c;
        for (const Parameters &p : params) c.push_back(p.to_c());
        check(gs_ensemble_set_params(ctx_->get(), e_, c.data(), c.size()));
    }
    // u or v may be null: that species stays as it is
    void upload(std::size_t first, std::size_t count, const float *u, const float *v)
    {
        check(gs_ensemble_upload(ctx_->get(), e_, first, count, u, v));
    }
    // species 0 = U, 1 = V of members [first, first + count)
    std::vector<float> download(std::size_t first, std::size_t count, int species = 1) const
    {
        std::vector<float> out(count * shape_[0] * shape_[1]);
        check(gs_ensemble_download(ctx_->get(), e_, first, count, species, out.data()));
        return out;
    }
    void prepare_steps(std::size_t steps) { check(gs_ensemble_run(ctx_->get(), e_, steps)); }
    void perform_steps(std::size_t steps)
    {
        prepare_steps(steps);
        ctx_->sync();
    }
    // active flags of members [first, first + mask.size()) (gs_members_set_active, blocking; nonzero = active): the steps
    // advance the active members only, an inactive member keeps its state -- every reader sees it -- and its step count
    void set_active(const std::vector<uint8_t> &mask, std::size_t first = 0)
    {
        check(gs_members_set_active(ctx_->get(), e_, first, mask.size(), mask.data()));
    }
    // the active flags (0 or 1) of all members
    std::vector<uint8_t> active() const
    {
        std::vector<uint8_t> out(members_);
        check(gs_members_get_active(ctx_->get(), e_, 0, members_, out.data(), nullptr, nullptr));
        return out;
    }
    // the steps every member has been advanced by since the ensemble was made
    std::vector<uint64_t> steps_taken() const
    {
        std::vector<uint64_t> out(members_);
        check(gs_members_get_active(ctx_->get(), e_, 0, members_, nullptr, out.data(), nullptr));
        return out;
    }
    // noise of members [first, first + noise.size()) (gs_members_set_noise, blocking), one struct per member: its sigmas,
    // its seed and the index of its next step, which advances with the steps that member takes.  The first call attaches
    // noise to the ensemble (members never named: sigmas 0, seed 0, step 0); Simulation::set_noise never touches an ensemble
    void set_noise(const std::vector<gs_noise> &noise, std::size_t first = 0)
    {
        check(gs_members_set_noise(ctx_->get(), e_, first, noise.size(), noise.data(), noise.size()));
    }
    // ... and one struct for all of members [first, first + count)
    void set_noise(const gs_noise &noise, std::size_t first, std::size_t count)
    {
        check(gs_members_set_noise(ctx_->get(), e_, first, count, &noise, 1));
    }
    // every member's struct with its current step; empty when the ensemble has no noise (gs_members_get_noise)
    std::vector<gs_noise> noise() const
    {
        std::vector<gs_noise> out(members_);
        int32_t attached = 0;
        check(gs_members_get_noise(ctx_->get(), e_, 0, members_, out.data(), &attached));
        if (!attached) out.clear();
        return out;
    }
    // detach: the next run launches the kernels of an ensemble without noise
    void clear_noise() { check(gs_members_clear_noise(ctx_->get(), e_)); }
    // summaries of members [first, first + count) from the newest state (gs_members_summarize, blocking): element
    // 2 i = U, 2 i + 1 = V of member first + i, bit for bit what Species::summary gives for a lone Species in that state
    std::vector<Summary> summaries(std::size_t first, std::size_t count) const
    {
        std::vector<gs_summary> c(2 * count);
        check(gs_members_summarize(ctx_->get(), e_, first, count, c.data()));
        std::vector<Summary> out;
        for (const gs_summary &s : c) out.push_back(Summary::from_c(s, shape_[0] * shape_[1]));
        return out;
    }
    // histograms of members [first, first + count) from the newest state (gs_members_histogram, blocking): element
    // 2 i = U over u_range, 2 i + 1 = V over v_range of member first + i, what Species::histogram gives for a lone Species
    // in that state
    std::vector<Histogram> histograms(std::size_t first, std::size_t count, int32_t bins = 256,
                                      std::array<float, 2> u_range = {0.0f, 1.0f},
                                      std::array<float, 2> v_range = {0.0f, 0.5f}) const
    {
        const float lo[2] = {u_range[0], v_range[0]}, hi[2] = {u_range[1], v_range[1]};
        const std::size_t each = (std::size_t)(bins > 0 ? bins + 3 : 3);
        std::vector<uint64_t> c(2 * count * each);
        check(gs_members_histogram(ctx_->get(), e_, first, count, lo, hi, bins, c.data()));
        std::vector<Histogram> out;
        for (std::size_t i = 0; i < 2 * count; ++i)
            out.push_back(Histogram::from_c(c.data() + i * each, bins, lo[i & 1], hi[i & 1], shape_[0] * shape_[1]));
        return out;
    }
    // bit-quad counts of members [first, first + count) from the newest state (gs_members_morphology, blocking): element
    // (2 i + s) * nt + k = species s (0 = U, 1 = V) of member first + i at that species' threshold k, what
    // Species::morphology gives for a lone Species in that state
    std::vector<Morphology> morphologies(std::size_t first, std::size_t count, const std::vector<float> &v_thresholds,
                                         const std::vector<float> &u_thresholds, bool v_above = true, bool u_above = false) const
    {
        const std::size_t nt = v_thresholds.size();
        const std::vector<float> t = detail::uv_thresholds(u_thresholds, v_thresholds);
        const int32_t sense[2] = {u_above ? 1 : 0, v_above ? 1 : 0};
        std::vector<gs_morphology> c(2 * count * nt + 1);
        check(gs_members_morphology(ctx_->get(), e_, first, count, t.data(), sense, (int32_t)nt, c.data()));
        std::vector<Morphology> out;
        for (std::size_t i = 0; i < 2 * count * nt; ++i) {
            const std::size_t species = (i / nt) & 1, k = i % nt;
            out.push_back(Morphology::from_c(c[i], t[species * nt + k], sense[species] != 0, shape_[0] * shape_[1]));
        }
        return out;
    }
    // connected components of members [first, first + count) from the newest state (gs_members_components, blocking): element
    // (2 i + s) * nt + k = species s (0 = U, set below; 1 = V, set above) of member first + i at that species' threshold k,
    // what Species::components gives for a lone Species in that state
    std::vector<Components> components(std::size_t first, std::size_t count, const std::vector<float> &v_thresholds,
                                       const std::vector<float> &u_thresholds, int32_t connectivity = 8) const
    {
        const std::size_t nt = v_thresholds.size();
        const std::vector<float> t = detail::uv_thresholds(u_thresholds, v_thresholds);
        const int32_t sense[2] = {0, 1};
        std::vector<gs_components> c(2 * count * nt + 1);
        check(gs_members_components(ctx_->get(), e_, first, count, t.data(), sense, (int32_t)nt, connectivity, c.data()));
        std::vector<Components> out;
        for (std::size_t i = 0; i < 2 * count * nt; ++i) {
            const std::size_t species = (i / nt) & 1, k = i % nt;
            out.push_back(Components::from_c(c[i], t[species * nt + k], species != 0, connectivity));
        }
        return out;
    }
    // component lists of members [first, first + count) from the newest state (gs_members_component_list, blocking): element i
    // = the records of species (0 = U, 1 = V) of member first + i, what Species::component_list gives for a lone Species in that
    // state; rows are the member's own
    std::vector<std::vector<gs_component_record>> component_lists(std::size_t first, std::size_t count, float threshold = 0.25f,
                                                                  int32_t species = 1, bool above = true,
                                                                  int32_t connectivity = 8, uint64_t min_size = 1) const
    {
        gs_component_list *list = nullptr;
        check(gs_members_component_list(ctx_->get(), e_, first, count, species, threshold, above ? 1 : 0, connectivity, min_size,
                                        &list));
        return detail::take_component_lists(list);
    }
    // what became of the spots of members [first, first + count) since the same members of ref (gs_members_match, blocking):
    // element i = member first + i of ref as `before` against member first + i of this ensemble as `after`, what
    // Species::match_since gives for lone Species in those states
    std::vector<ComponentMatch> matches_since(const Ensemble &ref, std::size_t first, std::size_t count, float threshold = 0.25f,
                                              int32_t species = 1, bool above = true, int32_t connectivity = 8,
                                              uint64_t min_size = 1) const
    {
        gs_component_match *match = nullptr;
        check(gs_members_match(ctx_->get(), ref.e_, e_, first, count, species, threshold, above ? 1 : 0, connectivity, min_size,
                               &match));
        return detail::take_component_matches(match);
    }
    // two-point pair counts of members [first, first + count) from the newest state (gs_members_correlation, blocking):
    // element (2 i + s) * nt + j = species s (0 = U, 1 = V) of member first + i at that species' threshold j, what
    // Species::correlation gives for a lone Species in that state
    std::vector<Correlation> correlations(std::size_t first, std::size_t count, const std::vector<float> &v_thresholds,
                                          const std::vector<float> &u_thresholds, int32_t max_lag = 32, bool v_above = true,
                                          bool u_above = false) const
    {
        const std::size_t nt = v_thresholds.size(), lags = max_lag >= 1 && max_lag <= 64 ? (std::size_t)max_lag + 1 : 1;
        const std::vector<float> t = detail::uv_thresholds(u_thresholds, v_thresholds);
        const int32_t sense[2] = {u_above ? 1 : 0, v_above ? 1 : 0};
        std::vector<uint64_t> c(2 * count * nt * 4 * lags + 1);
        check(gs_members_correlation(ctx_->get(), e_, first, count, t.data(), sense, (int32_t)nt, max_lag, c.data()));
        std::vector<Correlation> out;
        for (std::size_t i = 0; i < 2 * count * nt; ++i) {
            const std::size_t species = (i / nt) & 1, j = i % nt;
            out.push_back(Correlation::from_c(c.data() + i * 4 * lags, max_lag, t[species * nt + j], sense[species] != 0, shape_[0],
                                              shape_[1]));
        }
        return out;
    }
    // tile-averaged power spectra of members [first, first + count) from the newest state (gs_members_spectrum, blocking):
    // element 2 i + s = species s (0 = U, 1 = V) of member first + i, what Species::spectrum gives for a lone Species in
    // that state
    std::vector<Spectrum> spectra(std::size_t first, std::size_t count, int32_t tile = 64, bool hann = true) const
    {
        const std::size_t t = tile == 16 || tile == 32 || tile == 64 || tile == 128 ? (std::size_t)tile : 16;
        const std::size_t bins = t * (t / 2 + 1);
        std::vector<double> power(2 * count * bins + 1);
        std::vector<uint64_t> tiles(4 * count + 1);
        check(gs_members_spectrum(ctx_->get(), e_, first, count, tile, hann ? 1 : 0, power.data(), tiles.data()));
        std::vector<Spectrum> out;
        for (std::size_t i = 0; i < 2 * count; ++i)
            out.push_back(Spectrum::from_c(power.data() + i * bins, tiles.data() + 2 * i, tile, hann ? 1 : 0));
        return out;
    }
    // an ensemble of the same shape and member count on the same context whose members hold this one's current states
    // (gs_members_copy; blocking): a store of states for changes_since and copy_from, with the context's parameters
    Ensemble snapshot() const
    {
        Ensemble snap(ctx_, members_, shape_);
        snap.copy_from(*this, 0, members_);
        return snap;
    }
    // members [first, first + count) of src's newest state into the same members of this ensemble (gs_members_copy,
    // device to device, blocking)
    void copy_from(const Ensemble &src, std::size_t first, std::size_t count)
    {
        check(gs_members_copy(ctx_->get(), e_, src.e_, first, count));
    }
    // how far members [first, first + count) are from the same members of ref (gs_members_compare, blocking): element
    // 2 i = U, 2 i + 1 = V of member first + i, bit for bit what Species::change_since gives for lone Species in those states
    std::vector<Change> changes_since(const Ensemble &ref, std::size_t first, std::size_t count) const
    {
        std::vector<gs_change> c(2 * count);
        check(gs_members_compare(ctx_->get(), e_, ref.e_, first, count, c.data()));
        std::vector<Change> out;
        for (const gs_change &x : c) out.push_back(Change::from_c(x, shape_[0] * shape_[1]));
        return out;
    }
    // per-cell statistics ACROSS members (gs_members_bundle_stats, blocking): every run of `span` consecutive members of
    // [first, first + count) is a bundle, and result which[i] (GS_TSTAT_MEAN .. GS_TSTAT_OCCUPANCY) of bundle b becomes
    // member b of the i-th ensemble returned -- count / span members, the context's parameters, as snapshot() --, U from the
    // members' U and V from their V: bit for bit the time statistics of a lone Species sampled through the members' states.
    // The occupancy needs thresholds = {U's, V's} and above = {U's, V's} (set above it)
    std::vector<Ensemble> bundle_stats(std::size_t span, const std::vector<int32_t> &which, const std::vector<float> &thresholds = {},
                                       const std::vector<int32_t> &above = {}, std::size_t first = 0,
                                       std::size_t count = (std::size_t)-1) const
    {
        if (count == (std::size_t)-1) count = members_ - first;
        if ((!thresholds.empty() && thresholds.size() != 2) || above.size() != thresholds.size())
            throw HipError(GS_ERR_INVALID, "bundle statistics: thresholds and above are {U's, V's}, or both empty");
        const std::size_t bundles = span ? count / span : 0;
        std::vector<Ensemble> out;
        std::vector<gs_ensemble *> raw;
        for (std::size_t i = 0; i < which.size(); ++i) {
            out.push_back(Ensemble(ctx_, bundles ? bundles : 1, shape_));
            raw.push_back(out.back().e_);
        }
        check(gs_members_bundle_stats(ctx_->get(), e_, first, count, span, which.data(), (int32_t)which.size(),
                                      thresholds.empty() ? nullptr : thresholds.data(), above.empty() ? nullptr : above.data(),
                                      raw.data(), 0));
        return out;
    }

  private:
    // all members zero, every member with the context's parameters (snapshot)
    Ensemble(Context ctx, std::size_t members, Shape shape) : ctx_(std::move(ctx)), members_(members), shape_(shape)
    {
        check(gs_ensemble_create(ctx_->get(), &e_, members, shape[0], shape[1]));
    }
    Context ctx_;
    gs_ensemble *e_ = nullptr;
    std::size_t members_;
    Shape shape_;
};

// Time statistics (gs_time_stats_*): per-cell accumulators over the samples of a run, kept on the device.  `groups` is a sum
// of GS_TSTAT_SUM, _SQUARES, _EXTREMES, _CROSSINGS; crossings need a threshold per species (thresholds = {U's, V's}; above[i]:
// set above it).  accumulate(stamp) between perform_steps calls; for a Species the result planes are HipConcentrations (every
// observable, reduced download and colour map applies), for an Ensemble dense [count, rows, cols] host arrays.  No standard
// deviation is formed on the device: take the square root of the variance read.
class TimeStats {
  public:
    TimeStats(Species &species, uint32_t groups, const std::vector<float> &thresholds = {}, const std::vector<int32_t> &above = {})
        : ctx_(species.context()), species_(&species), shape_(species.shape())
    {
        check_rule(groups, thresholds, above);
        check(gs_time_stats_create(ctx_->get(), &ts_, shape_[0], shape_[1], 2, groups, thresholds.empty() ? nullptr : thresholds.data(),
                                   above.empty() ? nullptr : above.data()));
    }
    TimeStats(Ensemble &ensemble, uint32_t groups, const std::vector<float> &thresholds = {}, const std::vector<int32_t> &above = {},
              std::size_t first = 0, std::size_t count = (std::size_t)-1)
        : ctx_(ensemble.context()), ensemble_(&ensemble), shape_(ensemble.shape()),
          count_(count == (std::size_t)-1 ? ensemble.members() - first : count)
    {
        check_rule(groups, thresholds, above);
        check(gs_members_time_stats_create(ctx_->get(), &ts_, ensemble.raw(), first, count_, groups,
                                           thresholds.empty() ? nullptr : thresholds.data(), above.empty() ? nullptr : above.data()));
    }
    ~TimeStats()
    {
        if (ts_) gs_time_stats_destroy(ctx_->get(), ts_);
    }
    TimeStats(const TimeStats &) = delete;
    TimeStats &operator=(const TimeStats &) = delete;
    TimeStats(TimeStats &&o) noexcept
        : ctx_(std::move(o.ctx_)), ts_(o.ts_), species_(o.species_), ensemble_(o.ensemble_), shape_(o.shape_), count_(o.count_)
    {
        o.ts_ = nullptr;
    }
    // one sample of the source's current state (waits for the steps enqueued, enqueues one launch per slab, returns)
    void accumulate(uint32_t stamp)
    {
        if (ensemble_) {
            check(gs_members_time_stats_accumulate(ctx_->get(), ts_, ensemble_->raw(), stamp));
        } else {
            gs_field *planes[2] = {species_->u().in().raw(), species_->v().in().raw()};
            check(gs_time_stats_accumulate(ctx_->get(), ts_, planes, 2, stamp));
        }
    }
    uint64_t samples() const
    {
        uint64_t n = 0;
        check(gs_time_stats_samples(ts_, &n));
        return n;
    }
    void reset() { check(gs_time_stats_reset(ctx_->get(), ts_)); }
    // result plane `which` (GS_TSTAT_MEAN .. GS_TSTAT_ARRIVAL) of species 0 = U, 1 = V of a Species' statistics
    HipConcentration result(int32_t species, int32_t which)
    {
        HipConcentration out = HipConcentration::default_(ctx_, shape_);
        check(gs_time_stats_result(ctx_->get(), ts_, species, which, out.raw()));
        return out;
    }
    HipConcentration mean(int32_t species = 1) { return result(species, GS_TSTAT_MEAN); }
    HipConcentration variance(int32_t species = 1) { return result(species, GS_TSTAT_VARIANCE); }
    HipConcentration min(int32_t species = 1) { return result(species, GS_TSTAT_MIN); }
    HipConcentration max(int32_t species = 1) { return result(species, GS_TSTAT_MAX); }
    HipConcentration occupancy(int32_t species = 1) { return result(species, GS_TSTAT_OCCUPANCY); }
    HipConcentration arrival(int32_t species = 1) { return result(species, GS_TSTAT_ARRIVAL); }
    // ... of an Ensemble's: [count, rows, cols]
    std::vector<float> members_result(int32_t species, int32_t which)
    {
        std::vector<float> out(count_ * shape_[0] * shape_[1]);
        check(gs_members_time_stats_result(ctx_->get(), ts_, species, which, out.data()));
        return out;
    }
    // a raw accumulator (GS_TSTAT_RAW_SUM ..: T = double, float or uint32_t to match) of this process's rows, dense
    template <typename T>
    std::vector<T> raw(int32_t species, int32_t raw_plane)
    {
        const bool wide = raw_plane == GS_TSTAT_RAW_SUM || raw_plane == GS_TSTAT_RAW_SQUARES;
        if (sizeof(T) != (wide ? 8u : 4u)) throw std::logic_error("TimeStats::raw: element type does not match the accumulator");
        std::size_t rows = count_ * shape_[0];
        if (species_) {
            uint64_t r0 = 0, r1 = 0;
            check(gs_field_local_rows(species_->u().in().raw(), &r0, &r1));
            rows = (std::size_t)(r1 - r0);
        }
        std::vector<T> out(rows * shape_[1]);
        check(gs_time_stats_download(ctx_->get(), ts_, species, raw_plane, out.data()));
        return out;
    }

  private:
    static void check_rule(uint32_t groups, const std::vector<float> &thresholds, const std::vector<int32_t> &above)
    {
        if ((groups & GS_TSTAT_CROSSINGS) && (thresholds.size() != 2 || above.size() != 2))
            throw std::logic_error("TimeStats: crossings need two thresholds and two senses (U's, V's)");
    }
    Context ctx_;
    gs_time_stats *ts_ = nullptr;
    Species *species_ = nullptr;
    Ensemble *ensemble_ = nullptr;
    Shape shape_{};
    std::size_t count_ = 1;
};

class Simulation {
  public:
    using CliArgs = HipArgs;
    // SimulateCreate::new
    static Simulation new_(const Parameters &params, const HipArgs &args = HipArgs())
    {
        return Simulation(std::make_shared<HipContext>(params, args));
    }
    // SimulateBase::make_species
    Species make_species(Shape shape) const
    {
        Species s = Species::new_(context_, shape);
        // planes of >= 256 MiB: below, they largely stay in the last-level cache and where they lie does not show
        if (context_->place_candidates() > 0 && (uint64_t)shape[0] * (uint64_t)shape[1] >= (1ull << 26))
            s.place(context_->place_candidates());
        return s;
    }
    // Simulate::perform_steps: the steps are DONE on return (as in every backend of the reference:
    // compute/shared/src/gpu/mod.rs:77-91 ends in a fence wait); results end up in the input slots
    void perform_steps(Species &species, std::size_t steps) const
    {
        prepare_steps(species, steps);
        check(gs_sync(context_->get()));
    }
    // SimulateGpu::prepare_steps (compute/shared/src/gpu/mod.rs:70-75): enqueue only; a download or
    // gs_sync waits.  HIP streams order the work, so no future object is passed along.
    void prepare_steps(Species &species, std::size_t steps) const
    {
        int32_t slot = 0;
        check(gs_run(context_->get(), species.u().in().raw(), species.v().in().raw(), species.u().out().raw(),
                     species.v().out().raw(), steps, &slot));
        if (slot == 1) {
            species.u().swap_slots();
            species.v().swap_slots();
        }
    }
    // SimulateStep::perform_step (compute/shared/src/cpu.rs:21-28): one gs_step, then flip
    void perform_step(Species &species) const
    {
        check(gs_step(context_->get(), species.u().in().raw(), species.v().in().raw(), species.u().out().raw(),
                      species.v().out().raw()));
        species.flip();
    }
    // Parameter map (gs_ctx_set_param_map): feed and kill of every cell, dense row-major [rows, cols] arrays of the GLOBAL
    // grid (each process uploads its own rows); the library copies them.  clear_param_map() detaches it.
    void set_param_map(Shape shape, const float *feed, const float *kill) const
    {
        Context c = context_;
        HipConcentration f = HipConcentration::zeros(c, shape), k = HipConcentration::zeros(c, shape);
        uint64_t r0 = 0, r1 = 0;
        check(gs_field_local_rows(f.raw(), &r0, &r1));
        check(gs_field_upload(context_->get(), f.raw(), feed + r0 * shape[1]));
        check(gs_field_upload(context_->get(), k.raw(), kill + r0 * shape[1]));
        check(gs_ctx_set_param_map(context_->get(), f.raw(), k.raw()));
    }
    void clear_param_map() const { check(gs_ctx_set_param_map(context_->get(), nullptr, nullptr)); }
    // Domain mask (gs_ctx_set_mask): a dense row-major [rows, cols] array of the GLOBAL grid, nonzero (NaN included) =
    // wall (each process uploads its own rows); the library copies it.  clear_mask() detaches it.
    void set_mask(Shape shape, const float *mask) const
    {
        Context c = context_;
        HipConcentration m = HipConcentration::zeros(c, shape);
        uint64_t r0 = 0, r1 = 0;
        check(gs_field_local_rows(m.raw(), &r0, &r1));
        check(gs_field_upload(context_->get(), m.raw(), mask + r0 * shape[1]));
        check(gs_ctx_set_mask(context_->get(), m.raw()));
    }
    void clear_mask() const { check(gs_ctx_set_mask(context_->get(), nullptr)); }
    // Noise (gs_ctx_set_noise): every step adds sigma * xi per species, xi uniform on [-1, 1) and a pure function of (seed,
    // step index, global row, global column); `step` is the index of the next step.  noise() returns the term in force with
    // the current step -- saved with a snapshot it continues the run exactly -- or nothing; clear_noise() detaches it.
    void set_noise(float sigma_u, float sigma_v = 0.0f, uint64_t seed = 0, uint64_t step = 0) const
    {
        const gs_noise n{sigma_u, sigma_v, seed, step};
        check(gs_ctx_set_noise(context_->get(), &n));
    }
    void clear_noise() const { check(gs_ctx_set_noise(context_->get(), nullptr)); }
    bool noise(gs_noise *out) const
    {
        int32_t attached = 0;
        check(gs_ctx_get_noise(context_->get(), out, &attached));
        return attached != 0;
    }
    const Context &context() const { return context_; }
    // an Ensemble of params.size() members (Species::new's pattern in each)
    Ensemble make_ensemble(Shape shape, const std::vector<Parameters> &params) const
    {
        return Ensemble(context_, params.size(), shape, params);
    }

  private:
    explicit Simulation(Context c) : context_(std::move(c)) {}
    Context context_;
};

} // namespace gs
