// plane_scan.cpp -- three device-free checks of grayscott_amd/csrc/gs_plane_scan.h, the header the plane-scanning kernels share:
//   1. gs_is_set with the launchers' gs_set_rule against the rule as include/gs_hip.h words it -- a cell is set when it is
//      above the threshold, or with the other sense below it, NaN never -- written out here independently, over every pair
//      of the cells and thresholds that can tell a sign flip from a comparison: NaN, +-0, +-inf, +-FLT_MIN, a sub-normal,
//      +-1, 0.25 and its two neighbours;
//   2. gs_scan_groups by its properties, with each kernel's floor;
//   3. gs_plane_set's verdict on 16-byte loads against a table written by hand.
// Exit status 0 and "ok" when everything agrees.  Stand-alone: it links nothing of the library.
#include "../../grayscott_amd/csrc/gs_plane_scan.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <limits>
#include <vector>

namespace {

int failures = 0;

void expect(bool ok, const char *what, double a = 0, double b = 0, double c = 0, double d = 0)
{
    if (ok) return;
    std::fprintf(stderr, "FAILED %s (%g, %g, %g, %g)\n", what, a, b, c, d);
    ++failures;
}

void check_set_rule()
{
    const float inf = std::numeric_limits<float>::infinity(), quarter = 0.25f;
    const std::vector<float> thresholds = {0.0f, -0.0f, inf, -inf, FLT_MIN, -FLT_MIN, std::ldexp(1.0f, -140), 1.0f, -1.0f,
                                           quarter, std::nextafter(quarter, 1.0f), std::nextafter(quarter, -1.0f)};
    std::vector<float> cells = thresholds;
    cells.push_back(std::numeric_limits<float>::quiet_NaN());
    for (const int32_t above : {1, 0})
        for (const float t : thresholds) {
            float rule_t[4][4];
            uint32_t rule_flip[4];
            const int32_t sense[1] = {above};
            gs_set_rules(rule_t, rule_flip, &t, sense, 1, 1); // (what the launchers call; through gs_set_rule)
            for (const float x : cells) {
                const bool want = std::isnan(x) ? false : (above ? x > t : x < t);
                expect(gs_is_set(x, rule_flip[0], rule_t[0][0]) == want, "gs_is_set(x, t, above)", x, t, above);
            }
        }
}

void check_groups()
{
    const int64_t floors[] = {2048 /* kHistUnitsPerGroup */, 4 * (int64_t(1) << 16) /* 4 kQuadUnitsPerWave */,
                              4 * (int64_t(1) << 12) /* 4 kPairUnitsPerWave */, 0 /* gs_comp_tally_k: none */};
    for (const int64_t units : {int64_t(1), int64_t(3), int64_t(4), int64_t(5), int64_t(1) << 20, int64_t(1) << 40})
        for (const int64_t max_groups : {int64_t(1), int64_t(2048), int64_t(8 * 256)})
            for (const int64_t nplanes : {int64_t(1), int64_t(2), int64_t(7), int64_t(1) << 20})
                for (const int64_t divisor : floors) {
                    int64_t groups = -1;
                    const bool ok = gs_scan_groups(units, divisor, max_groups, nplanes, groups);
                    const int64_t share = max_groups / nplanes > 1 ? max_groups / nplanes : 1;
                    const int64_t least = divisor ? (units + divisor - 1) / divisor : 0;
                    expect(groups >= 1, "groups >= 1", units, divisor, max_groups, nplanes);
                    expect(groups <= (share > least ? share : least), "groups <= max(share, least)", units, divisor, max_groups, nplanes);
                    expect(groups * 4 >= units || groups == share || groups == least, "no fewer than the units ask for without a reason",
                           units, divisor, max_groups, nplanes);
                    if (divisor) expect(groups * divisor >= units, "groups * divisor >= units", units, divisor, max_groups, nplanes);
                    expect(ok == (groups * nplanes <= INT32_MAX), "refused exactly when the grid exceeds INT32_MAX", units, divisor,
                           max_groups, nplanes);
                }
    // the tally's units are stretches of 64 entries: a workgroup per stretch of 256
    for (const int64_t cells : {int64_t(1), int64_t(256), int64_t(257), int64_t(1000003)}) {
        int64_t groups = -1;
        expect(gs_scan_groups((cells + 63) / 64, 0, int64_t(1) << 40, 1, groups) && groups == (cells + 255) / 256,
               "a workgroup per 256 entries", cells, groups);
    }
}

void check_vector_verdict()
{
    alignas(16) static float buffer[64];
    const float *aligned = buffer, *odd = buffer + 1, *half = buffer + 2;
    struct Case {
        const float *plane, *other;
        const float *also; // (null: none named)
        int64_t pitch, repeat, stride;
        bool want;
    };
    const Case table[] = {
        {aligned, aligned, nullptr, 256, 1, 0, true},   {aligned, aligned, nullptr, 256, 1, 221, true}, // repeat 1: any stride
        {aligned, aligned, nullptr, 256, 1, 224, true}, {aligned, aligned, nullptr, 258, 1, 0, false},  // pitch 258: rows drift
        {odd, aligned, nullptr, 256, 1, 0, false},      {aligned, odd, nullptr, 256, 1, 0, false},      // any plane odd
        {half, aligned, nullptr, 256, 1, 0, false},     {aligned, aligned, nullptr, 256, 3, 224, true},
        {aligned, aligned, nullptr, 256, 3, 221, false}, {aligned, aligned, nullptr, 258, 3, 224, false},
        {odd, aligned, nullptr, 256, 3, 224, false},    {aligned, aligned, aligned, 256, 1, 0, true},   // the rows above, too
        {aligned, aligned, odd, 256, 1, 0, false},      {odd, aligned, aligned, 256, 1, 0, false},
    };
    int i = 0;
    for (const Case &c : table) {
        const float *planes[2] = {c.plane, c.other}, *also[2] = {nullptr, c.also}; // (a null entry is aligned)
        GsPlaneSet set{};
        const bool vec = gs_plane_set(set, planes, 2, c.repeat, c.stride, c.pitch, 33, 255, c.also ? also : nullptr);
        expect(vec == c.want, "16-byte verdict of table row", i);
        expect(set.p[0] == c.plane && set.p[1] == c.other && !set.p[2] && !set.p[3] && set.np == 2 && set.stride == c.stride &&
                   set.pitch == c.pitch && set.rows == 33 && set.cols == 255,
               "the set holds the launcher's arguments", i);
        ++i;
    }
    static_assert(sizeof(GsPlaneSet) == 64, "the set is 64 bytes of kernel arguments");
}

} // namespace

int main()
{
    check_set_rule();
    check_groups();
    check_vector_verdict();
    if (failures) return 1;
    std::puts("ok");
    return 0;
}
