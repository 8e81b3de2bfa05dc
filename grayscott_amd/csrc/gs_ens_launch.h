// gs_ens_launch.h -- the one body of each ensemble launcher (gs_ensemble.h's kernels), shared by the unit of the plain and
// listed forms (gs_step_kernels.hip) and the unit of the noise forms (gs_step_noise.hip).  Either hands in its own tables of
// names and entries and the kernel's optional second argument.  Include behind gs_step_flavour.h and gs_lds_resident.h.
//
// `fast` = 3 when EVERY member has side weights 0.5 and dt == 1 (strict only), else 0.  Launches are split so that none
// dispatches more than kGsEnsMaxGroups workgroups.  `second`: nullptr, or what the kernel takes behind GsEnsArgs -- the
// listed forms' pointer to the device list of the active members' indices (the launch then covers entries [e.first,
// e.first + e.members) of it; without one: members [e.first, e.first + e.members) themselves), the noise forms'
// GsEnsNoiseArgs.
#pragma once

// Resident form: `steps` time steps of every member in one launch; the result is stored in the out-planes when steps is
// odd, else back in the in-planes.  names: [rule][variant]; fns: [gs_boundary][variant][cells per thread: 1, 2, 4, 8], nullptr
// where a form is not built.
static hipError_t ens_launch_resident(const GsEnsArgs &e, const char *const (&names)[3][2], const void *const (&fns)[4][2][4], void *second,
                                      int steps, int fast, hipStream_t s, const char **name)
{
    const long cells = (long)e.rows * e.cols;
    if (e.rows <= 0 || e.cols <= 0 || e.members < 0 || steps < 0) return hipErrorInvalidValue;
    const long threads = cells >= 1024 ? 1024 : ((cells + 63) / 64) * 64; // the waves that hold cells
    const int cpt = gs_ens_resident_cpt(e.rows, e.cols, e.zero_halo);
    const size_t lds = (size_t)4 * (e.rows + 2) * (e.cols + 2) * sizeof(float);
    if (!cpt || lds > kGsEnsResidentMaxLds) return hipErrorInvalidValue;
    fast = GS_MATH_FUSED ? 0 : (fast == 3 ? 3 : 0);
    const int zh = e.zero_halo >= 2 && e.zero_halo <= 3 ? e.zero_halo : (e.zero_halo ? 1 : 0); // gs_boundary
    if (name) *name = names[rule_set(zh)][fast ? 1 : 0];
    const void *fn = fns[zh][fast ? 1 : 0][__builtin_ctz(cpt)];
    if (!fn) return hipErrorInvalidValue;
    { // more than 64 KB of dynamic LDS needs the opt-in, per device and device function
        const hipError_t err = gs_ensure_dyn_lds(fn, lds);
        if (err != hipSuccess) return err;
    }
    int to_out = steps & 1;
    for (long m0 = 0; m0 < e.members; m0 += kGsEnsMaxGroups) {
        GsEnsArgs args = e;
        args.first = e.first + m0;
        args.members = (int32_t)(e.members - m0 < kGsEnsMaxGroups ? e.members - m0 : kGsEnsMaxGroups);
        void *kargs[] = {&args, &steps, &to_out}, *sargs[] = {&args, second, &steps, &to_out};
        const hipError_t err = hipLaunchKernel(fn, dim3((unsigned)args.members), dim3((unsigned)threads), second ? sargs : kargs, lds, s);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

// Windowed form: K <= kGsTileMaxSteps steps of every member (in-planes -> out-planes); `shape` as gs_launch_tile's.
// names, fns: [rule][shape][variant].
static hipError_t ens_launch_tile(const GsEnsArgs &e, const char *const (&names)[3][3][2], const void *const (&fns)[3][3][2], void *second,
                                  int k, int shape, int fast, hipStream_t s, const char **name)
{
    static const int rpw[3] = {2, 1, 4};
    const int per = rule_set(e.zero_halo); // the periodic and zero-flux rules: gs_ens_tile_pk / _nk
    if (e.rows <= 0 || e.cols <= 0 || e.members < 0 || k < 1 || k > kTileMaxK || shape < 0 || shape > 2 || 2 * k >= tile_rows(rpw[shape]))
        return hipErrorInvalidValue;
    fast = GS_MATH_FUSED ? 0 : (fast == 3 ? 3 : 0);
    if (name) *name = names[per][shape][fast ? 1 : 0];
    const long ho = tile_rows(rpw[shape]) - 2 * k, wo = kTileCols - 2 * k;
    const long windows = ((e.rows + ho - 1) / ho) * ((e.cols + wo - 1) / wo);
    if (windows > kGsEnsMaxGroups) return hipErrorInvalidConfiguration;
    const void *fn = fns[per][shape][fast ? 1 : 0];
    const size_t lds = tile_lds_bytes(rpw[shape]);
    {
        const hipError_t err = gs_ensure_dyn_lds(fn, lds);
        if (err != hipSuccess) return err;
    }
    const long per_launch = kGsEnsMaxGroups / windows; // members per launch
    int wins = (int)windows;
    for (long m0 = 0; m0 < e.members; m0 += per_launch) {
        GsEnsArgs args = e;
        args.first = e.first + m0;
        args.members = (int32_t)(e.members - m0 < per_launch ? e.members - m0 : per_launch);
        void *kargs[] = {&args, &k, &wins}, *sargs[] = {&args, second, &k, &wins};
        const hipError_t err = hipLaunchKernel(fn, dim3((unsigned)(args.members * windows)), dim3(kTileWaves * 64), second ? sargs : kargs, lds, s);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}
