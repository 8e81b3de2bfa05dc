// gs_step_noise.hip -- the noise forms, one translation unit per flavour:
//   gs_step_tb_zk<K, FAST, CPL, RULE>  the marching kernel's (gs_march.h: the map forms' set; second argument GsNoiseArgs), with
//       the table of their entries that gs_launch_tb (gs_step_kernels.hip) launches from;
//   gs_ens_resident_z*, gs_ens_tile_z*  the two ensemble kernels' (gs_ensemble.h: second argument GsEnsNoiseArgs,
//       gs_members_set_noise -- a seed, sigmas and a step counter per member, the step key formed on the device), with their
//       launchers.  Nothing else of gs_lds_resident.h and gs_ensemble.h is instantiated here.
#include "gs_step_cell_tables.h"
#include "gs_lds_resident.h"
#include "gs_ensemble.h"
#include "gs_ens_launch.h"

// The noise forms of the ensemble launchers (GsLaunchers::ens_resident_noise, ens_tile_noise): gs_ens_launch.h's bodies over
// the kernels gs_ens_resident_z* / gs_ens_tile_z*.  The name carries "/noise" behind the rule's suffix, and "/listed" behind
// that when z.list is set.
hipError_t GS_SUFFIX(gs_launch_ens_resident_noise)(const GsEnsArgs &e, const GsEnsNoiseArgs &z, int steps, int fast, hipStream_t s,
                                                   const char **name)
{
    static const char *const names[2][3][2] = {GS_RULES_OF(GS_NAMES_OP, "ensemble-resident", "/noise"),
                                               GS_RULES_OF(GS_NAMES_OP, "ensemble-resident", "/noise/listed")};
    // [rule][variant][cells per thread: 1, 2, 4, 8]; the clipped rule has no 8-cell form (gs_ens_resident_cpt)
#define GS_CPT_FNS(KER, ...) {GS_FN(KER, 1, __VA_ARGS__), GS_FN(KER, 2, __VA_ARGS__), GS_FN(KER, 4, __VA_ARGS__), GS_FN(KER, 8, __VA_ARGS__)}
    static const void *const fns[4][2][4] = {
        {{GS_FN(gs_ens_resident_zk, 1, 0, 0), GS_FN(gs_ens_resident_zk, 2, 0, 0), GS_FN(gs_ens_resident_zk, 4, 0, 0), nullptr},
         {GS_FN(gs_ens_resident_zk, 1, kOp, 0), GS_FN(gs_ens_resident_zk, 2, kOp, 0), GS_FN(gs_ens_resident_zk, 4, kOp, 0), nullptr}},
        {GS_CPT_FNS(gs_ens_resident_zk, 0, 1), GS_CPT_FNS(gs_ens_resident_zk, kOp, 1)},
        {GS_CPT_FNS(gs_ens_resident_zpk, 0), GS_CPT_FNS(gs_ens_resident_zpk, kOp)},
        {GS_CPT_FNS(gs_ens_resident_znk, 0), GS_CPT_FNS(gs_ens_resident_znk, kOp)}};
#undef GS_CPT_FNS
    if (!z.table) return hipErrorInvalidValue;
    GsEnsNoiseArgs nz = z;
    return ens_launch_resident(e, names[z.list ? 1 : 0], fns, &nz, steps, fast, s, name);
}
hipError_t GS_SUFFIX(gs_launch_ens_tile_noise)(const GsEnsArgs &e, const GsEnsNoiseArgs &z, int k, int shape, int fast, hipStream_t s,
                                               const char **name)
{
    static const char *const names[2][3][3][2] = {GS_RULES_OF(GS_TILE_NAMES, "ensemble-", "/noise"),
                                                  GS_RULES_OF(GS_TILE_NAMES, "ensemble-", "/noise/listed")};
    static const void *const fns[3][3][2] = {GS_TILE_FNS(gs_ens_tile_zk), GS_TILE_FNS(gs_ens_tile_zpk), GS_TILE_FNS(gs_ens_tile_znk)};
    if (!z.table) return hipErrorInvalidValue;
    GsEnsNoiseArgs nz = z;
    return ens_launch_tile(e, names[z.list ? 1 : 0], fns, &nz, k, shape, fast, s, name);
}

// Kernel entry of the marching kernel's noise form (gs_step_flavour.h: gs_tb_noise_kernel_*), the parameters of
// gs_tb_map_kernel_*.
const void *GS_SUFFIX(gs_tb_noise_kernel)(int k, int fast, int cpl, int rule)
{
    static const void *const general[3][3][4] = GS_CELL_RULES(gs_step_tb_zk, 0);
#if GS_MATH_FUSED
    return tb_cell_entry(general, nullptr, k, fast, cpl, rule);
#else
    static const void *const op[3][3][4] = GS_CELL_RULES(gs_step_tb_zk, 3);
    return tb_cell_entry(general, op, k, fast, cpl, rule);
#endif
}
