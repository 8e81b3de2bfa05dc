// gs_step_mask.hip -- the domain mask's forms of the marching kernel (gs_step_tb_wk<K, FAST, CPL, RULE>, gs_march.h: the map
// forms' set but for two .op forms, below), one translation unit per flavour, and the table of their entries that
// gs_launch_tb (gs_step_kernels.hip) launches from.
#include "gs_step_cell_tables.h"

// Kernel entry of the marching kernel's domain-mask form (gs_step_flavour.h: gs_tb_mask_kernel_*), the parameters of
// gs_tb_map_kernel_*.  Not built: the .op form of the clipped and zero-halo rules' kernels with 4 columns per lane and 3 or
// 4 fused steps -- the selects of their left and right edge cells on top of the masks' keep a stack frame in scratch;
// gs_launch_tb runs the general form there.
const void *GS_SUFFIX(gs_tb_mask_kernel)(int k, int fast, int cpl, int rule)
{
    static const void *const general[3][3][4] = GS_CELL_RULES(gs_step_tb_wk, 0);
#if GS_MATH_FUSED
    return tb_cell_entry(general, nullptr, k, fast, cpl, rule);
#else
    static const void *const op[3][3][4] = {
        {GS_CELL_KS(gs_step_tb_wk, 3, 1, 0), GS_CELL_KS(gs_step_tb_wk, 3, 2, 0),
         {GS_FN(gs_step_tb_wk, 1, 3, 4, 0), GS_FN(gs_step_tb_wk, 2, 3, 4, 0), nullptr, nullptr}},
        GS_CELL_CPLS(gs_step_tb_wk, 3, 1), GS_CELL_CPLS(gs_step_tb_wk, 3, 2)};
    return tb_cell_entry(general, op, k, fast, cpl, rule);
#endif
}
