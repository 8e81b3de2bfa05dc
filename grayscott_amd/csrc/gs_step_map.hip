// gs_step_map.hip -- the parameter map's forms of the marching kernel (gs_step_tb_mk<K, FAST, CPL, RULE>, gs_march.h: K = 1..4,
// 1, 2 and 4 columns per lane, every boundary rule's kernel set; the general variant and, strict only, .op), one translation
// unit per flavour, and the table of their entries that gs_launch_tb (gs_step_kernels.hip) launches from.
#include "gs_step_cell_tables.h"

// Kernel entry of the marching kernel's parameter-map form (gs_step_flavour.h: gs_tb_map_kernel_*).
const void *GS_SUFFIX(gs_tb_map_kernel)(int k, int fast, int cpl, int rule)
{
    static const void *const general[3][3][4] = GS_CELL_RULES(gs_step_tb_mk, 0);
#if GS_MATH_FUSED
    return tb_cell_entry(general, nullptr, k, fast, cpl, rule);
#else
    static const void *const op[3][3][4] = GS_CELL_RULES(gs_step_tb_mk, 3);
    return tb_cell_entry(general, op, k, fast, cpl, rule);
#endif
}
