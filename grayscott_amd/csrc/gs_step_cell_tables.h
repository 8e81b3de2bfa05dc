// gs_step_cell_tables.h -- what the map, mask and noise units (gs_step_map.hip, gs_step_mask.hip, gs_step_noise.hip) share:
// the marching kernel and the shape of the entry table each of them hands the main unit (gs_tb_*_kernel_<flavour>).
#pragma once
#include "gs_step_flavour.h"
#include "gs_cell.h"
#include "gs_march.h"

// Entry tables of the marching kernel's per-cell form KER (gs_step_tb_mk, gs_step_tb_wk, gs_step_tb_zk), variant F (0:
// general, 3: .op): [k - 1], [cpl 1, 2, 4][k - 1] and [rule][cpl 1, 2, 4][k - 1]
#define GS_CELL_KS(KER, F, C, R) {GS_FN(KER, 1, F, C, R), GS_FN(KER, 2, F, C, R), GS_FN(KER, 3, F, C, R), GS_FN(KER, 4, F, C, R)}
#define GS_CELL_CPLS(KER, F, R) {GS_CELL_KS(KER, F, 1, R), GS_CELL_KS(KER, F, 2, R), GS_CELL_KS(KER, F, 4, R)}
#define GS_CELL_RULES(KER, F) {GS_CELL_CPLS(KER, F, 0), GS_CELL_CPLS(KER, F, 1), GS_CELL_CPLS(KER, F, 2)}
// ... and the entry for K = 1..4 fused steps, `fast` 0 (general) or 3 (.op: side weights 0.5, dt == 1; `op` is nullptr in the
// fused flavour, which has none), 1, 2 or 4 columns per lane, `rule` the kernel set of the boundary rule (rule_set);
// nullptr for a form that is not built.
static const void *tb_cell_entry(const void *const (*general)[3][4], const void *const (*op)[3][4], int k, int fast, int cpl, int rule)
{
    if (k < 1 || k > 4 || (cpl != 1 && cpl != 2 && cpl != 4) || rule < 0 || rule > 2) return nullptr;
    const void *const(*table)[3][4] = fast == 0 ? general : (fast == 3 ? op : nullptr);
    return table ? table[rule][cpl == 4 ? 2 : cpl - 1][k - 1] : nullptr;
}
