// gs_step_op.hip -- the parameter-specialised (".op") instances of the marching kernel gs_step_tb_k, of its forms with
// difference sharing (gs_step_tb_ds_k, gs_step_tb_dx_k) and of their periodic and zero-flux forms, and the quiet entries
// (gs_step_tb_dx_qk): strict flavour only, built apart from the main unit so that the two compile in parallel.  The main unit
// reaches them through gs_tb_op_kernel_strict() and gs_tb_quiet_kernel_strict() (gs_kernels.h).
#include "gs_step_flavour.h"
#if GS_MATH_FUSED
#error "the fused build has no specialised variants"
#endif
#include "gs_cell.h"
#include "gs_march.h"

// Kernel entry of the specialised variant for K fused steps, `fast` in {1, 3} (GsStepArgs::fast)
// and `cpl` columns per lane; RULE: the kernel set of the boundary rule (1 = the periodic rule's form, 2 = the zero-flux
// rule's).
template <int RULE>
static const void *tb_op_kernel(int k, int fast, int cpl, int wg)
{
#define GS_OP_FN(KER, ...) (RULE == 1 ? reinterpret_cast<const void *>(&GS_SUFFIX(KER##_pk)<__VA_ARGS__>) \
                            : RULE == 2 ? reinterpret_cast<const void *>(&GS_SUFFIX(KER##_nk)<__VA_ARGS__>) \
                                        : reinterpret_cast<const void *>(&GS_SUFFIX(KER##_k)<__VA_ARGS__>))
    if (fast == 7) { // full difference sharing: 2 columns per lane
        if (cpl != 2) return nullptr;
        if (wg == 16) return k == 4 ? GS_OP_FN(gs_step_tb_ds, 4, 16) : nullptr;
        switch (k) {
        case 2: return GS_OP_FN(gs_step_tb_ds, 2);
        case 3: return GS_OP_FN(gs_step_tb_ds, 3);
        case 4: return GS_OP_FN(gs_step_tb_ds, 4);
        default: return nullptr;
        }
    }
    if (fast == 15) { // ... and across lanes
        if (cpl != 2) return nullptr;
        if (wg == 16) return k == 4 ? GS_OP_FN(gs_step_tb_dx, 4, 16) : nullptr;
        switch (k) {
        case 2: return GS_OP_FN(gs_step_tb_dx, 2);
        case 3: return GS_OP_FN(gs_step_tb_dx, 3);
        case 4: return GS_OP_FN(gs_step_tb_dx, 4);
        default: return nullptr;
        }
    }
    if (wg == 16) {
        if (k != 4 || (cpl != 1 && cpl != 2) || (fast != 1 && fast != 3)) return nullptr;
        if (fast == 1)
            return cpl == 1 ? GS_OP_FN(gs_step_tb, 4, 1, 1, 16) : GS_OP_FN(gs_step_tb, 4, 1, 2, 16);
        return cpl == 1 ? GS_OP_FN(gs_step_tb, 4, 3, 1, 16) : GS_OP_FN(gs_step_tb, 4, 3, 2, 16);
    }
#define GS_TB_CASE(KK, FF, CC)                                                                  \
    case ((KK) * 4 + (FF)) * 8 + (CC): return GS_OP_FN(gs_step_tb, KK, FF, CC);
#define GS_TB_CASES(FF, CC) GS_TB_CASE(1, FF, CC) GS_TB_CASE(2, FF, CC) GS_TB_CASE(3, FF, CC) GS_TB_CASE(4, FF, CC)
    switch ((k * 4 + fast) * 8 + cpl) {
        GS_TB_CASES(1, 4) GS_TB_CASES(3, 4)
        GS_TB_CASES(1, 2) GS_TB_CASES(3, 2)
        GS_TB_CASES(1, 1) GS_TB_CASES(3, 1)
    default: return nullptr;
    }
#undef GS_TB_CASES
#undef GS_TB_CASE
#undef GS_OP_FN
}
const void *gs_tb_quiet_kernel_strict(int k)
{
    switch (k) {
    case 2: return GS_FN(gs_step_tb_dx_qk, 2);
    case 3: return GS_FN(gs_step_tb_dx_qk, 3);
    case 4: return GS_FN(gs_step_tb_dx_qk, 4);
    default: return nullptr;
    }
}
const void *gs_tb_op_kernel_strict(int k, int fast, int cpl, int wg, int rule)
{
    return rule == 1 ? tb_op_kernel<1>(k, fast, cpl, wg) : (rule == 2 ? tb_op_kernel<2>(k, fast, cpl, wg) : tb_op_kernel<0>(k, fast, cpl, wg));
}

#if defined(GS_TB_TRACE)
extern "C" int32_t gs_debug_trace_read_op(unsigned long long *dst, int32_t units, int32_t clear) { return gs_trace_read(dst, units, clear); }
#endif
