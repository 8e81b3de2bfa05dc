// gs_step_flavour.h -- what every translation unit of the step kernels starts with: the arithmetic flavour and the
// vocabulary of the launch tables.
//
// The step kernels are built from five sources into nine objects (grayscott_amd/_build.py), each source once per flavour:
//   gs_step_kernels.hip  the main unit: every kernel but the ones below, and all launchers but the noise unit's two
//   gs_step_op.hip       strict only: the parameter-specialised (".op") marching kernels and the quiet entries
//   gs_step_map.hip      the marching kernel's parameter-map forms (gs_step_tb_mk)
//   gs_step_mask.hip     ... its domain-mask forms (gs_step_tb_wk)
//   gs_step_noise.hip    ... its noise forms (gs_step_tb_zk), and the ensemble kernels' noise forms with their launchers
// GS_MATH_FUSED is the one macro the build sets per unit:
//   GS_MATH_FUSED=0 ("strict"): taps are sub, mul, add; f32 denormal mode = flush results, keep inputs
//       (-fdenormal-fp-math-f32=preserve-sign,ieee -> FP_DENORM 1), which is MXCSR.FTZ without DAZ, i.e. the reference's
//       DenormalsFlusher (compute/shared/src/lib.rs:161-180).
//   GS_MATH_FUSED=1 ("fused"):  taps are sub, fma; denormals kept.  Exact for weights that are 0 or a power of two
//       whenever the product is a normal number.
// Every unit includes this header first, then the kernel headers it instantiates from.
#pragma once
#include "gs_kernels.h"
#include "gs_experiments.h"

#ifndef GS_MATH_FUSED
#error "compile with -DGS_MATH_FUSED=0 or 1"
#endif

#if GS_MATH_FUSED
#define GS_SUFFIX(x) x##_fused
#define GS_TAP(acc, w, s, c) (acc) = __builtin_fmaf((w), (s) - (c), (acc))
#define GS_MATH_NAME "fused"
#else
#define GS_SUFFIX(x) x##_strict
#define GS_TAP(acc, w, s, c) (acc) = (acc) + (w) * ((s) - (c))
#define GS_MATH_NAME "strict"
#endif

// Launch tables.  GS_FN: the entry of a kernel instance (GS_PLAIN_FN: of a kernel that is no template).  kOp: the FAST
// argument of the ".op" variant (the fused build has none: its launchers reduce `fast` to 0).  GS_NAME: the name a launcher
// reports for kernel family BASE, variant V ("", ".op", ...) under the boundary rule of suffix R; GS_RULES: a table of such
// names per kernel set of a rule ("" for the clipped and zero-halo rules, which share their kernels, then "/periodic" and
// "/neumann") from one macro M(BASE, R), indexed by rule_set(); GS_RULES_OF: ... with a suffix A behind the rule's.
#define GS_FN(KER, ...) reinterpret_cast<const void *>(&GS_SUFFIX(KER)<__VA_ARGS__>)
#define GS_PLAIN_FN(KER) reinterpret_cast<const void *>(&GS_SUFFIX(KER))
[[maybe_unused]] constexpr int kOp = GS_MATH_FUSED ? 0 : 3;
#define GS_NAME(BASE, V, R) BASE "/" GS_MATH_NAME V R
#define GS_RULES_OF(M, BASE, A) {M(BASE, A), M(BASE, "/periodic" A), M(BASE, "/neumann" A)}
#define GS_RULES(M, BASE) GS_RULES_OF(M, BASE, "")
#define GS_NAMES_OP(BASE, R) {GS_NAME(BASE, "", R), GS_NAME(BASE, ".op", R)}
// [shape: 32 x 64, 16 x 64, 64 x 64][variant] of the LDS-window kernels, BASE "" or "ensemble-"
#define GS_TILE_NAMES(BASE, R) {GS_NAMES_OP(BASE "tile32x64", R), GS_NAMES_OP(BASE "tile16x64", R), GS_NAMES_OP(BASE "tile64x64", R)}
#define GS_TILE_FNS(KER) {{GS_FN(KER, 2, 0), GS_FN(KER, 2, kOp)}, {GS_FN(KER, 1, 0), GS_FN(KER, 1, kOp)}, {GS_FN(KER, 4, 0), GS_FN(KER, 4, kOp)}}
// The kernel set of boundary rule `boundary` (gs_boundary): 0 = the clipped and zero-halo rules' kernels (*_k), 1 = the
// periodic rule's (*_pk), 2 = the zero-flux rule's (*_nk).
static inline int rule_set(int boundary) { return boundary == 2 ? 1 : (boundary == 3 ? 2 : 0); }

// What the main unit takes from the other units of its flavour.
// gs_tb_map_kernel_*: the entry of the marching kernel's map form (gs_step_tb_mk) for k fused steps, fast in {0, 3} (3: the
// .op variant, strict only), cpl columns per lane and rule = rule_set(boundary); nullptr for a form that is not built.
// gs_tb_mask_kernel_*: the same for the domain mask's forms (gs_step_tb_wk), gs_tb_noise_kernel_*: for the noise forms
// (gs_step_tb_zk).
const void *GS_SUFFIX(gs_tb_map_kernel)(int k, int fast, int cpl, int rule);
const void *GS_SUFFIX(gs_tb_mask_kernel)(int k, int fast, int cpl, int rule);
const void *GS_SUFFIX(gs_tb_noise_kernel)(int k, int fast, int cpl, int rule);
// The ensemble launchers' noise forms (gs_step_noise.hip; GsLaunchers::ens_resident_noise, ens_tile_noise).
hipError_t GS_SUFFIX(gs_launch_ens_resident_noise)(const GsEnsArgs &e, const GsEnsNoiseArgs &z, int steps, int fast, hipStream_t s,
                                                   const char **name);
hipError_t GS_SUFFIX(gs_launch_ens_tile_noise)(const GsEnsArgs &e, const GsEnsNoiseArgs &z, int k, int shape, int fast, hipStream_t s,
                                               const char **name);
