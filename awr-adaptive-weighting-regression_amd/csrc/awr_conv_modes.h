// Process-wide modes and study knobs of the convolution family, shared by its translation units (defined in csrc/awr_conv.hip), and the
// build-time rules of a plan in the form that takes the plan's modes as an argument (the exported functions pass the process-wide ones).
#pragma once
#include <stdlib.h>

#include "../../include/awr_hip.h"

namespace awr {
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
extern int g_force_tm, g_force_tn, g_products, g_wgrad_split, g_staging, g_accum, g_accum_auto_k, g_accum_auto_dgrad, g_train_split_k;
extern int g_knob_deep, g_knob_deep_1x1, g_knob_fast_stats;
inline int wg_products() { return (g_products == 6 && g_wgrad_split) ? 6 : 1; }

// range checks of the per-plan modes (AWR_OK, or AWR_ERR_ARG with the message set): shared by the setters and awr_plan_create_modes
int check_gemm_accum(int mode);
int check_gemm_accum_auto(int min_k);
int check_train_split_k(int on);
int check_conv_winograd(int code);
// awr_resolve_gemm_accum / awr_wino_eligible / awr_wino_wgrad_eligible under the modes `m` / the Winograd code `code`
int resolve_gemm_accum(const awr_plan_modes& m, int k_extent, int kind);
int wino_eligible(int code, int B, int H, int W, int C, int N);
int wino_wgrad_eligible(int code, int B, int H, int W, int C, int N);
}  // namespace awr
