// The dispatch decisions of libsr3hip.so: which launch takes which form (conv_plan.hip — host arithmetic only, no kernel
// and no HIP runtime call). ConvPlan / conv_plan / conv_plan_offered / conv_f8_supported are declared in sr3_internal.h;
// here is what the launchers (kernels_conv.hip) and the API (sr3_api.hip) need besides.
#pragma once
#include "sr3_internal.h"

namespace sr3 {

// ---- environment switches (the prose is at the head of sr3_internal.h) ----------------------------------------------
enum Switch {
    SW_NO_GRAPH, SW_NO_HALO, SW_HALO_SPLITS, SW_NO_INPLACE_SPLIT, SW_NO_WINOGRAD, SW_NO_GN_WINO,
    SW_NO_WINO_GEMM_OUT, SW_WINO_GEMM_OUT_FORCE, SW_NO_WINO_FUSED_ROWS, SW_WINO_FUSED_ROWS_FORCE,
    SW_NO_UP2_WINO, SW_UP2_WINO_FORCE, SW_NO_GN_RES1X1, SW_GN_RES1X1_FORCE, SW_NO_CONV_IN_F32,
    SW_COUNT
};
// the variable's value (its default when unset): read from the environment on the FIRST call for this switch, then kept
int env_switch(Switch s);
// ... read now, nothing kept (sr3_create reads SR3_NO_GRAPH once per context)
int env_switch_now(Switch s);
// the SR3_NO_<FORM>=1 / SR3_<FORM>_FORCE=1 pair of a form that a tuned gate guards
enum Form { FORM_WINO_GEMM_OUT, FORM_WINO_FUSED_ROWS, FORM_UP2_WINO, FORM_GN_RES1X1 };
struct FormSwitch { bool off, force; };
FormSwitch form_switch(Form f);
// the first conv of the exact-f32 UNet on its own kernel (run_unet_body's M_CONV_IN, sr3_op_conv_in_f32, sr3_conv_in_f32_gate):
// a form without a tuned gate, so SR3_NO_CONV_IN_F32 has no _FORCE twin
bool conv_in_f32_gate(bool split_arith, int Cin, int Cout, int H, int W);
inline bool gn_wino_off() { return env_switch(SW_NO_GN_WINO) != 0; }

// ---- what launch_conv / launch_wino_gemm share with the plan --------------------------------------------------------
// tile of the generic kernel (and of the x-halo kernel that replaces it where its preconditions hold)
struct Tile { ConvKernel generic; int bm, bn; };
Tile conv_tile_choice(long M, int Cout);
// p as the kernels see it: an upsample conv becomes its four sub-pixel phases over the low-resolution pixels (one
// launch: blockIdx.z picks (py, px)); splits / phase_slices / phase_part_stride are the plan's to fill
ConvParams phase_form(const ConvParams &p_in);
// pixels per block of the split-K reduce (at most 64 statistics slices per image and phase)
int splitk_reduce_tp(int HWo);
// a split conv's fused GroupNorm statistics come out of its reduce pass: slices per image (and per sub-pixel phase)
// for an output of HWo pixels; 0: the reduce pass cannot produce the statistics of this shape
int splitk_stats_slices(int HWo, int Cout);

// ---- the GroupNorm apply pass in front of a conv ---------------------------------------------------------------------
// The form an apply pass takes: decided HERE for the engine (run_gn_act) and for sr3_op_groupnorm_apply's route 0
enum GnRoute { GN_FOLDED = 1, GN_FINALIZE_ROWS = 2 };   // finalize folded into the apply launch | finalize launch + streaming rows
// do the producers' epilogues cover the pass? (else the streaming statistics kernel runs first: launch_groupnorm_partials)
inline bool gn_stats_fused(const TDesc &b, const StatsRef &sa, const StatsRef &sb) { return sa.p && (!b.p || sb.p); }
GnRoute gn_route(const TDesc &a, const TDesc &b, int B, const StatsRef &sa, const StatsRef &sb);

// Does the GroupNorm apply pass in front of a conv write the conv's Winograd input transform (into the Winograd workspace)
// instead of the conv's activated input? Where the conv's plan `pl` is the three-pass form (not its wino_fused_rows form,
// which reads the zero-bordered activated tensor like the one-pass plan), in f32 (split_arith: the context computes in a
// split-f16 arithmetic) with unsplit inputs and no raw side output wanted (raw_wanted also stands for "the pass applies a
// Dropout mask": only launch_gn_apply* know one). The ONE spelling of the rule: the engine (run_res), ScratchConv and
// sr3_gn_res1x1_gate ask here.
bool gn_pass_writes_u(bool split_arith, const ConvPlan &pl, bool raw_wanted, int in_split);

// Does block1's GroupNorm + Swish pass also multiply the block's 1x1 res_conv (launch_gn_res1x1 in place of the apply pass
// and of the side launch of conv2's Winograd plan)? Decided HERE, before block1's pass runs, for the engine (run_res),
// sr3_op_gn_res1x1 and sr3_gn_res1x1_gate.
//   valid: exact f32 and a res_conv whose operands are x / skip themselves, unsplit (`direct`, in_split 0, no raw copy
//          wanted); mode 2; conv1 reads the plain activated tensor (its pass does not write U) and does not run
//          wino_fused_kernel<4> (conv1_fused_rows, its plan's wino_fused_rows: the kernel has not been run behind that
//          form); conv2's plan is a Winograd plan, so that today's 1x1 is a side launch; the kernel's shapes
//          (gn_res1x1_shape_ok).
//   tuned: the levels where every shape of the B = 64 step measured at or under 0.9 of the pair (profiles/README.md,
//          finding 99), from GN_RES1X1_MIN_BLOCKS blocks on (the smallest count timed).
struct GnResGate {
    bool valid = false, tuned = false;
    bool takes() const;     // valid, and tuned or forced, and not switched off
};
GnResGate gn_res1x1_gate(int prec, bool has_res, bool direct, bool raw_wanted, int in_split, int mode, bool conv1_reads_u,
                         int conv1_fused_rows, const ConvPlan &pl2, int B, int H, int W, int C0, int C1, int Cout);
// the gate of a single op (sr3_op_gn_res1x1, sr3_bench_gn_res1x1), which has no convs around it
GnResGate gn_res1x1_gate_op(int prec, int B, int H, int W, int C0, int C1, int Cout);

} // namespace sr3
