// Host-side helpers shared by the translation units of libumnn_cc.so.
#pragma once
#include <atomic>
#include <cstdio>
#include <cstdlib>

#include "cc_common.h"

int umnn_fail(int code, const char* msg);                 // records msg (thread-local), returns code
int umnn_check(hipError_t e, const char* what);           // 0 or records + returns the hipError_t
// Validates `net`, fills the device-side descriptor (tile / K-step counts, LDS offsets) and reports
// tmax = max tiles over hidden layers and ksu = the common K-step count if all hidden layers agree (else 0).
// max_out: the output width the caller's kernels accept -- 1 (every single-output entry point: widths[n_linear] must be 1), or
// an upper bound above 1 (the multi-output entry points of cc_multi.hip: min_out <= widths[n_linear] <= max_out; min_out = 1: the
// node-value entry, whose K-output kernel serves a single output too).
int umnn_prepare_mlp(const umnn_mlp* net, int E, MlpDev* out, int* tmax, int* ksu, int max_out = 1, int min_out = 2);
int umnn_check_io(const umnn_io* io);                     // 0, or UMNN_EINVAL for an unknown dtype code
int umnn_num_cus();                                      // CU count of the CURRENT device (cached per device)
constexpr size_t UMNN_LDS_LIMIT = 160 * 1024;            // bytes of LDS one workgroup may take (gfx950: 160 KiB per CU)
// Overflow protocol of the fp16-piece launches (cc_fwd_launch.h): mode 1 = the fp16 launch, 2 = the bf16 build queued behind it;
// the flag word and generation number of the pair come from umnn_ovf_slot (cc_api.hip)
struct UmnnOvfPlan { int mode; unsigned long long* flag; unsigned long long gen; };
int umnn_ovf_slot(unsigned long long** flag, unsigned long long* gen);

// Process-wide launch options.  The UMNN_* environment variables are read ONCE (first use, or umnn_reload_env());
// after that every launch reads plain atomics -- no getenv on the launch path.  -1 = "auto" for the tuning knobs.
struct UmnnOptions {
    std::atomic<int> fwd_precision{UMNN_PRECISION_F16X3};    // UMNN_FWD_PRECISION = fp32 | bf16x3 | bf16x6 | f16x3 (default)
    std::atomic<int> bwd_precision{UMNN_PRECISION_BF16X3};   // UMNN_BWD_PRECISION = fp32 | bf16x3
    std::atomic<int> fwd_p{-1};          // UMNN_FWD_P: point tiles per wave (1|2)
    std::atomic<int> fwd_ns{-1};         // UMNN_FWD_NS: node-range split (1|2|4)
    std::atomic<int> fwd_tail{-1};       // UMNN_FWD_TAIL: VALU-tail fp32 variant (0|1)
    std::atomic<int> fwd_pipe{1};        // UMNN_FWD_PIPE: software-pipelined two-tile loop
    std::atomic<int> fwd_pad{1};         // UMNN_FWD_PAD: zero-pad mixed 3..4-tile nets to the shape-exact kernels
    std::atomic<int> fwd_pad_min{1};     // UMNN_FWD_PAD_MIN
    std::atomic<int> bwd_ns{-1};         // UMNN_BWD_NS: node-range split of the backward (1..32)
    // (the rules these three switch -- sizes, thresholds, eligibility -- are written once, in cc_bwd_plan.h: bwd_ws_fills, bwd_ws16_ok, bwd_route)
    std::atomic<int> bwd_ws{1};          // UMNN_BWD_WS: weight-stationary workgroup pipeline (cc_bwd_ws_kernel.h) where the plan finds it eligible
    std::atomic<int> bwd_ws16{1};        // UMNN_BWD_WS16: that pipeline on fp16 pieces (cc_bwd_ws16_kernel.h: three-term recompute): 1 = large launches, 2 = whenever eligible, 0 = never (the bf16 pipeline)
    std::atomic<int> front_bwd2{1};      // UMNN_FRONT_BWD2: stage C of the three-stage backward with two waves per tile of integrals (cc_backward_front.hip; 1: on fp16 pieces behind the fp16 middle stage, 2: bf16 pieces always); 0 = one
    std::atomic<int> bwd_swp{1};         // UMNN_BWD_SWP: software-pipelined one-pass bf16 backward (cc_bwd_swp_kernel.h); 0 = round-2 loop
};
UmnnOptions& umnn_options();
int umnn_allow_lds(const void* fn, size_t bytes);         // hipFuncSetAttribute(MaxDynamicSharedMemorySize)
void umnn_note_launch(const char* kernel_name);
void umnn_note_made_launch(const char* kernel_name);      // conditioner kernels: separate counter / name
long long umnn_param_count(const umnn_mlp* net);
// d_h[b, e d + i] = sum_f W1[f][1 + e] dc[q][f] for every integral q = b d + i: the simple finishing kernel of cc_backward.hip
// (16 or 64 integrals per workgroup), shared with cc_multi.hip.  dh: fp32, or bf16 when h_bf16.  Launches only: no profiling
// bracket, no umnn_note_launch.  Returns 0, or the error of umnn_allow_lds.
int umnn_launch_bwd_dh(const float* dc, const float* W0, float* dh, long long NI, int d, int E, int H1, int h_bf16, hipStream_t stream);

// Optional per-launch timing (umnn_profile_enable): hipEvents recorded on the launch stream around each kernel.
void umnn_prof_begin(hipStream_t stream);
void umnn_prof_end(hipStream_t stream, double flops, int tag = UMNN_PROF_FORWARD);
