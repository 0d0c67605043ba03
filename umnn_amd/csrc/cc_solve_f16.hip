// The Newton solve on fp16 PIECES: cc_solve.hip (variant tables + launcher) and cc_fwd_bf16_kernel.h (the kernels) compiled with the
// 16-bit piece type switched to fp16.  Exports umnn_solve_impl_f16, which umnn_cc_solve (the bf16 build of that file) calls under
// fwd_precision = f16x3, the library default; every launch is followed by its queued bf16x3 fallback (file header there).
#define UMNN_FWD_PIECE_F16 1
#include "cc_solve.hip"
