// Launch plan of the forward quadrature, the bracket search and the Newton solve, decided once: which kernel family a call runs, on
// which build (fp16 or bf16 pieces), with which variant, weight-image layout, P, node-range split, grid and LDS bytes, and whether the
// bf16 build is queued behind it.  Written for the launchers (cc_forward.hip, cc_forward_bf16.hip and its fp16 build,
// cc_forward_p32.hip, cc_inv_launch.h for cc_invert.hip / cc_solve.hip) and for the read-only query umnn_cc_launch_plan.  Plain host
// arithmetic: no HIP call, no global state, no umnn_options() read -- the caller passes a snapshot of the forward options and the CU
// count.  A launcher executes a plan (cc_fwd_launch.h) and never falls through to another family: a shape a family cannot run is a
// predicate here.  The variant lists below are the single source of the kernel names AND of the order of every translation unit's
// table of instantiations, so a plan names its kernel by an index.
#pragma once
#include "cc_host.h"

struct FwdOptions { int fwd_precision, fwd_p, fwd_ns, fwd_tail, fwd_pipe, fwd_pad, fwd_pad_min; };
enum FwdJob { FWD_JOB_FORWARD = 0, FWD_JOB_SEARCH = 1, FWD_JOB_SOLVE = 2 };      // = the INV argument of cc_fwd_bf16_kernel
enum FwdFamily {
    FWD_FAMILY_PIECES = 1,    // cc_fwd_bf16_kernel on two or three 16-bit pieces: shape-exact or generic (runtime tile counts)
    FWD_FAMILY_WIDE_FIRST,    // ... its variants for a wide first hidden layer over a narrow rest
    FWD_FAMILY_P32,           // the 32x32x16 formulation of the flagship shape (cc_forward_p32.hip; opt-in, fwd_pipe = 2)
    FWD_FAMILY_FP32,          // fp32 MFMA (cc_forward.hip)
};
struct FwdCall {
    int job;                  // FwdJob
    long long NI;             // forward: integrals
    long long groups;         // search / solve: tiles in the launch
    int n;                    // nb_steps
    int scratch;              // search / solve: floats of reduction scratch per wave when a tile's node range is split
    bool alias;               // forward: the marker output (F, or z) aliases an input
    bool z2;                  // forward: z_2 is to be saved
};
inline FwdCall fwd_call_forward(long long NI, int n, bool alias, bool z2) { return FwdCall{FWD_JOB_FORWARD, NI, 0, n, 0, alias, z2}; }
// bracket search: one tile = one sample (scratch: the candidates' partial sums); Newton solve: one tile = sixteen rows (scratch:
// the partial sums and f(x) of a split tile)
inline FwdCall fwd_call_search(long long B, int n) { return FwdCall{FWD_JOB_SEARCH, B, B, n, 16, false, false}; }
inline FwdCall fwd_call_solve(long long rows, int n) { return FwdCall{FWD_JOB_SOLVE, rows, (rows + 15) / 16, n, 2 * 16, false, false}; }

// ------------------------------------------------------------------------------------------ variants and their names
// Piece kernels: X(T, NPARTS, P, EXACT, LIVE, PIPE, TREST, WPB, ...) = cc_fwd_bf16_kernel<T, NPARTS, P, EXACT, LIVE, PIPE, INV, TREST, WPB>.
// LIVE: live registers per lane when every layer agrees (13 = widths 48..51, 26 = 96..103), 0 = all.  WPB = 8: one workgroup per CU.
#define UMNN_FWD_ROWS_2(X, ...) \
    X(4, 2, 2, 1, 13, 1, 0, 4, __VA_ARGS__) X(4, 2, 2, 1, 0, 1, 0, 4, __VA_ARGS__)      /* software-pipelined node loop (ahead of the plain rows: picked when wanted) */ \
    X(4, 2, 1, 1, 13, 0, 0, 4, __VA_ARGS__) X(4, 2, 2, 1, 13, 0, 0, 4, __VA_ARGS__)     /* widths 48..51 */ \
    X(4, 2, 1, 1, 0, 0, 0, 4, __VA_ARGS__) X(4, 2, 2, 1, 0, 0, 0, 4, __VA_ARGS__)       /* widths 52..62, and zero-padded nets */ \
    X(2, 2, 1, 0, 0, 0, 0, 4, __VA_ARGS__) X(2, 2, 2, 0, 0, 0, 0, 4, __VA_ARGS__) \
    X(4, 2, 1, 0, 0, 0, 0, 4, __VA_ARGS__) X(4, 2, 2, 0, 0, 0, 0, 4, __VA_ARGS__) \
    X(7, 2, 1, 1, 26, 0, 0, 4, __VA_ARGS__) X(7, 2, 1, 1, 0, 0, 0, 4, __VA_ARGS__)      /* widths 96..111 (100-wide toy / MonotonicNN nets): 3 K-steps + a half one */ \
    X(5, 2, 1, 1, 0, 0, 0, 4, __VA_ARGS__) X(6, 2, 1, 1, 0, 0, 0, 4, __VA_ARGS__) X(8, 2, 1, 1, 0, 0, 0, 4, __VA_ARGS__)   /* widths 64..79, 80..95, 112..127 */ \
    X(7, 2, 1, 1, 26, 0, 0, 8, __VA_ARGS__) X(7, 2, 1, 1, 0, 0, 0, 8, __VA_ARGS__) X(5, 2, 1, 1, 0, 0, 0, 8, __VA_ARGS__) \
    X(6, 2, 1, 1, 0, 0, 0, 8, __VA_ARGS__) X(8, 2, 1, 1, 0, 0, 0, 8, __VA_ARGS__) \
    X(8, 2, 1, 0, 0, 0, 0, 4, __VA_ARGS__) X(8, 2, 2, 0, 0, 0, 0, 4, __VA_ARGS__)       /* (8 tiles x 3 parts does not fit the register file: fp32 kernels instead) */
// (two point tiles per wave, P = 2, in the wide-first family: 260 registers = one wave per SIMD, 0.63 ms against 0.49 ms at the MNIST shape -- not instantiated)
#define UMNN_FWD_ROWS_WIDE_FIRST(X, ...) \
    X(5, 2, 1, 1, 13, 0, 4, 4, __VA_ARGS__) X(6, 2, 1, 1, 13, 0, 4, 4, __VA_ARGS__) X(7, 2, 1, 1, 13, 0, 4, 4, __VA_ARGS__) X(8, 2, 1, 1, 13, 0, 4, 4, __VA_ARGS__) \
    X(5, 2, 1, 1, 0, 0, 4, 4, __VA_ARGS__) X(6, 2, 1, 1, 0, 0, 4, 4, __VA_ARGS__) X(7, 2, 1, 1, 0, 0, 4, 4, __VA_ARGS__) X(8, 2, 1, 1, 0, 0, 4, 4, __VA_ARGS__)
// three pieces / six cross terms (bf16x6): bf16 build only -- pointless on fp16 pieces, whose two already carry 22 bits
#define UMNN_FWD_ROWS_3(X, ...) \
    X(4, 3, 1, 1, 13, 0, 0, 4, __VA_ARGS__) X(4, 3, 2, 1, 13, 0, 0, 4, __VA_ARGS__) X(4, 3, 1, 1, 0, 0, 0, 4, __VA_ARGS__) X(4, 3, 2, 1, 0, 0, 0, 4, __VA_ARGS__) \
    X(2, 3, 1, 0, 0, 0, 0, 4, __VA_ARGS__) X(2, 3, 2, 0, 0, 0, 0, 4, __VA_ARGS__) X(4, 3, 1, 0, 0, 0, 0, 4, __VA_ARGS__) X(4, 3, 2, 0, 0, 0, 0, 4, __VA_ARGS__)
// search and solve (INV = 1 | 2): one tile per wave
#define UMNN_INV_ROWS_2(X, ...) \
    X(4, 2, 1, 1, 13, 0, 0, 4, __VA_ARGS__) X(4, 2, 1, 1, 0, 0, 0, 4, __VA_ARGS__)      /* UCI / VAE nets (31-50^4-1) and every other 3..4-tile net (zero-padded) */ \
    X(7, 2, 1, 1, 26, 0, 0, 4, __VA_ARGS__) X(7, 2, 1, 1, 0, 0, 0, 4, __VA_ARGS__)      /* 100-wide toy nets */ \
    X(5, 2, 1, 1, 0, 0, 0, 4, __VA_ARGS__) X(6, 2, 1, 1, 0, 0, 0, 4, __VA_ARGS__) X(8, 2, 1, 1, 0, 0, 0, 4, __VA_ARGS__) \
    X(7, 2, 1, 1, 26, 0, 0, 8, __VA_ARGS__) X(7, 2, 1, 1, 0, 0, 0, 8, __VA_ARGS__) X(5, 2, 1, 1, 0, 0, 0, 8, __VA_ARGS__) \
    X(6, 2, 1, 1, 0, 0, 0, 8, __VA_ARGS__) X(8, 2, 1, 1, 0, 0, 0, 8, __VA_ARGS__) \
    X(2, 2, 1, 0, 0, 0, 0, 4, __VA_ARGS__) X(4, 2, 1, 0, 0, 0, 0, 4, __VA_ARGS__) X(8, 2, 1, 0, 0, 0, 0, 4, __VA_ARGS__)   /* generic: e.g. 20-20, mixed wide 70-90 */
// wide first hidden layer over a narrow rest (MNISTExperiment's integrand: sampling d = 784 images is 3 920 search launches)
#define UMNN_INV_ROWS_WIDE_FIRST(X, ...) UMNN_FWD_ROWS_WIDE_FIRST(X, __VA_ARGS__)
// three pieces (fwd_precision = fp32 | bf16x6; bf16 build only): nets of up to four tiles per layer
#define UMNN_INV_ROWS_3(X, ...) \
    X(4, 3, 1, 1, 13, 0, 0, 4, __VA_ARGS__) X(4, 3, 1, 1, 0, 0, 0, 4, __VA_ARGS__) X(2, 3, 1, 0, 0, 0, 0, 4, __VA_ARGS__) X(4, 3, 1, 0, 0, 0, 0, 4, __VA_ARGS__)

struct FwdRow { int T, np, p, ex, nr, pipe, trest, wpb; const char* name; };
#define UMNN_FWD_SFX_0_4 ""
#define UMNN_FWD_SFX_1_4 ",PIPE"
#define UMNN_FWD_SFX_0_8 ",WAVES=8"
#define UMNN_FWD_KEY(T, NP, P, EX, NR, PIPE, TREST, WPB) T, NP, P, EX, NR, PIPE, TREST, WPB
#define UMNN_FWD_NAME(T, NP, P, EX, NR, PIPE, TREST, WPB, STEM) \
    { UMNN_FWD_KEY(T, NP, P, EX, NR, PIPE, TREST, WPB), STEM "<T=" #T ",PARTS=" #NP ",P=" #P ",EXACT=" #EX ",LIVE=" #NR UMNN_FWD_SFX_##PIPE##_##WPB ">" },
#define UMNN_FWD_NAME_WIDE_FIRST(T, NP, P, EX, NR, PIPE, TREST, WPB, STEM) \
    { UMNN_FWD_KEY(T, NP, P, EX, NR, PIPE, TREST, WPB), STEM "<T1=" #T ",TREST=" #TREST ",PARTS=" #NP ",P=" #P ",EXACT=" #EX ",LIVE=" #NR ">" },
#define UMNN_INV_NAME(T, NP, P, EX, NR, PIPE, TREST, WPB, STEM) \
    { UMNN_FWD_KEY(T, NP, P, EX, NR, PIPE, TREST, WPB), STEM "<T=" #T ",EXACT=" #EX ",LIVE=" #NR UMNN_FWD_SFX_##PIPE##_##WPB ">" },
#define UMNN_INV_NAME_WIDE_FIRST(T, NP, P, EX, NR, PIPE, TREST, WPB, STEM) \
    { UMNN_FWD_KEY(T, NP, P, EX, NR, PIPE, TREST, WPB), STEM "<T1=" #T ",TREST=" #TREST ",LIVE=" #NR ">" },
#define UMNN_INV_NAME_3(T, NP, P, EX, NR, PIPE, TREST, WPB, STEM) \
    { UMNN_FWD_KEY(T, NP, P, EX, NR, PIPE, TREST, WPB), STEM "<T=" #T ",PARTS=" #NP ",EXACT=" #EX ",LIVE=" #NR ">" },
// One table per job and build.  The two-piece rows come first and are the same lists in both builds, so an index into the fp16
// table names the same variant in the bf16 table: that is what lets a queued fallback take the plan of the launch it follows.
#define UMNN_FWD_TABLE(STEM) UMNN_FWD_ROWS_2(UMNN_FWD_NAME, STEM) UMNN_FWD_ROWS_WIDE_FIRST(UMNN_FWD_NAME_WIDE_FIRST, STEM)
#define UMNN_INV_TABLE(STEM) UMNN_INV_ROWS_2(UMNN_INV_NAME, STEM) UMNN_INV_ROWS_WIDE_FIRST(UMNN_INV_NAME_WIDE_FIRST, STEM)
constexpr FwdRow kFwdRowsF16[] = { UMNN_FWD_TABLE("cc_fwd_f16") };
constexpr FwdRow kFwdRowsBf16[] = { UMNN_FWD_TABLE("cc_fwd_bf16") UMNN_FWD_ROWS_3(UMNN_FWD_NAME, "cc_fwd_bf16") };
constexpr FwdRow kInvertRowsF16[] = { UMNN_INV_TABLE("cc_invert_f16") };
constexpr FwdRow kInvertRowsBf16[] = { UMNN_INV_TABLE("cc_invert_bf16") UMNN_INV_ROWS_3(UMNN_INV_NAME_3, "cc_invert_bf16") };
constexpr FwdRow kSolveRowsF16[] = { UMNN_INV_TABLE("cc_solve_f16") };
constexpr FwdRow kSolveRowsBf16[] = { UMNN_INV_TABLE("cc_solve_bf16") UMNN_INV_ROWS_3(UMNN_INV_NAME_3, "cc_solve_bf16") };
template <int N> constexpr int fwd_count(const FwdRow (&)[N]) { return N; }
// every key of the fp16 table sits at the same index of the bf16 table
template <int NA, int NB>
constexpr bool fwd_rows_prefix(const FwdRow (&a)[NA], const FwdRow (&b)[NB]) {
    if (NA > NB) return false;
    for (int i = 0; i < NA; ++i)
        if (a[i].T != b[i].T || a[i].np != b[i].np || a[i].p != b[i].p || a[i].ex != b[i].ex || a[i].nr != b[i].nr ||
            a[i].pipe != b[i].pipe || a[i].trest != b[i].trest || a[i].wpb != b[i].wpb || a[i].np != 2) return false;
    return true;
}
static_assert(fwd_rows_prefix(kFwdRowsF16, kFwdRowsBf16) && fwd_rows_prefix(kInvertRowsF16, kInvertRowsBf16) &&
              fwd_rows_prefix(kSolveRowsF16, kSolveRowsBf16), "the bf16 build holds every variant of the fp16 build, at the same index");
inline const FwdRow* fwd_rows(int job, bool f16, int* count) {
    if (job == FWD_JOB_FORWARD) { *count = f16 ? fwd_count(kFwdRowsF16) : fwd_count(kFwdRowsBf16); return f16 ? kFwdRowsF16 : kFwdRowsBf16; }
    if (job == FWD_JOB_SEARCH) { *count = f16 ? fwd_count(kInvertRowsF16) : fwd_count(kInvertRowsBf16); return f16 ? kInvertRowsF16 : kInvertRowsBf16; }
    *count = f16 ? fwd_count(kSolveRowsF16) : fwd_count(kSolveRowsBf16);
    return f16 ? kSolveRowsF16 : kSolveRowsBf16;
}

// the fp32-MFMA variants: X(T, KS, P, TAIL, NT) = cc_fwd_kernel<T, KS, P, TAIL, NT> (cc_forward.hip instantiates them in this order)
#define UMNN_FWD_FP32_VARIANTS(X) \
    X(4, 13, 1, 1, 2) X(4, 13, 2, 1, 2)      /* hidden width 50 (UCI / VAE nets): VALU tail for 48,49 */ \
    X(4, 13, 1, 0, 0) X(4, 13, 2, 0, 0)      /* widths 48..51, all four tiles on MFMA */ \
    X(7, 26, 1, 0, 0) X(7, 26, 2, 0, 0)      /* hidden width 100 (toy / MonotonicMLP nets) */ \
    X(2, 0, 1, 0, 0) X(2, 0, 2, 0, 0)        /* generic, hidden widths <= 31 */ \
    X(4, 0, 1, 0, 0) X(4, 0, 2, 0, 0)        /* generic, <= 63 */ \
    X(8, 0, 1, 0, 0) X(8, 0, 2, 0, 0)        /* generic, <= 127 */
struct FwdFp32Row { int tmax, ksc, p, tail, nt; const char* name; };
#define UMNN_FWD_FP32_ROW(T, K, PP, TL, NT) { T, K, PP, TL, NT, "cc_fwd<T=" #T ",KS=" #K ",P=" #PP ",TAIL=" #TL ">" },
constexpr FwdFp32Row kFwdFp32Rows[] = { UMNN_FWD_FP32_VARIANTS(UMNN_FWD_FP32_ROW) };
constexpr int kFwdFp32Count = (int)(sizeof(kFwdFp32Rows) / sizeof(kFwdFp32Rows[0]));
constexpr const char* kFwdP32Name = "cc_fwd_bf16<32x32x16,PARTS=2,P=2,EXACT=1,LIVE=26,PIPE32>";

// ------------------------------------------------------------------------------------------ weight-image layouts
// Piece kernels: image l (hidden layer l -> l + 1) holds t_out[l + 1] output tiles x (ks32[l] K-steps of 32 features + half_in[l] half
// step) x nparts pieces of 512 (256) 16-bit words at ushort offset off16[l]; lds_off[L] is where the images end (floats, a multiple
// of four): the NS-reduction scratch starts there.  (The first three arrays of Bf16Plan, cc_fwd_bf16_kernel.h.)
struct FwdImages { int ks32[UMNN_MAX_LINEAR], off16[UMNN_MAX_LINEAR], half_in[UMNN_MAX_LINEAR]; };
// T: tile count of the variant; exact: every hidden layer has exactly T tiles; nrl: live registers per lane (K-steps of four
// features) when every layer agrees, else 0 -- of layers 2..L, and only 13, in the wide-first family; wide: see fwd_uniform_wide
struct FwdLayout { int T, exact, nrl, wide; };

inline int fwd_tile_bucket(int tmax) { return tmax <= 2 ? 2 : tmax <= 4 ? 4 : 8; }

// every hidden layer the same tile count above four (exact single-tile variants, odd counts with a half K-step): that count, else 0
inline int fwd_uniform_wide(const MlpDev& m, int tmax) {
    int wide = tmax >= 5 ? tmax : 0;
    for (int l = 1; l < m.n_linear && wide; ++l) if (m.t_out[l] != wide) wide = 0;
    return wide;
}

inline void fwd_close_images(MlpDev& m, int off16) { m.lds_off[m.n_linear - 1] = (((off16 + 1) / 2) + 3) & ~3; }

// Wide first hidden layer (T1 = 5..8 tiles) over a rest of at most four tiles each (MNISTExperiment's 31-100-50-50-50-50-1)
inline bool fwd_wide_first_shape(const MlpDev& m) {
    const int L = m.n_linear - 1, T1 = m.t_out[1];
    if (L < 2 || T1 < 5 || T1 > 8) return false;
    for (int l = 2; l <= L; ++l) if (m.t_out[l] > 4) return false;
    return true;
}
// ... its images: the rest zero-padded to four tiles; layer 1's GEMM contracts over T1 tiles, the others over four.  False (nothing
// touched) for any other shape.
inline bool fwd_images_wide_first(MlpDev& m, FwdImages& im, int nparts, FwdLayout* lay) {
    if (!fwd_wide_first_shape(m)) return false;
    const int L = m.n_linear - 1, T1 = m.t_out[1];
    int off16 = 0;
    for (int l = 1; l <= L; ++l) {
        im.ks32[l] = l == 1 ? T1 / 2 : 2;
        im.half_in[l] = l == 1 ? (T1 & 1) : 0;
        if (l >= 2) m.t_out[l] = 4;
    }
    for (int l = 1; l < L; ++l) {
        im.off16[l] = off16;
        off16 += 4 * (im.ks32[l] * nparts * 512 + im.half_in[l] * nparts * 256);
    }
    fwd_close_images(m, off16);
    int nrest = m.ks_in[2];           // live registers of the later layers when they all agree (13 = widths 48..51)
    for (int l = 2; l <= L; ++l) if (m.ks_in[l] != nrest) nrest = 0;
    *lay = FwdLayout{T1, 1, nrest == 13 ? 13 : 0, 0};
    return true;
}

// Every other net.  wide (fwd_uniform_wide, or 0 where the job has no such variant): images of wide / 2 K-steps and a half one.
// Otherwise one K-step per pair of tiles of the layer as it is (the generic variants read the counts at run time) -- unless pad:
// mixed or narrow nets of pad_min..4 tiles are zero-padded to four tiles per layer (the staged images carry the zeros) and run the
// shape-exact kernels: the padded MFMAs cost less than the runtime guards of the generic variants.
inline FwdLayout fwd_images(MlpDev& m, FwdImages& im, int nparts, int tmax, int wide, bool pad, int pad_min) {
    const int L = m.n_linear - 1;
    FwdLayout lay{wide ? wide : fwd_tile_bucket(tmax), 1, m.ks_in[1], wide};
    int off16 = 0;
    for (int l = 1; l <= L; ++l) {
        im.half_in[l] = wide ? (wide & 1) : 0;
        im.ks32[l] = wide ? wide / 2 : (m.t_out[l] + 1) / 2;
    }
    for (int l = 1; l < L; ++l) {
        im.off16[l] = off16;
        off16 += m.t_out[l + 1] * (im.ks32[l] * nparts * 512 + im.half_in[l] * nparts * 256);
    }
    for (int l = 1; l <= L; ++l) {
        lay.exact = lay.exact && m.t_out[l] == lay.T;
        if (m.ks_in[l] != lay.nrl) lay.nrl = 0;
    }
    if (pad && !lay.exact && !wide && tmax <= 4 && tmax >= pad_min) {
        lay.T = 4; lay.exact = 1; lay.nrl = 0;
        for (int l = 1; l <= L; ++l) { m.t_out[l] = 4; im.ks32[l] = 2; }
        off16 = 0;
        for (int l = 1; l < L; ++l) { im.off16[l] = off16; off16 += 4 * 2 * nparts * 512; }
    }
    fwd_close_images(m, off16);
    return lay;
}

// The 32x32x16 kernel: 2..5 hidden layers, every one 48..51 wide; per layer 14 fragments of 512 ushorts (cc_forward_p32.hip)
constexpr int FWD_P32_IMAGE_USHORTS = 14 * 512;
inline bool fwd_p32_shape(const MlpDev& m) {
    const int L = m.n_linear - 1;
    if (L < 2 || L > 5) return false;
    for (int l = 1; l <= L; ++l) if (m.ks_in[l] != 13) return false;
    return true;
}
inline void fwd_images_p32(MlpDev& m) {
    const int L = m.n_linear - 1;
    const size_t img_bytes = (size_t)(L - 1) * FWD_P32_IMAGE_USHORTS * sizeof(unsigned short);
    m.lds_off[L] = (int)((img_bytes / 4 + 3) & ~(size_t)3);
}

// fp32-MFMA TAIL variants: T - 1 tiles per image on MFMA, then the rows of the last tile's n_tail real features for the VALU
inline void fwd_images_fp32_tail(MlpDev& m, int tmax) {
    const int L = m.n_linear - 1;
    int off = 0;
    for (int l = 1; l <= L; ++l) m.t_mfma[l] = m.t_out[l] - 1;
    for (int l = 1; l < L; ++l) { m.lds_off[l] = off; off += m.t_mfma[l + 1] * m.ks_in[l] * 64; }
    m.tail_off = off;
    m.n_tail = m.width[1] - 16 * (tmax - 1);
    off += (L - 1) * 3 * 4 * 16;
    m.lds_off[L] = off;
}

// ------------------------------------------------------------------------------------------ the rules, once each
// node-range split of the forward: four waves per tile up to lim4 tiles, two up to lim2, never more parts than nodes
inline int fwd_split(long long tiles16, long long lim4, long long lim2, int n) {
    const int ns = tiles16 <= lim4 ? 4 : tiles16 <= lim2 ? 2 : 1;
    return ns > n + 1 ? 1 : ns;
}
// Search and solve, small batches: one tile per WORKGROUP, its node range split over all the workgroup's waves (partials meet in LDS
// once per round or iteration, in a fixed order) -- B waves of a 100-image sampling call leave nine SIMDs in ten idle, and every wave
// walks its (n + 1) nodes alone.  Taken while all groups x wpb waves are resident at once (two per SIMD).
inline int fwd_split_over(long long groups, int wpb, int n, int cus) { return (groups * (long long)wpb <= (long long)cus * 8 && wpb <= n + 1) ? wpb : 1; }
// Uniform wide nets: how many workgroups of images fit a CU?  One -> eight waves per workgroup (both waves of every SIMD share the
// images); two -> four waves each.  Either way a CU runs eight waves.
inline int fwd_waves(const FwdLayout& lay, int nparts, size_t image_bytes) {
    return lay.wide && lay.exact && nparts == 2 && 2 * (image_bytes + 1024) > UMNN_LDS_LIMIT ? 8 : UMNN_WAVES_PER_BLOCK;
}
// The variant of a layout: the exact one for (T, live registers) if instantiated, else the exact one with all registers live, else
// the generic one of the tile-count bucket (runtime counts; wherever that is reached the bucket is the layout's own T).  -1: none
inline int fwd_pick(const FwdRow* rows, int count, const FwdLayout& lay, int tmax, int nparts, int P, bool want_pipe, int wpb) {
    for (int ex = lay.exact; ex >= 0; --ex)
        for (int pass = 0; pass < 2; ++pass)      // pass 0: a variant with exactly this live-register count
            for (int i = 0; i < count; ++i) {
                const FwdRow& v = rows[i];
                if (!v.trest && v.T == (ex ? lay.T : fwd_tile_bucket(tmax)) && v.np == nparts && v.p == P && v.ex == ex &&
                    (!v.pipe || want_pipe) && v.wpb == (ex ? wpb : UMNN_WAVES_PER_BLOCK) &&
                    (pass == 0 ? (ex && lay.nrl && v.nr == lay.nrl) : v.nr == 0)) return i;
            }
    return -1;
}
inline int fwd_pick_wide_first(const FwdRow* rows, int count, const FwdLayout& lay) {
    for (int i = 0; i < count; ++i)
        if (rows[i].trest && rows[i].T == lay.T && rows[i].nr == lay.nrl) return i;
    return -1;
}

// ------------------------------------------------------------------------------------------ the plan
struct FwdPlan {
    int error;                // 0, or the code the entry point returns (launching nothing) ...
    const char* error_text;   // ... with this text
    int family;               // FwdFamily
    int f16, nparts;          // build (1: fp16 pieces) and piece count (0: fp32 MFMA)
    int variant;              // index into the table of (job, build): fwd_rows / kFwdFp32Rows; P32: hidden layers - 2
    const char* name;
    MlpDev m;                 // the net with the layout edits of the family
    FwdImages img;
    int P, ns, wpb;
    unsigned ngroups, blocks;
    int block;                // threads per workgroup
    size_t lds_bytes;
    int fallback;             // the bf16 build of the same variant is queued behind the launch (fp16 pieces: overflow protocol)
};
constexpr const char* kFwdPlanError = "forward: internal error, a launcher was handed a plan it cannot run";

inline void fwd_plan_fail(FwdPlan& pl, const char* text) { pl.error = UMNN_EUNSUPPORTED; pl.error_text = text; }
inline void fwd_plan_grid(FwdPlan& pl, int family, const char* name, int variant, int P, int ns, int wpb, long long groups, size_t lds_bytes) {
    pl.family = family; pl.name = name; pl.variant = variant;
    pl.P = P; pl.ns = ns; pl.wpb = wpb;
    pl.ngroups = (unsigned)groups;
    const unsigned gpb = wpb / ns;                 // tile groups per workgroup
    pl.blocks = (pl.ngroups + gpb - 1) / gpb;
    pl.block = 64 * wpb;
    pl.lds_bytes = lds_bytes;
}

// The piece families of the forward on one build and piece count; false: this build has no kernel for the call (pl untouched).
// P, ns: what the batch-size rule of fwd_plan gave.
inline bool fwd_plan_pieces(FwdPlan& out, const MlpDev& m0, int tmax, const FwdCall& c, const FwdOptions& o, int cus, bool f16, int nparts, int P, int ns) {
    const int L = m0.n_linear - 1;
    const bool p_set = o.fwd_p > 0, ns_set = o.fwd_ns > 0;      // (the options: they override the rules below)
    const long long tiles16 = (c.NI + 15) / 16;
    int count = 0;
    const FwdRow* rows = fwd_rows(FWD_JOB_FORWARD, f16, &count);
    FwdPlan pl = out;
    pl.f16 = f16; pl.nparts = nparts; pl.fallback = f16;
    // uniform wide nets: two-piece single-tile variants only (no two-tile variant at these widths); the node range is split only as
    // far as that fills the SIMDs (two waves each)
    int wide = nparts == 2 ? fwd_uniform_wide(m0, tmax) : 0;
    if (wide && (P == 1 || !p_set)) P = 1; else wide = 0;
    if (wide && !ns_set) ns = fwd_split(tiles16, 2LL * cus, 4LL * cus, c.n);
    // ---- wide first hidden layer over a narrow rest: its own shape-exact family, the only one that knows how to leave z_2 behind
    FwdLayout lay;
    if (nparts == 2 && (P == 1 || !p_set) && fwd_images_wide_first(pl.m, pl.img, nparts, &lay)) {
        if (!ns_set) ns = fwd_split(tiles16, 2LL * cus, 4LL * cus, c.n);
        const size_t lds_bytes = ((size_t)pl.m.lds_off[L] + (ns > 1 ? UMNN_WAVES_PER_BLOCK * 3 * 16 : 0)) * sizeof(float);
        const int v = fwd_pick_wide_first(rows, count, lay);
        if (v >= 0 && lds_bytes <= UMNN_LDS_LIMIT) {
            fwd_plan_grid(pl, FWD_FAMILY_WIDE_FIRST, rows[v].name, v, 1, ns, UMNN_WAVES_PER_BLOCK, (c.NI + 15) / 16, lds_bytes);
            out = pl;
            return true;
        }
        pl.m = m0;          // (images above the LDS limit: the generic plan, on the unedited net)
    }
    if (c.z2) return false;
    // mixed or narrow widths up to 63 run zero-padded on the shape-exact kernels (fwd_pad = 0 keeps the generic ones)
    lay = fwd_images(pl.m, pl.img, nparts, tmax, wide, nparts == 2 && o.fwd_pad, o.fwd_pad_min);
    const bool flagship = lay.exact && lay.T == 4 && nparts == 2;
    // the 32x32x16 formulation of the flagship shape: opt-in (fwd_pipe = 2), bf16 build only.  Same wall time as the default at C3
    // with 10 % fewer cycles -- the chip clocks it lower (the kernel is power-bound)
    if (!f16 && o.fwd_pipe == 2 && flagship && lay.nrl == 13 && fwd_p32_shape(m0)) {
        FwdPlan p32 = out;
        p32.nparts = 2;
        fwd_images_p32(p32.m);
        const size_t lds_bytes = (size_t)p32.m.lds_off[L] * sizeof(float);
        if (lds_bytes <= UMNN_LDS_LIMIT) {
            fwd_plan_grid(p32, FWD_FAMILY_P32, kFwdP32Name, L - 2, 2, 1, UMNN_WAVES_PER_BLOCK, (c.NI + 31) / 32, lds_bytes);
            out = p32;
            return true;
        }
    }
    // the pipelined loop needs two point tiles per wave and pays off as soon as that still leaves a wave per SIMD
    // (measured at the POWER and VAE shapes: P=2, NS=1 beats every P=1 split by 6-7 %)
    const bool want_pipe = o.fwd_pipe != 0 && L >= 2;
    if (want_pipe && flagship && !p_set && !ns_set && tiles16 >= 2LL * cus * 4) { P = 2; ns = 1; }
    const size_t image_bytes = (size_t)pl.m.lds_off[L] * sizeof(float);
    int wpb = fwd_waves(lay, nparts, image_bytes);
    auto lds_for = [&](int waves) { return image_bytes + (ns > 1 ? (size_t)waves * 3 * P * 16 * sizeof(float) : 0); };
    if (wpb == 8 && lds_for(wpb) > UMNN_LDS_LIMIT) wpb = UMNN_WAVES_PER_BLOCK;
    if (lds_for(wpb) > UMNN_LDS_LIMIT) return false;
    const int v = fwd_pick(rows, count, lay, tmax, nparts, P, want_pipe, wpb);
    if (v < 0) return false;
    fwd_plan_grid(pl, FWD_FAMILY_PIECES, rows[v].name, v, P, ns, rows[v].wpb, (c.NI + 16 * P - 1) / (16 * P), lds_for(wpb));
    out = pl;
    return true;
}

// fp32 MFMA: exact (compile-time K-steps) when all hidden layers share a width that is instantiated -- with the VALU tail when
// every hidden layer has the same width H with 16 (T - 1) <= H <= 16 (T - 1) + 3 --, otherwise the smallest generic tile count
inline void fwd_plan_fp32(FwdPlan& pl, int tmax, int ksu, const FwdCall& c, const FwdOptions& o, int P, int ns) {
    const int L = pl.m.n_linear - 1, nt = pl.m.width[1] - 16 * (tmax - 1);
    int want_tail = (ksu && ksu == 4 * (tmax - 1) + 1 && nt >= 0 && nt <= 3) ? 1 : 0;
    if (o.fwd_tail >= 0) want_tail = want_tail && o.fwd_tail != 0;
    int v = -1;
    for (int tl = want_tail; tl >= 0 && v < 0; --tl)
        for (int i = 0; i < kFwdFp32Count && v < 0; ++i) {
            const FwdFp32Row& r = kFwdFp32Rows[i];
            if (r.ksc && r.ksc == ksu && r.tmax == tmax && r.p == P && r.tail == tl && (!tl || r.nt == nt)) v = i;
        }
    for (int i = 0; i < kFwdFp32Count && v < 0; ++i)
        if (!kFwdFp32Rows[i].ksc && kFwdFp32Rows[i].tmax >= tmax && kFwdFp32Rows[i].p == P) v = i;
    if (v < 0) return fwd_plan_fail(pl, "forward: hidden width above UMNN_MAX_HIDDEN_WIDTH");
    if (kFwdFp32Rows[v].tail) fwd_images_fp32_tail(pl.m, tmax);
    const size_t lds_bytes = ((size_t)pl.m.lds_off[L] + (ns > 1 ? UMNN_WAVES_PER_BLOCK * 3 * P * 16 : 0)) * sizeof(float);
    if (lds_bytes > UMNN_LDS_LIMIT) return fwd_plan_fail(pl, "forward: weight images exceed 160 KiB of LDS");
    fwd_plan_grid(pl, FWD_FAMILY_FP32, kFwdFp32Rows[v].name, v, P, ns, UMNN_WAVES_PER_BLOCK, (c.NI + 16 * P - 1) / (16 * P), lds_bytes);
}

// Search and solve: the forward's P = 1 plans, except that 3..4-tile nets are always padded and uniform wide nets may run on any
// piece count.  Build and pieces by fwd_precision.  f16x3 (default): two fp16 pieces (fp32-level products) with the queued bf16x3
// fallback.  bf16x3: two bf16 pieces.  fp32 / bf16x6 ("exact products everywhere"): three bf16 pieces, which exist for up to four tiles
// per layer -- 8 tiles x 3 pieces do not fit the register file, so wider nets get their fp32-level products from the two-fp16-piece
// build instead: the same accuracy class, ~5e-7 on F; a tile whose integrals overflow fp16 is redone on two bf16 pieces, ~6e-6 on F
// (for the search, orders of magnitude inside its own resolution 100 / 9^iter for all but the last rounds).
#define UMNN_INV_TEXT(job, text) ((job) == FWD_JOB_SEARCH ? "invert: " text : "solve: " text)
inline void fwd_plan_inverse(FwdPlan& pl, int tmax, const FwdCall& c, const FwdOptions& o, int cus) {
    const int L = pl.m.n_linear - 1, prec = o.fwd_precision;
    if (L < 2) return fwd_plan_fail(pl, UMNN_INV_TEXT(c.job, "the matrix-core kernels need at least two hidden layers"));
    pl.f16 = prec == UMNN_PRECISION_F16X3 || (prec != UMNN_PRECISION_BF16X3 && tmax > 4);
    pl.nparts = pl.f16 || prec == UMNN_PRECISION_BF16X3 ? 2 : 3;
    pl.fallback = pl.f16;
    int count = 0;
    const FwdRow* rows = fwd_rows(c.job, pl.f16 != 0, &count);
    FwdLayout lay;
    if (fwd_images_wide_first(pl.m, pl.img, 2, &lay)) {                // (above four tiles every mode runs on two pieces)
        const int ns = fwd_split_over(c.groups, UMNN_WAVES_PER_BLOCK, c.n, cus);
        const size_t lds_bytes = ((size_t)pl.m.lds_off[L] + (ns > 1 ? c.scratch * UMNN_WAVES_PER_BLOCK : 0)) * sizeof(float);
        const int v = fwd_pick_wide_first(rows, count, lay);
        if (v < 0 || lds_bytes > UMNN_LDS_LIMIT) return fwd_plan_fail(pl, UMNN_INV_TEXT(c.job, "weight images exceed 160 KiB of LDS"));
        return fwd_plan_grid(pl, FWD_FAMILY_WIDE_FIRST, rows[v].name, v, 1, ns, UMNN_WAVES_PER_BLOCK, c.groups, lds_bytes);
    }
    lay = fwd_images(pl.m, pl.img, pl.nparts, tmax, fwd_uniform_wide(pl.m, tmax), true, 3);
    const size_t image_bytes = (size_t)pl.m.lds_off[L] * sizeof(float);
    if (image_bytes > UMNN_LDS_LIMIT) return fwd_plan_fail(pl, UMNN_INV_TEXT(c.job, "weight images exceed 160 KiB of LDS"));
    const int v = fwd_pick(rows, count, lay, tmax, pl.nparts, 1, false, fwd_waves(lay, pl.nparts, image_bytes));
    if (v < 0) return fwd_plan_fail(pl, UMNN_INV_TEXT(c.job, "no kernel variant for this shape"));
    int ns = fwd_split_over(c.groups, rows[v].wpb, c.n, cus);
    size_t lds_bytes = image_bytes + (ns > 1 ? (size_t)c.scratch * rows[v].wpb * sizeof(float) : 0);
    if (lds_bytes > UMNN_LDS_LIMIT) { ns = 1; lds_bytes = image_bytes; }         // (the scratch does not fit: unsplit)
    fwd_plan_grid(pl, FWD_FAMILY_PIECES, rows[v].name, v, 1, ns, rows[v].wpb, c.groups, lds_bytes);
}

// The plan of one call.  m0 / tmax / ksu: what umnn_prepare_mlp left.
inline FwdPlan fwd_plan(const MlpDev& m0, int tmax, int ksu, const FwdCall& c, const FwdOptions& o, int cus) {
    FwdPlan pl{};
    pl.m = m0;
    pl.name = "";
    if (c.job != FWD_JOB_FORWARD) { fwd_plan_inverse(pl, tmax, c, o, cus); return pl; }
    // a wave owns P tiles of 16 integrals: two once every SIMD has eight; below two per SIMD the node range is split instead
    const long long tiles16 = (c.NI + 15) / 16, simd_slots = (long long)cus * 4;
    int P = tiles16 >= 8 * simd_slots ? 2 : 1;
    int ns = fwd_split(tiles16, simd_slots, 2 * simd_slots - 1, c.n);
    if (o.fwd_p > 0) P = o.fwd_p;
    // (a forced split obeys the same limit as the rule: part 0 of a range cut into more parts than nodes is empty, and the wave
    // that owns part 0 is the one that publishes f(x))
    if (o.fwd_ns > 0) ns = o.fwd_ns > c.n + 1 ? 1 : o.fwd_ns;
    const int prec = o.fwd_precision;
    if (c.z2 && (prec == UMNN_PRECISION_FP32 || prec == UMNN_PRECISION_BF16X6)) {
        fwd_plan_fail(pl, "forward (z_2 saved): two-piece arithmetic modes only");
        return pl;
    }
    // Piece kernels (default): hidden GEMMs on the 16-bit matrix cores (a single hidden layer has no hidden->hidden GEMM at all).
    // f16x3 (default): two fp16 pieces, three cross terms (fp32-level), the bf16x3 build queued behind it for tile groups whose pieces
    // overflow.  The deferred groups are marked IN the output (F, or z), so a launch whose marker output aliases one of its inputs runs
    // bf16x3 outright -- the arithmetic its overflowing groups would get anyway.  Shapes that family does not cover take the
    // three-piece bf16 kernels (the same accuracy class), then fp32 MFMA.
    if (prec != UMNN_PRECISION_FP32 && m0.n_linear - 1 >= 2) {
        if (prec == UMNN_PRECISION_F16X3 && fwd_plan_pieces(pl, m0, tmax, c, o, cus, !c.alias, 2, P, ns)) return pl;
        if (fwd_plan_pieces(pl, m0, tmax, c, o, cus, false, prec == UMNN_PRECISION_BF16X3 ? 2 : 3, P, ns)) return pl;
    }
    if (c.z2) fwd_plan_fail(pl, "forward (z_2 saved): this net / launch is not served by the wide-first kernels");
    else fwd_plan_fp32(pl, tmax, ksu, c, o, P, ns);
    return pl;
}
