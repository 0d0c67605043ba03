// Launch plan of the quadrature backward, decided once: which kernel family a call runs, with which grid, LDS bytes and kernel
// name, written for its launchers (cc_backward.hip, cc_backward_bf16.hip, cc_backward_front.hip and its _p3 build) and for the
// read-only queries (umnn_cc_backward_workspace_bytes, _kind, _plan_name).  Plain host arithmetic: no HIP call, no global state,
// no umnn_options() read -- the caller passes a snapshot of the backward options and the CU count.  Two levels, because nb_steps
// is not known when the workspace is sized:
//   bwd_plan_shape   (net, B, d, E) -> BwdShapePlan: padding to an exact family, tile counts, waves per workgroup, node-range
//                    split, grid, workspace offsets;
//   bwd_route        shape plan + (nb_steps, inv_f, g_fx / z_2 / launch scalars present) -> BwdRoute: ONE family and everything
//                    its launcher needs.  A launcher never falls through to another family: a shape it cannot run is a
//                    predicate here.
#pragma once
#include "cc_bwd_bf16_kernel.h"
#if UMNN_BWD_NPB == 2
#include "cc_bwd_ws16_kernel.h"      // (the pipelines' sizes; the _p3 build of the three-stage family executes a route, it decides nothing)
#endif

constexpr size_t BWD_LDS_LIMIT = UMNN_LDS_LIMIT;      // (cc_host.h: shared with the forward plan)

struct BwdOptions { int bwd_precision, bwd_ws, bwd_ws16, bwd_swp, bwd_ns, front_bwd2; };

enum BwdFamily {
    BWD_FAMILY_FRONT = 1,   // three stages through HBM (cc_backward_front.hip; BwdFrontRoute::npb = 3: its _p3 build)
    BWD_FAMILY_WS16,        // workgroup pipeline on fp16 pieces, the bf16 pipeline queued behind it as the overflow fallback
    BWD_FAMILY_WS,          // workgroup pipeline on bf16 pieces
    BWD_FAMILY_SWP,         // software-pipelined one-pass loop
    BWD_FAMILY_LOOP,        // round-2 one-pass loop
    BWD_FAMILY_FP32,        // fp32-MFMA passes
};

// ---- kernels that take BwdBf16Args: one record type, one lookup; the names live here (the route reports them without device code)
enum BwdKind { BWD_KIND_LOOP, BWD_KIND_SWP, BWD_KIND_WS, BWD_KIND_WS16, BWD_KIND_MID, BWD_KIND_MID_P3, BWD_KIND_MID_WS, BWD_KIND_MID_WS16 };
typedef void (*bwd_bf16_kernel_t)(const BwdBf16Args);
struct BwdBf16Variant { int kind, lh, nrl; bwd_bf16_kernel_t fn; };
template <int N>
inline bwd_bf16_kernel_t bwd_bf16_fn(const BwdBf16Variant (&table)[N], int kind, int lh, int nrl) {
    for (const BwdBf16Variant& v : table)
        if (v.kind == kind && v.lh == lh && v.nrl == nrl) return v.fn;
    return nullptr;
}
// (LH, LIVE) of the one-pass kernels: LIVE=13 every hidden layer 48..51 wide (dead registers cost no VALU), LIVE=0 (all 16 registers)
// every other net of three or four tiles per layer; the workgroup pipelines hold four hidden layers
#define UMNN_BWD_LOOP_SHAPES(X, ...) X(4, 13, __VA_ARGS__) X(3, 13, __VA_ARGS__) X(2, 13, __VA_ARGS__) X(4, 0, __VA_ARGS__) X(3, 0, __VA_ARGS__) X(2, 0, __VA_ARGS__)
#define UMNN_BWD_WS_SHAPES(X, ...) X(4, 13, __VA_ARGS__) X(4, 0, __VA_ARGS__)
struct BwdKernelName { int kind, lh, nrl; const char* name; };
#define UMNN_BWD_NAME(LH, NR, KIND, STEM, MIDDLE, TAIL) { KIND, LH, NR, STEM "<L=" #LH MIDDLE "LIVE=" #NR TAIL ">" },
constexpr BwdKernelName kBwdKernelNames[] = {
    UMNN_BWD_LOOP_SHAPES(UMNN_BWD_NAME, BWD_KIND_LOOP, "cc_bwd_bf16", ",EDGE=1,", "")
    UMNN_BWD_LOOP_SHAPES(UMNN_BWD_NAME, BWD_KIND_SWP, "cc_bwd_bf16", ",", ",SWP")
    UMNN_BWD_WS_SHAPES(UMNN_BWD_NAME, BWD_KIND_WS, "cc_bwd_bf16", ",", ",WS")
    UMNN_BWD_WS_SHAPES(UMNN_BWD_NAME, BWD_KIND_WS16, "cc_bwd_f16", ",", ",WS")
    UMNN_BWD_LOOP_SHAPES(UMNN_BWD_NAME, BWD_KIND_MID, "cc_bwd_bf16", ",EDGE=1,", ",FRONT")
    UMNN_BWD_LOOP_SHAPES(UMNN_BWD_NAME, BWD_KIND_MID_P3, "cc_bwd_bf16x6", ",EDGE=1,", ",FRONT")
    UMNN_BWD_WS_SHAPES(UMNN_BWD_NAME, BWD_KIND_MID_WS, "cc_bwd_bf16", ",", ",WS,FRONT")
    UMNN_BWD_WS_SHAPES(UMNN_BWD_NAME, BWD_KIND_MID_WS16, "cc_bwd_f16", ",", ",WS,FRONT")
};
inline const char* bwd_kernel_name(int kind, int lh, int nrl) {
    for (const BwdKernelName& v : kBwdKernelNames)
        if (v.kind == kind && v.lh == lh && v.nrl == nrl) return v.name;
    return nullptr;
}

// ---- the fp32-MFMA variants (cc_backward.hip instantiates cc_bwd_kernel<T, NACC, EDGE, KS> from the same list, in this order)
#define UMNN_BWD_FP32_VARIANTS(X) \
    X(4, 3, 1, 13) X(4, 3, 0, 13)                      /* exact: every hidden layer 48..51 wide (UCI / VAE nets) */ \
    X(2, 3, 1, 0) X(2, 3, 0, 0) \
    X(4, 3, 1, 0) X(4, 3, 0, 0) \
    X(5, 2, 1, 17) X(5, 3, 0, 17)                      /* exact: every hidden layer 64 wide */ \
    X(7, 1, 1, 26) X(7, 0, 1, 26) X(7, 1, 0, 26)       /* exact: every hidden layer 100 wide (toy flows, MonotonicNN): no spills */ \
    X(7, 0, 1, 0) X(7, 1, 0, 0) \
    X(8, 0, 1, 0) X(8, 1, 0, 0) \
    X(8, 0, 1, 32) X(8, 1, 0, 32)                      /* exact: every hidden layer 124..127 wide, or zero-padded to that (edge pass without dW: no spills; 51 in the others) */
struct BwdFp32Variant { int tmax, nacc, edge, ksc; const char* name; };
#define UMNN_BWD_FP32_ROW(T, N, E, K) { T, N, E, K, "cc_bwd<T=" #T ",NACC=" #N ",EDGE=" #E ",KS=" #K ">" },
constexpr BwdFp32Variant kBwdFp32Variants[] = { UMNN_BWD_FP32_VARIANTS(UMNN_BWD_FP32_ROW) };
constexpr int kBwdFp32Count = (int)(sizeof(kBwdFp32Variants) / sizeof(kBwdFp32Variants[0]));

// index of the variant, preferring the shape-exact family; -1: none
inline int find_bwd(int tmax, int nacc, int edge, int ksu) {
    for (int exact = 1; exact >= 0; --exact)
        for (int i = 0; i < kBwdFp32Count; ++i) {
            const BwdFp32Variant& v = kBwdFp32Variants[i];
            if (v.tmax == tmax && v.nacc == nacc && v.edge == edge && (exact ? (v.ksc && v.ksc == ksu) : !v.ksc)) return i;
        }
    return -1;
}
inline bool bwd_exact_family(int tmax, int ksu) {
    if (ksu)
        for (const BwdFp32Variant& v : kBwdFp32Variants)
            if (v.ksc == ksu && v.tmax == tmax) return true;
    return false;
}
// template tile count: the net's own when a shape-exact family exists for it, else the next generic bucket
inline int pick_tmax_bwd(int tmax, int ksu) {
    if (bwd_exact_family(tmax, ksu)) return tmax;
    return tmax <= 2 ? 2 : tmax <= 4 ? 4 : tmax <= 7 ? 7 : 8;
}
// dW layers a pass can hold: the largest NACC instantiated for (T, edge), preferring the shape-exact family
inline int best_nacc(int T, int edge, int ksu) {
    for (int exact = 1; exact >= 0; --exact)
        for (int n = 3; n >= 0; --n)
            for (const BwdFp32Variant& v : kBwdFp32Variants)
                if (v.tmax == T && v.nacc == n && v.edge == edge && (exact ? (v.ksc && v.ksc == ksu) : !v.ksc)) return n;
    return -1;
}

// Nets with UNEQUAL hidden widths above 63 units (5..7 tiles) have no shape-exact variant of their own, and the generic
// variants with runtime tile counts spill hundreds of registers there (687 ms per call at 256 x 784 integrals).  Pad them --
// virtually: only the per-layer tile and K-step counts change, the staged images carry the zeros and the constant-one feature
// of every layer stays at its own index width[l] -- to the smallest shape-exact family that holds the widest layer: (5 tiles,
// 17 K-steps: widths up to 67) or (7, 26: up to 103).  A padded unit has zero weights and bias, so z = 0, act(0) = 0, and it
// contributes exact zeros to every sum; d_theta is written for the real entries only.  Returns 1 if the net was padded.
inline int pad_to_exact_family(MlpDev& m, int* tmax, int* ksu) {
    if (*tmax <= 4 || bwd_exact_family(*tmax, *ksu)) return 0;
    const int L = m.n_linear - 1;
    int ksmax = 0;
    for (int l = 1; l <= L; ++l) ksmax = m.ks_in[l] > ksmax ? m.ks_in[l] : ksmax;
    static const int kFamilies[][2] = {{5, 17}, {7, 26}, {8, 32}};
    for (const auto& f : kFamilies) {
        if (*tmax > f[0] || ksmax > f[1]) continue;
        for (int l = 1; l <= L; ++l) { m.t_out[l] = m.t_mfma[l] = f[0]; m.ks_in[l] = f[1]; }
        int off = 0;
        for (int l = 1; l < L; ++l) { m.lds_off[l] = off; off += m.t_out[l + 1] * m.ks_in[l] * 64; }
        m.lds_off[L] = off;
        *tmax = f[0]; *ksu = f[1];
        return 1;
    }
    return 0;
}

// row stride for the row-major image: >= cols, minimising bank conflicts of both fragment shapes
// (forward: 16 rows x 2 adjacent cols per half-wave; backward: 2 adjacent rows x 16 cols)
inline int pick_ld(int cols) {
    int best = cols, best_cost = 1 << 30;
    for (int ld = cols; ld < cols + 33; ++ld) {
        int cost = 0;
        for (int pattern = 0; pattern < 2; ++pattern) {
            int cnt[32] = {0};
            for (int a16 = 0; a16 < 16; ++a16)
                for (int b2 = 0; b2 < 2; ++b2) {
                    const int addr = pattern == 0 ? a16 * ld + b2 : b2 * ld + a16;
                    cnt[((addr % 32) + 32) % 32]++;
                }
            int worst = 0;
            for (int b = 0; b < 32; ++b) worst = cnt[b] > worst ? cnt[b] : worst;
            cost += worst;
        }
        if (cost < best_cost) { best_cost = cost; best = ld; }
    }
    return best;
}

// LDS of the dW1[:,1:] finishing kernel (cc_bwd_dw0_kernel): dc integral-major with a row stride of 16 mod 32 floats, h column-major
__host__ __device__ inline int dw0_stride(int cols) { return ((cols + 15) / 16 * 16 + 16 + 31) / 32 * 32 - 16; }   // >= cols, = 16 mod 32
__host__ __device__ inline size_t dw0_lds_floats(int chunk, int H1, int E) {
    return (size_t)chunk * dw0_stride(H1) + (size_t)((E + 1 + 15) / 16 * 16) * (chunk + 4);
}

// ---- the pieces every family shares, once each
// persistent grid: at most nblocks_max workgroups of wpb waves, no more than the work items fill
inline int bwd_clamp_blocks(int nblocks_max, long long items, int wpb) {
    int nblocks = nblocks_max;
    if ((long long)nblocks * wpb > items) nblocks = (int)((items + wpb - 1) / wpb);
    return nblocks < 1 ? 1 : nblocks;
}
// live registers per lane of hidden layers l0..L when every one of them is 48..51 wide (13 K-steps of four features), else 0 = all 16
inline int bwd_live_regs(const MlpDev& m, int l0) {
    for (int l = l0; l <= m.n_linear - 1; ++l) if (m.ks_in[l] != 13) return 0;
    return 13;
}
// ushort offsets of the one-pass kernels' LDS images for lh hidden layers (forward fragments of NPF pieces, transposed ones of npb
// pieces); returns where the per-wave transpose tiles start (off_trtile).  args may be null (sizes only).  (static: NPF and TRS are
// per-build names)
static inline int bwd_onepass_images(int lh, int npb, BwdBf16Args* args) {
    int off16 = 0;
    for (int l = 1; l < lh; ++l) { if (args) args->off_fwd[l] = off16; off16 += BT * BKS * UMNN_BWD_NS::NPF * FRAG; }
    for (int l = 1; l < lh; ++l) { if (args) args->off_tr[l] = off16; off16 += BT * BKS * npb * FRAG; }
    if (args) args->off_trtile = off16;
    return off16;
}
static inline size_t bwd_onepass_lds_bytes(int lh, int npb, int wpb) {
    return (size_t)(bwd_onepass_images(lh, npb, nullptr) + wpb * npb * 16 * UMNN_BWD_NS::TRS) * sizeof(unsigned short);
}
// grid of the cotangent-scale pre-pass of the fp16 pipeline (>= 4 integrals per thread; at most one workgroup per CU)
inline unsigned bwd_cotmax_blocks(long long NI, int nblocks_max) {
    const long long want = (NI + 1023) / 1024;
    return (unsigned)(want < (long long)nblocks_max ? want : (long long)nblocks_max);
}

// Does this net belong to the three-stage family?  hidden layer 1: 5..8 tiles; hidden layers 2..L: three or four tiles at most
// (zero-padded to four), 2..4 of them.
inline bool bwd_front_shape(const MlpDev& m) {
    const int L = m.n_linear - 1;
    if (L < 3 || L > 5) return false;
    if (m.t_out[1] < 5 || m.t_out[1] > 8) return false;
    for (int l = 2; l <= L; ++l) if (m.t_out[l] > BT) return false;
    return true;
}
// bytes of HBM scratch the three-stage backward wants for NI integrals (nb_steps is not known when the workspace is sized: the
// chunking adapts to whatever n the call brings)
inline long long bwd_front_scratch_bytes(const MlpDev& m, long long NI) {
    const long long tiles = (NI + 15) / 16;
    const long long nl2 = (m.width[2] + 1 + 3) / 4;
    const long long per_tile = (2LL * 257 + 1) * nl2 * 64 * 4;          // sized for n = 256
    const long long want = tiles * per_tile, cap = 2LL << 30;
    return want < cap ? want : cap;
}

// ------------------------------------------------------------------------------------------ the shape plan
struct BwdShapePlan {
    BwdArgs a;         // m (padded), image strides, theta offsets, NI / d / E / ngroups filled; the call's pointers are the launcher's
    int tmax;          // template tile count
    int ksu;           // common K-step count when every hidden layer fills exactly `tmax` tiles, else 0
    int padded;        // zero-padded to a shape-exact family
    int front_shape;   // first hidden layer of 5..8 tiles over 2..4 narrower ones (three-stage iff ws_front_bytes > 0)
    int nwaves, nblocks, wpb;
    int ns;            // node-range split (small batches: fewer tiles than waves)
    long long ws_partials, ws_dc, ws_p0;   // byte offsets in the workspace
    long long ws_scal;                     // 256 B of launch scalars (cc_bwd_ws16_kernel.h)
    long long ws_front, ws_front_bytes;    // HBM scratch of the three-stage backward, 0 if not that family
    long long ws_total;
    int nparts0, chunk0;
    size_t lds_bytes_for(int nacc, int waves) const { return (size_t)(a.scratch_off + waves * (nacc + 1) * tmax * 256) * sizeof(float); }
};
constexpr const char* kBwdLdsError = "backward: weight images exceed 160 KiB of LDS";
constexpr const char* kBwdVariantError = "backward: no kernel variant for this width";

// The net's part (no batch in it): family padding, tile counts, row-major image strides, waves per workgroup.  m0 / tmax0 / ksu0
// are what umnn_prepare_mlp left.  Returns nullptr, or the text of the UMNN_EUNSUPPORTED error (tmax / ksu / padded /
// front_shape are filled either way: umnn_cc_backward_kind reads them).
inline const char* bwd_plan_net(BwdShapePlan* pl, const MlpDev& m0, int tmax0, int ksu0) {
    BwdArgs& a = pl->a;
    // (the three-stage kernels take their shape first: they read the unpadded tile counts)
    pl->front_shape = bwd_front_shape(m0);
    // (the padded images of a deep net can exceed the LDS: the net's own counts then)
    for (int allow_pad = pl->front_shape ? 0 : 1; allow_pad >= 0; --allow_pad) {
        a.m = m0;
        int tmax = tmax0, ksu = ksu0;
        pl->padded = allow_pad ? pad_to_exact_family(a.m, &tmax, &ksu) : 0;
        pl->tmax = pick_tmax_bwd(tmax, ksu);
        pl->ksu = (ksu && tmax == pl->tmax) ? ksu : 0;
        const int L = a.m.n_linear - 1;
        int off = 0;
        for (int l = 1; l < L; ++l) {
            a.ld[l] = pick_ld(4 * a.m.ks_in[l]);
            a.roff[l] = off;
            off += 4 * a.m.ks_in[l + 1] * a.ld[l];
            off = (off + 3) & ~3;
        }
        a.scratch_off = off;
        // waves per workgroup: as many (4, 2, 1) as leave room for the wave-private transpose tiles
        const int nm = best_nacc(pl->tmax, 1, pl->ksu), nr = best_nacc(pl->tmax, 0, pl->ksu);
        const int nacc_max = nm > nr ? nm : nr;
        pl->wpb = 4;
        while (pl->wpb > 1 && pl->lds_bytes_for(nacc_max, pl->wpb) > BWD_LDS_LIMIT) pl->wpb >>= 1;
        if (pl->lds_bytes_for(nacc_max, pl->wpb) <= BWD_LDS_LIMIT) return nullptr;
        if (!pl->padded) break;
    }
    return kBwdLdsError;
}

// The whole shape plan of (net, B, d, E), B >= 1.  cus: CU count of the device; bwd_ns: that option.
inline const char* bwd_plan_shape(BwdShapePlan* pl, const MlpDev& m0, int tmax0, int ksu0, long long B, int d, int E, int cus, int bwd_ns) {
    if (const char* err = bwd_plan_net(pl, m0, tmax0, ksu0)) return err;
    BwdArgs& a = pl->a;
    const int H1 = a.m.width[1];
    a.n_params = bwd_param_offsets(a.m, a.poffW, a.poffb);
    a.NI = B * (long long)d; a.d = d; a.E = E;
    a.ngroups = (unsigned)((a.NI + 15) / 16);
    // fewer tiles than waves (the reference's own training batches are 100 samples): share a tile's nodes among
    // up to 32 waves; every work item keeps its own d_theta / dc partial, summed in a fixed order afterwards
    pl->ns = 1;
    {
        const long long waves = (long long)cus * pl->wpb;
        if ((long long)a.ngroups * 2 <= waves) pl->ns = (int)(waves / a.ngroups > 32 ? 32 : waves / a.ngroups);
        if (bwd_ns >= 1 && bwd_ns <= 32) pl->ns = bwd_ns;
    }
    pl->nblocks = bwd_clamp_blocks(cus, (long long)a.ngroups * pl->ns, pl->wpb);
    pl->nwaves = pl->nblocks * pl->wpb;
    a.ns = 1;
    pl->chunk0 = 64;
    while (pl->chunk0 > 16 && dw0_lds_floats(pl->chunk0, H1, E) * sizeof(float) > 32 * 1024) pl->chunk0 /= 2;
    while (pl->chunk0 > 16 && a.NI / pl->chunk0 < 2LL * cus) pl->chunk0 /= 2;     // small batches: more, smaller chunks
    {   // persistent blocks (four per CU), each accumulating its chunks in registers: at most that many partial slices
        const long long nchunks = (a.NI + pl->chunk0 - 1) / pl->chunk0, cap = 4LL * cus;
        pl->nparts0 = (int)(nchunks < cap ? nchunks : cap);
    }
    // The workspace.  nwaves, NI * ns and nparts0 all jump DOWN somewhere as B grows (ns falls as the tiles fill the waves; chunk0
    // doubles at 2 * cus chunks), so their regions are sized by bounds that never shrink with B: a workspace sized for the largest
    // batch holds every smaller one.
    const bool ns_forced = bwd_ns >= 1 && bwd_ns <= 32;
    const long long waves = (long long)cus * pl->wpb;
    const long long nwaves_bound = (long long)bwd_clamp_blocks(cus, (long long)a.ngroups * (ns_forced ? bwd_ns : 32), pl->wpb) * pl->wpb;
    // (unforced, ns <= 32 and ns <= waves / ngroups, and NI <= 16 ngroups)
    const long long dc_free = 16 * waves > a.NI ? 16 * waves : a.NI;
    const long long dc_bound = ns_forced ? a.NI * bwd_ns : (32 * a.NI < dc_free ? 32 * a.NI : dc_free);
    const long long nparts0_bound = (a.NI + 15) / 16 < 4LL * cus ? (a.NI + 15) / 16 : 4LL * cus;     // (chunk0 >= 16)
    long long o = 0;
    pl->ws_partials = o; o += nwaves_bound * a.n_params * 4; o = (o + 255) & ~255LL;
    pl->ws_dc = o; o += dc_bound * H1 * 4; o = (o + 255) & ~255LL;
    pl->ws_p0 = o; o += nparts0_bound * H1 * (E + 1) * 4; o = (o + 255) & ~255LL;
    pl->ws_scal = o; o += 256;
    pl->ws_front = o;
    pl->ws_front_bytes = (pl->front_shape && pl->wpb == 4) ? bwd_front_scratch_bytes(a.m, a.NI) : 0;
    o += pl->ws_front_bytes; o = (o + 255) & ~255LL;
    pl->ws_total = o;
    return nullptr;
}

// ------------------------------------------------------------------------------------------ the route of a call
enum BwdMidStage { BWD_MID_LOOP, BWD_MID_WS, BWD_MID_WS16 };
enum BwdStageC { BWD_STAGE_C_BWD, BWD_STAGE_C_BWD2, BWD_STAGE_C_BWD16 };
struct BwdFrontRoute {
    int npb;               // build: 2 pieces (cc_backward_front.hip) or 3 (its _p3 build)
    int T1, nl2, nl2_variant;      // tiles of hidden layer 1; live registers of hidden layer 2, and the stage kernels' NL2 (13 or 0)
    int saved;             // z_2 came with the call: the scratch holds delta_2 and the tangent only
    long long tiles, chunk;
    int wpb_mid, wpb_ws;   // waves per workgroup of the one-pass middle kernel / of the pipelines
    size_t lds_a, lds_mid, lds_c, lds_c2, lds_ws, lds_ws16;
    int mid_ws;            // the middle stage may run as a workgroup pipeline (chunks of >= four tiles per workgroup)
    int mid_ws16;          // ... on fp16 pieces (single-chunk calls only: its d_theta slices are written, not accumulated)
    int stage_c;           // BwdStageC
    const char* name_mid;  // what a one-pass middle stage would note
    // the middle stage of a chunk of nt tiles
    int mid_stage(long long nt, int nblocks_max) const {
        return mid_ws16 ? BWD_MID_WS16 : (mid_ws && nt >= 4LL * nblocks_max) ? BWD_MID_WS : BWD_MID_LOOP;
    }
};
struct BwdFp32Pass { int variant, nacc, l_lo; size_t lds_bytes; };
struct BwdRoute {
    const char* error;     // non-null: the call returns UMNN_EUNSUPPORTED with this text and launches nothing
    int family;            // BwdFamily
    const char* name;      // what the call notes last under UMNN_PROF_BACKWARD
    int L, nrl;            // hidden layers and live registers of the main BwdBf16Args kernel (bf16 families)
    int wpb, nblocks;      // waves per workgroup and grid of the main kernel (three-stage: nblocks = the grid cap of a chunk)
    size_t lds_bytes, lds16_bytes;     // main kernel (WS16: of the queued bf16 pipeline) / the fp16 pipeline
    unsigned cotmax_blocks;            // WS16 and fp16 middle stage: grid of the cotangent-scale pre-pass
    int nslices;           // d_theta slices the main pass writes
    int ns;                // node-range split in force
    int use_z2;            // BwdArgs::z2_saved is passed on (else the buffer is ignored and z_2 recomputed)
    int npasses;           // BWD_FAMILY_FP32: the EDGE pass (with as many dW layers as its variant holds), then the remaining layers
    BwdFp32Pass pass[UMNN_MAX_LINEAR];
    BwdFrontRoute front;
};

// The launchers execute a route; one they cannot run is an internal error and launches nothing.  `base`: the fully populated BwdArgs
// of the call (partials zeroed).
int umnn_launch_backward_bf16(const BwdArgs& base, const umnn_mlp* net, const BwdRoute& rt, hipStream_t stream);
int umnn_launch_backward_front(const BwdArgs& base, const umnn_mlp* net, const BwdRoute& rt, void* scratch, hipStream_t stream);
// (the same with three pieces in every product: cc_backward_front_p3.hip, bwd_precision = fp32)
int umnn_launch_backward_front_p3(const BwdArgs& base, const umnn_mlp* net, const BwdRoute& rt, void* scratch, hipStream_t stream);
// the fp16 pipeline's kernels live in cc_backward_bf16.hip (built under that file's scheduling flags): the launch scalars (zeroed, then
// the cotangent scale) of a call, once, ahead of its stages; and the middle stage of the three-stage family on fp16 pieces
int umnn_ws16_prepare(const BwdArgs& base, unsigned cotmax_blocks, hipStream_t stream);
int umnn_ws16_mid_launch(const BwdBf16Args& mid, int nrl, int nblocks, size_t lds_bytes, hipStream_t stream);
constexpr const char* kBwdRouteError = "backward: internal error, a launcher was handed a route it cannot run";

#if UMNN_BWD_NPB == 2
// the workgroup pipelines want an unsplit node range and four tiles per workgroup to keep every stage busy
inline bool bwd_ws_fills(long long tiles, int ns, int nblocks) { return ns <= 1 && tiles >= 4LL * nblocks; }
// fp16 pieces for a workgroup pipeline (whole net, or the middle stage of the three-stage family).  bwd_ws16 = 1 (default): only
// for launches of at least 2^21 node evaluations (2^22 until the whole GPU suite had passed at 2^21).  Its recompute carries ~3e-7
// of relative noise on a pre-activation (fp32: ~1e-7), i.e. 3-4 times as many LeakyReLU kink decisions differ from an exact
// evaluation; one such decision moves d_theta by ~4e-5 of its largest entry at 4e5 node evaluations (tools/bwd_truth64.py) and by
// 1 / N of that beyond, so below the threshold the six-term bf16 pipeline keeps mid-size batches inside the 1e-4 parity band.
// bwd_ws16 = 2: whenever the pipeline is eligible (tests, measurements).  1/f launches, sigmoid outputs and quadratures whose
// tables do not fit the kernel's LDS copy keep the bf16 pipeline.
inline bool bwd_ws16_ok(const BwdOptions& o, long long NI, int n, bool inv_f, bool has_scal, int out_act) {
    const bool size_ok = o.bwd_ws16 == 2 || (o.bwd_ws16 == 1 && NI * (long long)(n + 1) >= (1LL << 21));
    return size_ok && !inv_f && has_scal && out_act == UMNN_OUT_ELU_PLUS_ONE && n + 1 <= W16_MAX_NODES;
}

// three-stage family: false when this call cannot run it (scratch too small for one tile at this n, images above the LDS limit,
// no variant) -- the call then takes the fp32 passes
inline bool bwd_route_front(const BwdShapePlan& pl, int n, bool inv_f, bool has_gfx, bool has_scal, const BwdOptions& o, BwdRoute* rt) {
    const MlpDev& m = pl.a.m;
    BwdFrontRoute& f = rt->front;
    const int LH = m.n_linear - 2;
    f.npb = o.bwd_precision == UMNN_PRECISION_BF16X3 ? 2 : 3;
    f.T1 = m.t_out[1];
    f.nl2 = (m.width[2] + 1 + 3) / 4;
    f.nl2_variant = f.nl2 == 13 ? 13 : 0;
    rt->L = LH; rt->nrl = bwd_live_regs(m, 2);
    f.name_mid = bwd_kernel_name(f.npb == 2 ? BWD_KIND_MID : BWD_KIND_MID_P3, LH, rt->nrl);
    if (!f.name_mid) return false;
    f.saved = rt->use_z2;
    f.tiles = pl.a.ngroups;
    const long long per_tile = ((f.saved ? 1LL : 2LL) * (n + 1) + (has_gfx ? 1 : 0)) * f.nl2 * 64 * 4;
    f.chunk = pl.ws_front_bytes / per_tile;
    if (f.chunk < 1) return false;
    if (f.chunk > f.tiles) f.chunk = f.tiles;
    else {
        // several chunks: equal shares, rounded up to whole rounds of the persistent grid where the scratch allows (a chunk
        // of 3.06 rounds costs 4)
        const long long nchunks = (f.tiles + f.chunk - 1) / f.chunk, waves = (long long)pl.nblocks * UMNN_WAVES_PER_BLOCK;
        const long long even = (f.tiles + nchunks - 1) / nchunks;
        const long long rounded = (even + waves - 1) / waves * waves;
        f.chunk = rounded <= f.chunk ? rounded : even;
    }
    // (waves per workgroup of the one-pass middle kernel: four, or as many as leave room for their transpose tiles next to the weight
    // images -- the six-term build with four hidden layers after the cut holds two; the grid grows by the same factor, so the
    // d_theta slices stay one per wave of the plan)
    f.wpb_mid = UMNN_WAVES_PER_BLOCK;
    while (f.wpb_mid > 1 && bwd_onepass_lds_bytes(LH, f.npb, f.wpb_mid) > BWD_LDS_LIMIT) f.wpb_mid >>= 1;
    f.lds_mid = bwd_onepass_lds_bytes(LH, f.npb, f.wpb_mid);
    f.lds_a = ((size_t)BT * (f.T1 / 2) * NPF * FRAG + (f.T1 & 1 ? BT * NPF * 256 : 0)) * sizeof(unsigned short);
    f.lds_c = (size_t)f.T1 * BKS * f.npb * FRAG * sizeof(unsigned short);
    f.lds_c2 = f.lds_c + (size_t)2 * UMNN_WAVES_PER_BLOCK * 2 * (f.npb * 16 * TRS) * sizeof(unsigned short);      // + the waves' operand tiles
    f.wpb_ws = WS_WAVES;
    f.lds_ws = (size_t)WS_LDS_USHORTS * sizeof(unsigned short);
    f.lds_ws16 = (size_t)W16_LDS_USHORTS * sizeof(unsigned short);
    if (f.lds_mid > BWD_LDS_LIMIT || f.lds_a > BWD_LDS_LIMIT || f.lds_c > BWD_LDS_LIMIT) return false;
    // stage C with two waves per tile (two-piece build): front_bwd2 = 0 keeps one wave per tile
    const bool c2 = f.npb == 2 && o.front_bwd2 != 0;
    if (c2 && f.lds_c2 > BWD_LDS_LIMIT) return false;
    // the middle stage as a workgroup pipeline (two-piece build, four hidden layers after the cut); on fp16 pieces for one chunk
    f.mid_ws = f.npb == 2 && o.bwd_ws && LH == 4 && bwd_kernel_name(BWD_KIND_MID_WS, LH, rt->nrl);
    f.mid_ws16 = f.mid_ws && f.chunk == f.tiles && bwd_ws_fills(f.tiles, 1, pl.nblocks) &&
                 bwd_ws16_ok(o, pl.a.NI, n, inv_f, has_scal, m.out_act) && bwd_kernel_name(BWD_KIND_MID_WS16, LH, rt->nrl);
    // ... and stage C on fp16 pieces behind the fp16 middle stage (front_bwd2 = 2 keeps bf16 pieces there)
    f.stage_c = c2 ? (f.mid_ws16 && o.front_bwd2 == 1 ? BWD_STAGE_C_BWD16 : BWD_STAGE_C_BWD2) : BWD_STAGE_C_BWD;
    rt->family = BWD_FAMILY_FRONT;
    rt->wpb = UMNN_WAVES_PER_BLOCK; rt->nblocks = pl.nblocks;
    rt->lds_bytes = f.lds_mid; rt->lds16_bytes = f.lds_ws16;
    rt->cotmax_blocks = bwd_cotmax_blocks(pl.a.NI, pl.nblocks);
    rt->nslices = pl.nwaves;
    rt->ns = 1;
    // (chunks only shrink: the first one decides whether any ran the pipeline)
    const int first = f.mid_stage(f.chunk, pl.nblocks);
    rt->name = first == BWD_MID_WS16 ? bwd_kernel_name(BWD_KIND_MID_WS16, LH, rt->nrl)
               : first == BWD_MID_WS ? bwd_kernel_name(BWD_KIND_MID_WS, LH, rt->nrl) : f.name_mid;
    return true;
}

// one-pass bf16 families: false for shapes outside them (more than three hidden->hidden layers, a layer above four tiles, one or
// two tiles per layer -- the fp32 kernels waste less --, images above the LDS limit, no variant)
inline bool bwd_route_bf16(const BwdShapePlan& pl, int n, bool inv_f, bool has_scal, const BwdOptions& o, BwdRoute* rt) {
    const MlpDev& m = pl.a.m;
    const int L = m.n_linear - 1;
    if (L < 2 || L - 1 > 3) return false;
    int tmax = 0;
    for (int l = 1; l <= L; ++l) {
        if (m.t_out[l] > BT) return false;
        tmax = m.t_out[l] > tmax ? m.t_out[l] : tmax;
    }
    if (tmax < 3) return false;
    const int nrl = bwd_live_regs(m, 1);
    const long long items = (long long)pl.a.ngroups * rt->ns;
    rt->L = L; rt->nrl = nrl;
    if (o.bwd_ws && L == 4 && bwd_kernel_name(BWD_KIND_WS, L, nrl) && bwd_ws_fills(items, rt->ns, pl.nblocks)) {
        const char* name16 = bwd_ws16_ok(o, pl.a.NI, n, inv_f, has_scal, m.out_act) ? bwd_kernel_name(BWD_KIND_WS16, L, nrl) : nullptr;
        rt->family = name16 ? BWD_FAMILY_WS16 : BWD_FAMILY_WS;
        rt->name = name16 ? name16 : bwd_kernel_name(BWD_KIND_WS, L, nrl);
        rt->wpb = WS_WAVES; rt->nblocks = pl.nblocks;
        rt->lds_bytes = (size_t)WS_LDS_USHORTS * sizeof(unsigned short);
        rt->lds16_bytes = (size_t)W16_LDS_USHORTS * sizeof(unsigned short);
        rt->cotmax_blocks = bwd_cotmax_blocks(pl.a.NI, pl.nblocks);
        rt->nslices = rt->nblocks < pl.nwaves ? rt->nblocks : pl.nwaves;       // one d_theta slice per workgroup
        return true;
    }
    const size_t lds_swp = ((size_t)(L - 1) * BT * BKS * NPF * FRAG + (size_t)UMNN_WAVES_PER_BLOCK * L * NPB * 16 * TRS) * sizeof(unsigned short);
    const bool swp = o.bwd_swp && bwd_kernel_name(BWD_KIND_SWP, L, nrl) && lds_swp <= BWD_LDS_LIMIT;
    rt->family = swp ? BWD_FAMILY_SWP : BWD_FAMILY_LOOP;
    rt->name = bwd_kernel_name(swp ? BWD_KIND_SWP : BWD_KIND_LOOP, L, nrl);
    rt->lds_bytes = swp ? lds_swp : bwd_onepass_lds_bytes(L, 2, UMNN_WAVES_PER_BLOCK);
    if (!rt->name || rt->lds_bytes > BWD_LDS_LIMIT) return false;
    rt->wpb = UMNN_WAVES_PER_BLOCK;
    rt->nblocks = bwd_clamp_blocks(pl.nblocks, items, rt->wpb);
    const int nw = rt->nblocks * rt->wpb;
    rt->nslices = nw < pl.nwaves ? nw : pl.nwaves;
    return true;
}

inline void bwd_route_fp32(const BwdShapePlan& pl, BwdRoute* rt) {
    const int T = pl.tmax, L = pl.a.m.n_linear - 1;
    const int nacc_main = best_nacc(T, 1, pl.ksu), nacc_rest = best_nacc(T, 0, pl.ksu);
    rt->family = BWD_FAMILY_FP32;
    rt->wpb = pl.wpb; rt->nblocks = pl.nblocks; rt->nslices = pl.nwaves;
    if (nacc_main < 0 || nacc_rest < 1) { rt->error = kBwdVariantError; return; }
    int l_next = 1;
    for (int pass = 0; pass == 0 || l_next < L; ++pass) {
        BwdFp32Pass& p = rt->pass[pass];
        p.nacc = pass == 0 ? nacc_main : nacc_rest;
        p.variant = find_bwd(T, p.nacc, pass == 0 ? 1 : 0, pl.ksu);
        p.l_lo = l_next;
        p.lds_bytes = pl.lds_bytes_for(p.nacc, pl.wpb);
        if (p.variant < 0) { rt->error = kBwdVariantError; return; }
        if (p.lds_bytes > BWD_LDS_LIMIT) { rt->error = kBwdLdsError; return; }
        rt->name = kBwdFp32Variants[p.variant].name;
        rt->npasses = pass + 1;
        l_next += p.nacc;
    }
}

// The route of one call.  has_scal: the launch scalars of the fp16 pipelines are there (the workspace always has them).
inline BwdRoute bwd_route(const BwdShapePlan& pl, int nb_steps, bool inv_f, bool has_gfx, bool has_z2, bool has_scal, const BwdOptions& o) {
    BwdRoute rt{};
    const bool bf16 = o.bwd_precision == UMNN_PRECISION_BF16X3;
    // (a call the three-stage kernels do not serve -- tiny batches, bwd_precision fp32 -- simply recomputes z_2: the buffer is ignored)
    rt.use_z2 = has_z2 && pl.ws_front_bytes > 0 && bf16;
    if (pl.ws_front_bytes > 0 && bwd_route_front(pl, nb_steps, inv_f, has_gfx, has_scal, o, &rt)) return rt;
    rt.ns = pl.ns > nb_steps + 1 ? nb_steps + 1 : pl.ns;
    if (bf16 && bwd_route_bf16(pl, nb_steps, inv_f, has_scal, o, &rt)) return rt;
    bwd_route_fp32(pl, &rt);
    return rt;
}
#endif  // UMNN_BWD_NPB == 2
