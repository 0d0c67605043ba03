// Weight-image layout of the cc_fwd_bf16_kernel family (cc_fwd_bf16_kernel.h), written once for its three launchers: the forward
// (cc_forward_bf16.hip) and the two inverse directions (cc_inv_launch.h: cc_invert.hip, cc_solve.hip).  Plain host arithmetic on the
// MlpDev inside the launch arguments -- no HIP calls; which family a launcher tries, and when, is that launcher's policy.
// Image l (hidden layer l -> l + 1) holds t_out[l + 1] output tiles x (ks32[l] K-steps of 32 features + half_in[l] half step) x
// nparts pieces of 512 (256) 16-bit words at ushort offset off16[l]; lds_off[L] is where the images end (floats, a multiple of
// four): the NS-reduction scratch starts there.
#pragma once
#include "cc_fwd_bf16_kernel.h"

namespace UMNN_FWD_NS {

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

inline void fwd_close_images(FwdBf16Args& args, int off16) { args.f.m.lds_off[args.f.m.n_linear - 1] = (((off16 + 1) / 2) + 3) & ~3; }

// Wide first hidden layer (T1 = 5..8 tiles) over a rest of at most four tiles each, zero-padded to four (MNISTExperiment's
// 31-100-50-50-50-50-1): layer 1's GEMM contracts over T1 tiles, the others over four.  False (nothing touched) for any other shape.
inline bool fwd_plan_wide_first(FwdBf16Args& args, int nparts, FwdLayout* lay) {
    MlpDev& m = args.f.m;
    const int L = m.n_linear - 1, T1 = m.t_out[1];
    if (L < 2 || T1 < 5 || T1 > 8) return false;
    for (int l = 2; l <= L; ++l) if (m.t_out[l] > 4) return false;
    int off16 = 0;
    for (int l = 1; l <= L; ++l) {
        args.pl.ks32[l] = l == 1 ? T1 / 2 : 2;
        args.pl.half_in[l] = l == 1 ? (T1 & 1) : 0;
        if (l >= 2) m.t_out[l] = 4;
    }
    for (int l = 1; l < L; ++l) {
        args.pl.off16[l] = off16;
        off16 += 4 * (args.pl.ks32[l] * nparts * 512 + args.pl.half_in[l] * nparts * 256);
    }
    fwd_close_images(args, off16);
    int nrest = m.ks_in[2];           // live registers of the later layers when they all agree (13 = widths 48..51)
    for (int l = 2; l <= L; ++l) if (m.ks_in[l] != nrest) nrest = 0;
    *lay = FwdLayout{T1, 1, nrest == 13 ? 13 : 0, 0};
    return true;
}

// Every other net.  wide (fwd_uniform_wide, or 0 where the launcher has no such variant): images of wide / 2 K-steps and a half one.
// Otherwise one K-step per pair of tiles of the layer as it is (the generic variants read the counts at run time) -- unless pad:
// mixed or narrow nets of pad_min..4 tiles are zero-padded to four tiles per layer (the staged images carry the zeros) and run the
// shape-exact kernels: the padded MFMAs cost less than the runtime guards of the generic variants.
inline FwdLayout fwd_plan_images(FwdBf16Args& args, int nparts, int tmax, int wide, bool pad, int pad_min) {
    MlpDev& m = args.f.m;
    const int L = m.n_linear - 1;
    FwdLayout lay{wide ? wide : fwd_tile_bucket(tmax), 1, m.ks_in[1], wide};
    int off16 = 0;
    for (int l = 1; l <= L; ++l) {
        args.pl.half_in[l] = wide ? (wide & 1) : 0;
        args.pl.ks32[l] = wide ? wide / 2 : (m.t_out[l] + 1) / 2;
    }
    for (int l = 1; l < L; ++l) {
        args.pl.off16[l] = off16;
        off16 += m.t_out[l + 1] * (args.pl.ks32[l] * nparts * 512 + args.pl.half_in[l] * nparts * 256);
    }
    for (int l = 1; l <= L; ++l) {
        lay.exact = lay.exact && m.t_out[l] == lay.T;
        if (m.ks_in[l] != lay.nrl) lay.nrl = 0;
    }
    if (pad && !lay.exact && !wide && tmax <= 4 && tmax >= pad_min) {
        lay.T = 4; lay.exact = 1; lay.nrl = 0;
        for (int l = 1; l <= L; ++l) { m.t_out[l] = 4; args.pl.ks32[l] = 2; }
        off16 = 0;
        for (int l = 1; l < L; ++l) { args.pl.off16[l] = off16; off16 += 4 * 2 * nparts * 512; }
    }
    fwd_close_images(args, off16);
    return lay;
}

}  // namespace UMNN_FWD_NS
