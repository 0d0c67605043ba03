// Multi-output Clenshaw-Curtis quadrature: K = 2..16 monotone integrands f_k(t; h) that share every hidden layer of one MLP,
// integrated (and differentiated) in one launch.
//
//   F[q][k] = (x_q - x0_q)/2 * sum_j w_j f_k(t_j; h_q),   f_x[q][k] = f_k(x_q; h_q),   f_x0[q][k] = f_k(x0_q; h_q)
//
// The single-output kernels (cc_forward.hip, cc_backward.hip) end every node in a per-lane dot product and a reduction over the
// four lane groups.  Here the output layer is one more 16-row MFMA tile: rows fout_of(0, rho) < K of its image hold W_L, the bias
// sits in the column of the constant-one feature H_L, rows >= K are zero.  Lane (g, p), component r of that tile's accumulator
// holds output k = 4r + g of integral p -- the numbering every hidden tile has (feat_of(0, r, g)) -- so the hidden layers, nearly
// all of the work, run once for the K outputs.
//
// Exact fp32 on v_mfma_f32_16x16x4_f32 whatever the process-wide precision options say; fp32 storage only.  Every net is
// zero-padded (virtually: tile and K-step counts only, like cc_bwd_plan.h pad_to_exact_family) to one of the shape-exact families
// of kMultiFamilies, so the kernels carry no runtime tile counts.  A padded unit has zero weights and bias: z = 0, act(0) = 0, and
// it contributes exact zeros to every sum.
//
// Inverse (umnn_cc_solve_multi, cc_solve_multi_kernel): the forward's node loop inside the Newton iteration of umnn_cc_solve, for
// x with sum_k coef_k int_0^x f_k = target; see the kernel.
//
// Backward (the reference's gradient convention, ParallelNeuralIntegral.py:66-94,110-123, summed over the K outputs): persistent
// waves, the forward chain recomputed per node keeping sign bits, delta through W^T on MFMA, dW_l += delta_{l+1} (x) a_l through a
// wave-private LDS transpose, dc = sum_j delta_1 to the finishing kernels (d_h, dW_1[:, 1:], db_1), per-wave d_theta slices summed
// by a last kernel in a fixed order: no float atomics, two runs are bit-identical.  New at the output layer: dout_k =
// g_k (x - x0)/2 w_j out'(s_k) (times -1/f_k^2 under inv_f), delta_L = act'(z_L) * W_L^T dout (four K-steps against the
// transposed output image), dW_L / db_L += dout (x) [a_L, 1] through the same LDS trip.  With a cotangent g_fx of f_x
// (umnn_cc_backward_multi_fx, the FX builds of the passes) dout at node x gains g_fx,k out'(s_k) and dx the term
// sum_k g_fx,k df_k/dx, taken from the delta_1 of one more walk of node x in the EDGE pass (see cc_bwd_multi_kernel).
//
// Shared with cc_bwd_kernel (cc_backward.hip), in cc_bwd_shared.h: the row-major image staging, perm16, sign_bits / act_grad_bits
// (the kink convention), the theta offsets and the launch bracket of a pass; d_h is cc_backward.hip's cc_bwd_dh_kernel
// (umnn_launch_bwd_dh).  Still a copy of cc_bwd_kernel's text, to be changed in both files together: the first-layer hoist, the
// K-step loops of a layer, parking a tile in the transpose scratch with the dW accumulation, and the d_theta slice write -- as
// shared helpers they re-scheduled the node loop (profiles/multi_shared/).  Own to this file: the output tile and its dW_L, the
// x-column in LDS, the pass plan, and the simple dW_1 / reduction kernels (their sums run in another order than
// cc_backward.hip's, and their workspace layout is this file's).
#include <cstring>

#include "cc_bwd_shared.h"

struct MultiFamily { int T, KS; };
// (T tiles, KS K-steps per hidden layer): the smallest that holds the widest hidden layer (H + 1 features with the constant one)
static const MultiFamily kMultiFamilies[] = {{2, 8}, {4, 13}, {4, 16}, {7, 26}, {8, 32}};

struct MultiArgs {
    MlpDev m;                       // padded to the family; width[] stays the net's own
    const float* x0;                // nullable
    const float* x;
    const float* h;
    const float* g;                 // backward: [NI][K]
    const float* gfx;               // backward: cotangent of f_x, [NI][K]; nullable (FX variants only)
    const float* ccw;
    const float* ccs;
    float* F;                       // forward outputs [NI][K]; fx, fx0 nullable
    float* fx;
    float* fx0;
    float* dx0;                     // backward outputs [NI]; nullable
    float* dx;
    float* dc;                      // [NI][H1]
    float* partials;                // [nwaves][n_params]
    long long NI;
    int d, E, n, inv_f, K;
    unsigned ngroups;               // forward: groups of 16 P integrals; backward: tiles of 16
    int out_off;                    // forward: float offset of the output image behind the hidden images
    int ld[UMNN_MAX_LINEAR + 1];    // backward: row stride of the row-major image l (l = L: the output image)
    int roff[UMNN_MAX_LINEAR + 1];  // ... and its float offset in LDS
    int poffW[UMNN_MAX_LINEAR];     // offsets of W_l / b_l in the flat theta vector
    int poffb[UMNN_MAX_LINEAR];
    int w1x_off;                    // backward: float offset of the first layer's x-column, [16 T] in feature order
    int scratch_off, scratch_per_wave, l_lo, n_params;
    int outw;                       // backward: this pass accumulates the output layer's dW_L / db_L (OUTW variants only)
    const float* cot;               // backward, NC variants only: the cotangent of f_k at every node, [NI][n + 1][K], node 0 is x
};

// ------------------------------------------------------------------------------------------ forward
template <int TMAX, int KSC, int P>
__global__ __launch_bounds__(UMNN_BLOCK) void cc_fwd_multi_kernel(const MultiArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MlpDev& m = a.m;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, p = lane & 15;
    const int L = m.n_linear - 1;
    const int H1 = m.width[1], HL = m.width[L], K = a.K;
    const int E = a.E, d = a.d, n = a.n;
    const float slope = m.hidden_act == UMNN_ACT_RELU ? 0.f : 0.01f;

    stage_hidden_images(m, lds, tid, UMNN_BLOCK);
    {   // the output tile: one output tile of KSC K-steps, lane layout of every other image
        float* img = lds + a.out_off;
        const float* __restrict__ WL = m.W[L];
        const float* __restrict__ bL = m.b[L];
        for (int idx = tid; idx < KSC * 64; idx += UMNN_BLOCK) {
            const int ln = idx & 63, s = idx >> 6;
            const int k = fout_of(0, ln & 15), fi = 4 * s + (ln >> 4);
            float v = 0.f;
            if (k < K) {
                if (fi < HL) v = WL[k * HL + fi];
                else if (fi == HL) v = bL[k];
            }
            img[idx] = v;
        }
    }
    __syncthreads();

    const unsigned grp = xcd_remap(blockIdx.x, gridDim.x) * UMNN_WAVES_PER_BLOCK + wid;
    if (grp >= a.ngroups) return;

    float xv[P], x0v[P], dxv[P];
    bool ok[P];
    long long qv[P];
    IoView hb[P];
#pragma unroll
    for (int pt = 0; pt < P; ++pt) {
        const long long q = ((long long)grp * P + pt) * 16 + p;
        ok[pt] = q < a.NI;
        const long long qq = ok[pt] ? q : a.NI - 1;
        qv[pt] = qq;
        xv[pt] = a.x[qq];
        x0v[pt] = a.x0 ? a.x0[qq] : 0.f;
        dxv[pt] = xv[pt] - x0v[pt];
        const long long bi = qq / d;
        hb[pt] = IoView{a.h, 0} + (bi * ((long long)E * d) + (qq - bi * d));
    }

    // ---- per-lane constants: first-layer x-column
    float w1x[TMAX][4];
    {
        const float* __restrict__ W0 = m.W[0];
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = feat_of(t, r, g);
                w1x[t][r] = f < H1 ? W0[f * (1 + E)] : 0.f;
            }
    }

    // ---- hoisted first-layer term c = W1[:,1:] h + b1 (and the constant-one feature), on MFMA
    f32x4 c[P][TMAX];
    {
        const float* __restrict__ W0 = m.W[0];
        const float* __restrict__ b0 = m.b[0];
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            f32x4 init;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = feat_of(t, r, g);
                init[r] = f < H1 ? b0[f] : (f == H1 ? 1.f : 0.f);
            }
#pragma unroll
            for (int pt = 0; pt < P; ++pt) c[pt][t] = init;
        }
        for (int se = 0; se < (E + 3) / 4; ++se) {
            const int e = 4 * se + g;
            float hv[P];
#pragma unroll
            for (int pt = 0; pt < P; ++pt) hv[pt] = e < E ? hb[pt][(long long)e * d] : 0.f;
#pragma unroll
            for (int t = 0; t < TMAX; ++t) {
                const int fo = fout_of(t, p);
                const float A = (fo < H1 && e < E) ? W0[fo * (1 + E) + 1 + e] : 0.f;
#pragma unroll
                for (int pt = 0; pt < P; ++pt) c[pt][t] = mfma16(A, hv[pt], c[pt][t]);
            }
        }
    }

    f32x4 Facc[P], fxv[P], fx0v[P];
#pragma unroll
    for (int pt = 0; pt < P; ++pt) Facc[pt] = fxv[pt] = fx0v[pt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- walk the quadrature nodes
    const float* oimg = lds + a.out_off + lane;
    for (int k = 0; k <= n; ++k) {
        const float u = a.ccs[k] + 1.f;
        const float wk = a.ccw[k];
        f32x4 act[P][TMAX];
#pragma unroll
        for (int pt = 0; pt < P; ++pt) {
            // t_k = x0 + (x-x0)*(s_k+1)/2 in the reference's rounding order; node 0 is x itself
            const float tk = k == 0 ? xv[pt] : __fadd_rn(x0v[pt], __fmul_rn(dxv[pt], u) * 0.5f);
#pragma unroll
            for (int t = 0; t < TMAX; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) act[pt][t][r] = hidden_act_f(fmaf(w1x[t][r], tk, c[pt][t][r]), slope);
        }
        for (int l = 1; l < L; ++l) {
            const float* img = lds + m.lds_off[l] + lane;
            f32x4 acc[P][TMAX];
#pragma unroll
            for (int pt = 0; pt < P; ++pt)
#pragma unroll
                for (int t = 0; t < TMAX; ++t) acc[pt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KSC; ++s)
#pragma unroll
                for (int t = 0; t < TMAX; ++t) {
                    const float A = img[(t * KSC + s) * 64];
#pragma unroll
                    for (int pt = 0; pt < P; ++pt) acc[pt][t] = mfma16(A, act[pt][s >> 2][s & 3], acc[pt][t]);
                }
#pragma unroll
            for (int pt = 0; pt < P; ++pt)
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) act[pt][t][r] = hidden_act_f(acc[pt][t][r], slope);
        }
        // the output tile: component r of lane (g, p) = s_k of output k = 4r + g
        f32x4 o[P];
#pragma unroll
        for (int pt = 0; pt < P; ++pt) o[pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KSC; ++s) {
            const float A = oimg[s * 64];
#pragma unroll
            for (int pt = 0; pt < P; ++pt) o[pt] = mfma16(A, act[pt][s >> 2][s & 3], o[pt]);
        }
#pragma unroll
        for (int pt = 0; pt < P; ++pt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float f = out_act_f(o[pt][r], m.out_act);
                Facc[pt][r] = fmaf(wk, maybe_inverse(f, a.inv_f), Facc[pt][r]);
                if (k == 0) fxv[pt][r] = f;
                if (k == n) fx0v[pt][r] = f;
            }
    }

    // ---- [NI][K], k minor: a lane stores the (up to four) outputs it owns
#pragma unroll
    for (int pt = 0; pt < P; ++pt) {
        if (!ok[pt]) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 4 * r + g;
            if (k >= K) continue;
            const long long o = qv[pt] * K + k;
            a.F[o] = Facc[pt][r] * dxv[pt] * 0.5f;
            if (a.fx) a.fx[o] = fxv[pt][r];
            if (a.fx0) a.fx0[o] = fx0v[pt][r];
        }
    }
}

// cc_fwd_multi_kernel that also stores every node's f_k(t_j; h) to f_nodes[NI][n + 1][K] (node j = 0 is x, j = n is x0; k minor,
// masked k < K, tail rows masked): what cc_cumulate_kernel (cc_cumulate.hip) turns into the whole curve.  A sibling, and a copy of
// that kernel's text to be changed together with it, for the reason the header gives: as one body inlined into both kernels the
// forward's register counts moved (profiles/curve/README.md).  f_nodes is an argument of its own, so that MultiArgs -- the kernel
// argument of every other kernel of this file -- stays as it is.  (umnn_cc_forward_multi_nodes passes no inv_f, f_x or f_x0; the two texts differ in the store alone.)
template <int TMAX, int KSC, int P>
__global__ __launch_bounds__(UMNN_BLOCK) void cc_fwd_multi_nodes_kernel(const MultiArgs a, float* __restrict__ f_nodes) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MlpDev& m = a.m;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, p = lane & 15;
    const int L = m.n_linear - 1;
    const int H1 = m.width[1], HL = m.width[L], K = a.K;
    const int E = a.E, d = a.d, n = a.n;
    const float slope = m.hidden_act == UMNN_ACT_RELU ? 0.f : 0.01f;

    stage_hidden_images(m, lds, tid, UMNN_BLOCK);
    {   // the output tile: one output tile of KSC K-steps, lane layout of every other image
        float* img = lds + a.out_off;
        const float* __restrict__ WL = m.W[L];
        const float* __restrict__ bL = m.b[L];
        for (int idx = tid; idx < KSC * 64; idx += UMNN_BLOCK) {
            const int ln = idx & 63, s = idx >> 6;
            const int k = fout_of(0, ln & 15), fi = 4 * s + (ln >> 4);
            float v = 0.f;
            if (k < K) {
                if (fi < HL) v = WL[k * HL + fi];
                else if (fi == HL) v = bL[k];
            }
            img[idx] = v;
        }
    }
    __syncthreads();

    const unsigned grp = xcd_remap(blockIdx.x, gridDim.x) * UMNN_WAVES_PER_BLOCK + wid;
    if (grp >= a.ngroups) return;

    float xv[P], x0v[P], dxv[P];
    bool ok[P];
    long long qv[P];
    IoView hb[P];
#pragma unroll
    for (int pt = 0; pt < P; ++pt) {
        const long long q = ((long long)grp * P + pt) * 16 + p;
        ok[pt] = q < a.NI;
        const long long qq = ok[pt] ? q : a.NI - 1;
        qv[pt] = qq;
        xv[pt] = a.x[qq];
        x0v[pt] = a.x0 ? a.x0[qq] : 0.f;
        dxv[pt] = xv[pt] - x0v[pt];
        const long long bi = qq / d;
        hb[pt] = IoView{a.h, 0} + (bi * ((long long)E * d) + (qq - bi * d));
    }

    // ---- per-lane constants: first-layer x-column
    float w1x[TMAX][4];
    {
        const float* __restrict__ W0 = m.W[0];
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = feat_of(t, r, g);
                w1x[t][r] = f < H1 ? W0[f * (1 + E)] : 0.f;
            }
    }

    // ---- hoisted first-layer term c = W1[:,1:] h + b1 (and the constant-one feature), on MFMA
    f32x4 c[P][TMAX];
    {
        const float* __restrict__ W0 = m.W[0];
        const float* __restrict__ b0 = m.b[0];
#pragma unroll
        for (int t = 0; t < TMAX; ++t) {
            f32x4 init;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = feat_of(t, r, g);
                init[r] = f < H1 ? b0[f] : (f == H1 ? 1.f : 0.f);
            }
#pragma unroll
            for (int pt = 0; pt < P; ++pt) c[pt][t] = init;
        }
        for (int se = 0; se < (E + 3) / 4; ++se) {
            const int e = 4 * se + g;
            float hv[P];
#pragma unroll
            for (int pt = 0; pt < P; ++pt) hv[pt] = e < E ? hb[pt][(long long)e * d] : 0.f;
#pragma unroll
            for (int t = 0; t < TMAX; ++t) {
                const int fo = fout_of(t, p);
                const float A = (fo < H1 && e < E) ? W0[fo * (1 + E) + 1 + e] : 0.f;
#pragma unroll
                for (int pt = 0; pt < P; ++pt) c[pt][t] = mfma16(A, hv[pt], c[pt][t]);
            }
        }
    }

    f32x4 Facc[P], fxv[P], fx0v[P];
#pragma unroll
    for (int pt = 0; pt < P; ++pt) Facc[pt] = fxv[pt] = fx0v[pt] = f32x4{0.f, 0.f, 0.f, 0.f};

    // ---- walk the quadrature nodes
    const float* oimg = lds + a.out_off + lane;
    for (int k = 0; k <= n; ++k) {
        const float u = a.ccs[k] + 1.f;
        const float wk = a.ccw[k];
        f32x4 act[P][TMAX];
#pragma unroll
        for (int pt = 0; pt < P; ++pt) {
            // t_k = x0 + (x-x0)*(s_k+1)/2 in the reference's rounding order; node 0 is x itself
            const float tk = k == 0 ? xv[pt] : __fadd_rn(x0v[pt], __fmul_rn(dxv[pt], u) * 0.5f);
#pragma unroll
            for (int t = 0; t < TMAX; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) act[pt][t][r] = hidden_act_f(fmaf(w1x[t][r], tk, c[pt][t][r]), slope);
        }
        for (int l = 1; l < L; ++l) {
            const float* img = lds + m.lds_off[l] + lane;
            f32x4 acc[P][TMAX];
#pragma unroll
            for (int pt = 0; pt < P; ++pt)
#pragma unroll
                for (int t = 0; t < TMAX; ++t) acc[pt][t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KSC; ++s)
#pragma unroll
                for (int t = 0; t < TMAX; ++t) {
                    const float A = img[(t * KSC + s) * 64];
#pragma unroll
                    for (int pt = 0; pt < P; ++pt) acc[pt][t] = mfma16(A, act[pt][s >> 2][s & 3], acc[pt][t]);
                }
#pragma unroll
            for (int pt = 0; pt < P; ++pt)
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) act[pt][t][r] = hidden_act_f(acc[pt][t][r], slope);
        }
        // the output tile: component r of lane (g, p) = s_k of output k = 4r + g
        f32x4 o[P];
#pragma unroll
        for (int pt = 0; pt < P; ++pt) o[pt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int s = 0; s < KSC; ++s) {
            const float A = oimg[s * 64];
#pragma unroll
            for (int pt = 0; pt < P; ++pt) o[pt] = mfma16(A, act[pt][s >> 2][s & 3], o[pt]);
        }
#pragma unroll
        for (int pt = 0; pt < P; ++pt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float f = out_act_f(o[pt][r], m.out_act);
                Facc[pt][r] = fmaf(wk, maybe_inverse(f, a.inv_f), Facc[pt][r]);
                if (k == 0) fxv[pt][r] = f;
                if (k == n) fx0v[pt][r] = f;
                {
                    const int ko = 4 * r + g;
                    if (ok[pt] && ko < K) f_nodes[(qv[pt] * (n + 1) + k) * K + ko] = f;
                }
            }
    }

    // ---- [NI][K], k minor: a lane stores the (up to four) outputs it owns
#pragma unroll
    for (int pt = 0; pt < P; ++pt) {
        if (!ok[pt]) continue;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = 4 * r + g;
            if (k >= K) continue;
            const long long o = qv[pt] * K + k;
            a.F[o] = Facc[pt][r] * dxv[pt] * 0.5f;
            if (a.fx) a.fx[o] = fxv[pt][r];
            if (a.fx0) a.fx0[o] = fx0v[pt][r];
        }
    }
}

// ------------------------------------------------------------------------------------------ Newton solve of a weighted sum
// sum_k coef[b][k] int_0^{x_b} f_k(t; h_b) dt = target[b] for x_b in [lo, hi] (umnn_cc_solve_multi; d = 1): cc_fwd_multi_kernel's
// node loop with x0 = 0, dxv = x and P = 1 -- one 16-row tile per wave -- inside the iteration of umnn_cc_solve (the INV = 2 block
// of cc_fwd_bf16_kernel.h, word for word).  The staging and the hoisted first-layer term depend on the weights and h only and run
// once per launch.  After the node loop a lane holds F_k and f_k(x) of the outputs k = 4r + g it owns; S = sum_k coef_k F_k and
// D = sum_k coef_k f_k are a four-term fmaf chain per lane (coefficient 0 for k >= K: the padded outputs are finite and add exact
// zeros) and a butterfly over the four lane groups (xor 16, 32).  fp32 addition is commutative, so all four copies of a row end
// with the same bits, take the same step and cast the same vote.  A non-finite F_k makes S non-finite under a zero coefficient as
// well (0 * inf is a NaN): such a row ends UMNN_SOLVE_NONFINITE.

// the output tile as cc_fwd_multi_kernel stages it (a copy of its text: as a helper shared with the forward it moved that kernel's
// scalar register counts)
template <int KSC>
__device__ __forceinline__ void stage_output_tile(const MlpDev& m, float* img, int K, int tid) {
    const int L = m.n_linear - 1, HL = m.width[L];
    const float* __restrict__ WL = m.W[L];
    const float* __restrict__ bL = m.b[L];
    for (int idx = tid; idx < KSC * 64; idx += UMNN_BLOCK) {
        const int ln = idx & 63, s = idx >> 6;
        const int k = fout_of(0, ln & 15), fi = 4 * s + (ln >> 4);
        float v = 0.f;
        if (k < K) {
            if (fi < HL) v = WL[k * HL + fi];
            else if (fi == HL) v = bL[k];
        }
        img[idx] = v;
    }
}

struct SolveMultiArgs {
    MultiArgs a;                    // m, h, ccw, ccs, F (nullable here), fx (nullable), NI, E, n, K, ngroups, out_off
    const float* target;            // [NI]
    const float* coef;              // [NI][K]
    float* x;                       // [NI]
    int* status;                    // [NI], nullable
    float lo, hi, tol;
    int max_iter;
};

template <int TMAX, int KSC>
__global__ __launch_bounds__(UMNN_BLOCK) void cc_solve_multi_kernel(const SolveMultiArgs sa) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MultiArgs& a = sa.a;
    const MlpDev& m = a.m;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, p = lane & 15;
    const int L = m.n_linear - 1;
    const int H1 = m.width[1], K = a.K;
    const int E = a.E, n = a.n;
    const float slope = m.hidden_act == UMNN_ACT_RELU ? 0.f : 0.01f;

    stage_hidden_images(m, lds, tid, UMNN_BLOCK);
    stage_output_tile<KSC>(m, lds + a.out_off, K, tid);
    __syncthreads();

    const unsigned grp = xcd_remap(blockIdx.x, gridDim.x) * UMNN_WAVES_PER_BLOCK + wid;
    if (grp >= a.ngroups) return;

    // lane p's row; lanes beyond the batch mirror the last row, never run and store nothing
    const long long q = (long long)grp * 16 + p;
    const bool ok = q < a.NI;
    const long long qq = ok ? q : a.NI - 1;
    const IoView hb = IoView{a.h, 0} + qq * (long long)E;
    const float target = sa.target[qq];
    f32x4 cf;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = 4 * r + g;
        cf[r] = k < K ? sa.coef[qq * K + k] : 0.f;
    }

    // ---- per-lane constants: first-layer x-column
    float w1x[TMAX][4];
    {
        const float* __restrict__ W0 = m.W[0];
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = feat_of(t, r, g);
                w1x[t][r] = f < H1 ? W0[f * (1 + E)] : 0.f;
            }
    }

    // ---- hoisted first-layer term c = W1[:,1:] h + b1 (and the constant-one feature), on MFMA: once for all iterations
    f32x4 c[TMAX];
    {
        const float* __restrict__ W0 = m.W[0];
        const float* __restrict__ b0 = m.b[0];
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int f = feat_of(t, r, g);
                c[t][r] = f < H1 ? b0[f] : (f == H1 ? 1.f : 0.f);
            }
        for (int se = 0; se < (E + 3) / 4; ++se) {
            const int e = 4 * se + g;
            const float hv = e < E ? hb[(long long)e] : 0.f;
#pragma unroll
            for (int t = 0; t < TMAX; ++t) {
                const int fo = fout_of(t, p);
                const float A = (fo < H1 && e < E) ? W0[fo * (1 + E) + 1 + e] : 0.f;
                c[t] = mfma16(A, hv, c[t]);
            }
        }
    }

    // ---- Newton state: lane p's row; every lane group g holds the same values
    float sv_a = sa.lo, sv_b = sa.hi;
    float sv_x = fminf(fmaxf(0.f, sa.lo), sa.hi);
    bool sv_done = !ok, sv_aopen = true, sv_bopen = true, sv_bad = false;
    int sv_stat = 0;
    f32x4 Fout = f32x4{0.f, 0.f, 0.f, 0.f}, fout = f32x4{0.f, 0.f, 0.f, 0.f};      // F_k, f_k at the row's last evaluated x

    const float* oimg = lds + a.out_off + lane;
    const int rounds = sa.max_iter;
    for (int round = 0; round < rounds; ++round) {
        const float xv = sv_x;
        f32x4 Facc = f32x4{0.f, 0.f, 0.f, 0.f}, fxv = f32x4{0.f, 0.f, 0.f, 0.f};
        // ---- walk the quadrature nodes (cc_fwd_multi_kernel: x0 = 0, dxv = x)
        for (int k = 0; k <= n; ++k) {
            const float u = a.ccs[k] + 1.f;
            const float wk = a.ccw[k];
            const float tk = k == 0 ? xv : __fadd_rn(0.f, __fmul_rn(xv, u) * 0.5f);
            f32x4 act[TMAX];
#pragma unroll
            for (int t = 0; t < TMAX; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) act[t][r] = hidden_act_f(fmaf(w1x[t][r], tk, c[t][r]), slope);
            for (int l = 1; l < L; ++l) {
                const float* img = lds + m.lds_off[l] + lane;
                f32x4 acc[TMAX];
#pragma unroll
                for (int t = 0; t < TMAX; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KSC; ++s)
#pragma unroll
                    for (int t = 0; t < TMAX; ++t) acc[t] = mfma16(img[(t * KSC + s) * 64], act[s >> 2][s & 3], acc[t]);
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) act[t][r] = hidden_act_f(acc[t][r], slope);
            }
            // the output tile: component r of lane (g, p) = s_k of output k = 4r + g
            f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KSC; ++s) o = mfma16(oimg[s * 64], act[s >> 2][s & 3], o);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float f = out_act_f(o[r], m.out_act);
                Facc[r] = fmaf(wk, f, Facc[r]);
                if (k == 0) fxv[r] = f;
            }
        }
        // ---- S = sum_k coef_k F_k, D = sum_k coef_k f_k: the same bits in all four lane groups
        f32x4 Fk;
        float S = 0.f, D = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            Fk[r] = Facc[r] * xv * 0.5f;
            S = fmaf(cf[r], Fk[r], S);
            D = fmaf(cf[r], fxv[r], D);
        }
        S += __shfl_xor(S, 16); D += __shfl_xor(D, 16);
        S += __shfl_xor(S, 32); D += __shfl_xor(D, 32);

        if (!sv_done) {
            ++sv_stat;
            Fout = Fk; fout = fxv;
            const float r = S - target;
            if (!(__builtin_fabsf(S) < __builtin_inff()) || r != r) {
                sv_bad = true; sv_done = true;                   // a NaN in the target, the embedding or the coefficients; a non-finite F_k
            } else if (fabsf(r) <= sa.tol * fmaxf(1.f, fabsf(target)) && fabsf(r) < __builtin_inff()) {   // (no x meets an infinite target: the bound is infinite too)
                sv_done = true;
            } else {
                if (r > 0.f) {
                    if (sv_x <= sa.lo) { sv_stat |= UMNN_SOLVE_CLAMPED; sv_done = true; }      // target below G(lo)
                    sv_b = sv_x; sv_bopen = false;
                } else {
                    if (sv_x >= sa.hi) { sv_stat |= UMNN_SOLVE_CLAMPED; sv_done = true; }      // target above G(hi)
                    sv_a = sv_x; sv_aopen = false;
                }
                if (!sv_done) {
                    float xn = sv_x - r / D;
                    if (!(xn > sv_a && xn < sv_b)) {
                        if (xn >= sv_b && sv_bopen) { xn = sv_b; sv_bopen = false; }       // overshot an endpoint not yet evaluated: try it
                        else if (xn <= sv_a && sv_aopen) { xn = sv_a; sv_aopen = false; }
                        else {
                            xn = 0.5f * (sv_a + sv_b);
                            if (!(xn > sv_a && xn < sv_b)) sv_done = true;                 // bracket collapsed to adjacent floats
                        }
                    }
                    if (!sv_done) {
                        if (xn == sv_x) sv_done = true;                                    // x has stopped changing
                        else if (round + 1 < rounds) sv_x = xn;                            // (the last evaluated point is what leaves)
                    }
                }
            }
        }
        if (__all(sv_done)) break;
    }

    // ---- lane group 0 writes x and status; every lane the (up to four) outputs of F and f_x it owns, as the forward does
    if (!ok) return;
    if (g == 0) {
        if (!sv_done) sv_stat |= UMNN_SOLVE_CAPPED;
        if (sv_bad) sv_stat |= UMNN_SOLVE_NONFINITE;
        sa.x[qq] = sv_bad ? __builtin_nanf("") : sv_x;
        if (sa.status) sa.status[qq] = sv_stat;
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = 4 * r + g;
        if (k >= K) continue;
        if (a.F) a.F[qq * K + k] = Fout[r];
        if (a.fx) a.fx[qq * K + k] = fout[r];
    }
}

// ------------------------------------------------------------------------------------------ backward
__device__ __forceinline__ void stage_multi_rowmajor(const MultiArgs& a, float* lds, int tid, int nthreads, int rows) {
    const MlpDev& m = a.m;
    const int L = m.n_linear - 1;
    // hidden images: the `rows` features the next layer consumes.  Fragment reads of the rows (W^T fragments: columns) beyond
    // that run into the following image / the zero-initialised scratch: finite values that only ever reach padding features.
    for (int l = 1; l < L; ++l)
        stage_rowmajor_image(lds + a.roff[l], m.W[l], m.b[l], rows, a.ld[l], m.width[l], m.width[l + 1], true, tid, nthreads);
    // the output image: 16 rows, row k = [W_L[k][:], b_L[k], 0...] for k < K, zero above (no constant-one row: nothing consumes it)
    stage_rowmajor_image(lds + a.roff[L], m.W[L], m.b[L], 16, a.ld[L], m.width[L], a.K, false, tid, nthreads);
}

// NACC: hidden images whose dW this pass accumulates (layers l_lo .. l_lo + NACC - 1).  EDGE: the pass that owns what exists
// once per integral -- dc, dW_1[:, 0] and the Leibniz terms.  OUTW: the pass can hold the output layer's dW_L / db_L (it does when
// a.outw is set): a separate switch, because the seven-tile EDGE pass with one dW layer has no registers left for it.
// FX: the launch has a cotangent g_fx of f_x[q][k] = f_k(x_q; h_q) (a.gfx; f itself, also under inv_f).  Every pass adds
// g_fx out'(s_k) to the output layer's cotangent at node x.  The EDGE pass does it by walking node x once more, last, with that
// cotangent alone -- the ordinary node 0 keeps the quadrature's --, because the delta_1 of that walk is what dx needs:
// sum_k g_fx,k df_k/dx = sum_feature delta_1[feature] W_1[feature, x-column].  No register is held across the node loop for it
// (g_fx is loaded where it is used, dx is written from inside the walk), and the variants without FX are the kernels they were.
// NC: the node-cotangent build (umnn_cc_backward_multi_nodes: the backward of a whole curve).  The cotangent of f_k at node j is an
// input of its own, dout_k = cot[q][j][k] out'(s_k) (a.cot, loaded at the top of the node's iteration so that the forward recompute
// hides the loads; dead lanes and k >= K give 0): no quadrature weight, no g, no inv_f, and never together with FX.  Its EDGE pass
// has no Leibniz terms: a node t_j = x0 + (x - x0) u_j / 2 moves with both limits, so dx = sum_j (u_j / 2) tau_j and dx0 =
// sum_j (1 - u_j / 2) tau_j with tau_j = sum_k cot[j][k] df_k/dt (t_j) = sum_feature delta_1[feature] W_1[feature, x-column], the
// dot product of the FX build's extra walk, here at every node into two per-lane scalars that are reduced once after the loop.
// The variants without NC are the kernels they were.
template <int TMAX, int KSC, int NACC, bool EDGE, bool OUTW, bool FX, bool NC = false>
__global__ __launch_bounds__(UMNN_BLOCK, 1) void cc_bwd_multi_kernel(const MultiArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MlpDev& m = a.m;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, p = lane & 15;
    const int L = m.n_linear - 1;
    const int H1 = m.width[1], HL = m.width[L], K = a.K;
    const int E = a.E, d = a.d, n = a.n;
    const float slope = m.hidden_act == UMNN_ACT_RELU ? 0.f : 0.01f;
    constexpr int NA = NACC > 0 ? NACC : 1;

    const int nwb = blockDim.x >> 6;
    stage_multi_rowmajor(a, lds, tid, blockDim.x, 4 * KSC);
    for (int f = tid; f < 16 * TMAX; f += blockDim.x) lds[a.w1x_off + f] = f < H1 ? m.W[0][f * (1 + E)] : 0.f;
    for (int i = tid; i < nwb * a.scratch_per_wave; i += blockDim.x) lds[a.scratch_off + i] = 0.f;
    __syncthreads();

    // wave-private: [NACC a-tiles | 1 tile: a_L, then the deltas | the 16 x 16 tile of dout]
    float* scratch = lds + a.scratch_off + wid * a.scratch_per_wave;
    float* s_delta = scratch + NACC * (TMAX * 256);
    float* s_dout = s_delta + TMAX * 256;
    const int wr_off = g * 16 + p;                 // + (16t+4r)*16 : standard-layout write [feature][point]
    const int rd_off = (lane & 15) * 16 + 4 * g;   // + 16t*16      : transposed b128 read (feature on lane&15, points 4g..4g+3)

    const float* w1x = lds + a.w1x_off + g;        // first-layer x-column of feature 16t + 4r + g: read per node, not held
    const bool outw = OUTW && a.outw;
    const int ldO = a.ld[L];
    const float* oimg_f = lds + a.roff[L] + perm16(p) * ldO + g;       // forward fragments of the output image
    const float* oimg_b = lds + a.roff[L] + g * ldO + perm16(p);       // W_L^T fragments

    f32x4 dW[NA][TMAX][TMAX];
#pragma unroll
    for (int j = 0; j < NA; ++j)
#pragma unroll
        for (int to = 0; to < TMAX; ++to)
#pragma unroll
            for (int ti = 0; ti < TMAX; ++ti) dW[j][to][ti] = f32x4{0.f, 0.f, 0.f, 0.f};
    f32x4 dW1x[TMAX], dWo[TMAX];
#pragma unroll
    for (int t = 0; t < TMAX; ++t) { dW1x[t] = f32x4{0.f, 0.f, 0.f, 0.f}; dWo[t] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    const unsigned wave_global = blockIdx.x * nwb + wid;
    const unsigned nwaves = gridDim.x * nwb;

    for (unsigned grp = wave_global; grp < a.ngroups; grp += nwaves) {
        const long long q = (long long)grp * 16 + p;
        const bool ok = q < a.NI;
        const long long qq = ok ? q : a.NI - 1;
        const float xv = a.x[qq];
        const float x0v = a.x0 ? a.x0[qq] : 0.f;
        const float dxv = xv - x0v;
        f32x4 gv, cotbase;                             // dead lanes and outputs k >= K contribute nothing
        if (!NC) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * r + g;
                gv[r] = (ok && k < K) ? a.g[qq * K + k] : 0.f;
                cotbase[r] = gv[r] * dxv * 0.5f;
            }
        }
        const float* __restrict__ cotq = NC ? a.cot + qq * ((long long)(n + 1) * K) : nullptr;
        float taux = 0.f, taux0 = 0.f;                 // NC && EDGE: sum_j (u_j / 2) tau_j and sum_j (1 - u_j / 2) tau_j, this lane's part
        const long long bi = qq / d;
        const IoView hb = IoView{a.h, 0} + (bi * ((long long)E * d) + (qq - bi * d));

        f32x4 c[TMAX];
        {
            const float* __restrict__ W0 = m.W[0];
            const float* __restrict__ b0 = m.b[0];
#pragma unroll
            for (int t = 0; t < TMAX; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int f = feat_of(t, r, g);
                    c[t][r] = f < H1 ? b0[f] : (f == H1 ? 1.f : 0.f);
                }
            for (int se = 0; se < (E + 3) / 4; ++se) {
                const int e = 4 * se + g;
                const float hv = e < E ? hb[(long long)e * d] : 0.f;
#pragma unroll
                for (int t = 0; t < TMAX; ++t) {
                    const int fo = fout_of(t, p);
                    const float A = (fo < H1 && e < E) ? W0[fo * (1 + E) + 1 + e] : 0.f;
                    c[t] = mfma16(A, hv, c[t]);
                }
            }
        }

        f32x4 dcs[TMAX];
#pragma unroll
        for (int t = 0; t < TMAX; ++t) dcs[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 fxv = f32x4{0.f, 0.f, 0.f, 0.f}, fx0v = f32x4{0.f, 0.f, 0.f, 0.f};

        const int klast = (FX && EDGE) ? n + 1 : n;                       // EDGE with g_fx: node x once more
        for (int k = 0; k <= klast; ++k) {
            const bool xtra = FX && EDGE && k > n;
            const int kn = xtra ? 0 : k;
            const float u = a.ccs[kn] + 1.f;
            const float wk = NC ? 0.f : a.ccw[kn];
            f32x4 cotv;
            if (NC) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int ko = 4 * r + g;
                    cotv[r] = (ok && ko < K) ? cotq[k * K + ko] : 0.f;
                }
            }
            const float tk = kn == 0 ? xv : __fadd_rn(x0v, __fmul_rn(dxv, u) * 0.5f);
            unsigned bits[UMNN_MAX_LINEAR];          // bits[l]: sign bits of hidden layer l's activation
            f32x4 act[TMAX];
            // ---------------- forward recompute ----------------
#pragma unroll
            for (int t = 0; t < TMAX; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) act[t][r] = hidden_act_f(fmaf(w1x[16 * t + 4 * r], tk, c[t][r]), slope);
            bits[1] = sign_bits<TMAX>(act);
            for (int l = 1; l < L; ++l) {
#pragma unroll
                for (int j = 0; j < NACC; ++j)
                    if (l == a.l_lo + j) {
#pragma unroll
                        for (int t = 0; t < TMAX; ++t)
#pragma unroll
                            for (int r = 0; r < 4; ++r) scratch[j * (TMAX * 256) + (16 * t + 4 * r) * 16 + wr_off] = act[t][r];
                    }
                const int LD = a.ld[l];
                const float* wf = lds + a.roff[l] + perm16(p) * LD + g;
                f32x4 acc[TMAX];
#pragma unroll
                for (int t = 0; t < TMAX; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KSC; ++s)
#pragma unroll
                    for (int t = 0; t < TMAX; ++t) acc[t] = mfma16(wf[16 * t * LD + 4 * s], act[s >> 2][s & 3], acc[t]);
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) act[t][r] = hidden_act_f(acc[t][r], slope);
                bits[l + 1] = sign_bits<TMAX>(act);
            }
            // the output tile
            f32x4 o = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KSC; ++s) o = mfma16(oimg_f[4 * s], act[s >> 2][s & 3], o);
            f32x4 dout;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float f = out_act_f(o[r], m.out_act);
                const float fp = out_grad_f(o[r], m.out_act);
                if (k == 0) fxv[r] = f;
                if (k == n) fx0v[r] = f;
                if (NC) {
                    dout[r] = cotv[r] * fp;
                } else {
                    const float invs = a.inv_f ? -__frcp_rn(f * f) : 1.f;
                    dout[r] = cotbase[r] * invs * wk * fp;
                }
                if (FX && (xtra || (!EDGE && k == 0))) {
                    const int ko = 4 * r + g;
                    const float gf = (ok && ko < K) ? a.gfx[qq * K + ko] : 0.f;
                    dout[r] = xtra ? gf * fp : fmaf(gf, fp, dout[r]);
                }
            }

            // ---------------- backward sweep ----------------
            if (outw) {
                // dW_L[k][f] += dout_k a_L[f]  (and db_L through the constant-one feature): contract over the 16 points
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) s_delta[(16 * t + 4 * r) * 16 + wr_off] = act[t][r];
#pragma unroll
                for (int r = 0; r < 4; ++r) s_dout[(4 * r) * 16 + wr_off] = dout[r];
                const f32x4 dT = *reinterpret_cast<const f32x4*>(s_dout + rd_off);
#pragma unroll
                for (int ti = 0; ti < TMAX; ++ti) {
                    const f32x4 aT = *reinterpret_cast<const f32x4*>(s_delta + 16 * ti * 16 + rd_off);
#pragma unroll
                    for (int r = 0; r < 4; ++r) dWo[ti] = mfma16(dT[r], aT[r], dWo[ti]);
                }
            }
            // delta_L = act'(z_L) * W_L^T dout: four K-steps (16 outputs) against the transposed output image
            f32x4 delta[TMAX];
            {
                f32x4 nd[TMAX];
#pragma unroll
                for (int t = 0; t < TMAX; ++t) nd[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < 4; ++s)
#pragma unroll
                    for (int t = 0; t < TMAX; ++t) nd[t] = mfma16(oimg_b[4 * s * ldO + 16 * t], dout[s], nd[t]);
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) delta[t][r] = nd[t][r] * act_grad_bits(bits[L], t, r, slope);
            }
            for (int l = L - 1; l >= 1; --l) {
                // dW_l += delta_{l+1} (x) a_l  (contract over the 16 points through the LDS transpose)
#pragma unroll
                for (int j = 0; j < NACC; ++j)
                    if (l == a.l_lo + j) {
#pragma unroll
                        for (int t = 0; t < TMAX; ++t)
#pragma unroll
                            for (int r = 0; r < 4; ++r) s_delta[(16 * t + 4 * r) * 16 + wr_off] = delta[t][r];
                        f32x4 dT[TMAX], aT[TMAX];
#pragma unroll
                        for (int t = 0; t < TMAX; ++t) {
                            dT[t] = *reinterpret_cast<const f32x4*>(s_delta + 16 * t * 16 + rd_off);
                            aT[t] = *reinterpret_cast<const f32x4*>(scratch + j * (TMAX * 256) + 16 * t * 16 + rd_off);
                        }
#pragma unroll
                        for (int to = 0; to < TMAX; ++to)
#pragma unroll
                            for (int ti = 0; ti < TMAX; ++ti)
#pragma unroll
                                for (int r = 0; r < 4; ++r) dW[j][to][ti] = mfma16(dT[to][r], aT[ti][r], dW[j][to][ti]);
                    }
                // delta_l = (W_l^T delta_{l+1}) * act'(z_l)
                const int LD = a.ld[l];
                const float* wt = lds + a.roff[l] + g * LD + perm16(p);
                f32x4 nd[TMAX];
#pragma unroll
                for (int t = 0; t < TMAX; ++t) nd[t] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int s = 0; s < KSC; ++s)
#pragma unroll
                    for (int t = 0; t < TMAX; ++t) nd[t] = mfma16(wt[4 * s * LD + 16 * t], delta[s >> 2][s & 3], nd[t]);
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) delta[t][r] = nd[t][r] * act_grad_bits(bits[l], t, r, slope);
            }
            if (EDGE) {
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        dcs[t][r] += delta[t][r];
                        dW1x[t][r] = fmaf(delta[t][r], tk, dW1x[t][r]);
                    }
                if (NC) {
                    float tau = 0.f;
#pragma unroll
                    for (int t = 0; t < TMAX; ++t)
#pragma unroll
                        for (int r = 0; r < 4; ++r) tau = fmaf(delta[t][r], w1x[16 * t + 4 * r], tau);
                    const float hu = u * 0.5f;             // (node 0 is x: u = 2; node n is x0: u = 0)
                    taux = fmaf(hu, tau, taux);
                    taux0 = fmaf(1.f - hu, tau, taux0);
                }
            }
            if (xtra) {
                // dx = sum_k g_k f_k(x) + sum_feature delta_1[feature] W_1[feature, x-column]  (delta_1 of g_fx out' alone)
                float sx = 0.f, sfx = 0.f;
#pragma unroll
                for (int r = 0; r < 4; ++r) sx = fmaf(gv[r], fxv[r], sx);
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) sfx = fmaf(delta[t][r], w1x[16 * t + 4 * r], sfx);
                sx = group_allreduce(sx);
                sfx = group_allreduce(sfx);
                if (ok && g == 0 && a.dx) a.dx[q] = sx + sfx;
            }
        }

        if (EDGE) {
            if (ok) {
#pragma unroll
                for (int t = 0; t < TMAX; ++t)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int f = feat_of(t, r, g);
                        if (f < H1) a.dc[q * H1 + f] = dcs[t][r];
                    }
            }
            if (NC) {
                // the limits move the nodes: the tau sums alone (the caller adds what the cotangents of t and of the span give)
                taux = group_allreduce(taux);
                taux0 = group_allreduce(taux0);
                if (ok && g == 0) {
                    if (a.dx) a.dx[q] = taux;
                    if (a.dx0) a.dx0[q] = taux0;
                }
            } else {
            // Leibniz terms (the convention of cc_backward.hip: f itself, also under inv_f), summed over the K outputs
            float sx = 0.f, sx0 = 0.f;
#pragma unroll
            for (int r = 0; r < 4; ++r) { sx = fmaf(gv[r], fxv[r], sx); sx0 = fmaf(gv[r], fx0v[r], sx0); }
            sx = group_allreduce(sx);
            sx0 = group_allreduce(sx0);
            if (ok && g == 0) {
                if (!FX && a.dx) a.dx[q] = sx;
                if (a.dx0) a.dx0[q] = -sx0;
            }
            }
        }
    }

    // ---------------- write this wave's partial d_theta ----------------
    float* part = a.partials + (size_t)wave_global * a.n_params;
#pragma unroll
    for (int j = 0; j < NACC; ++j) {
        const int l = a.l_lo + j;
        if (l < L) {
            const int Hin = m.width[l], Hout = m.width[l + 1];
#pragma unroll
            for (int to = 0; to < TMAX; ++to)
#pragma unroll
                for (int ti = 0; ti < TMAX; ++ti)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int fo = 16 * to + 4 * g + r, fi = 16 * ti + (lane & 15);
                        if (fo < Hout) {
                            if (fi < Hin) part[a.poffW[l] + fo * Hin + fi] = dW[j][to][ti][r];
                            else if (fi == Hin) part[a.poffb[l] + fo] = dW[j][to][ti][r];
                        }
                    }
        }
    }
    if (outw) {
#pragma unroll
        for (int ti = 0; ti < TMAX; ++ti)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = 4 * g + r, fi = 16 * ti + (lane & 15);
                if (k < K) {
                    if (fi < HL) part[a.poffW[L] + k * HL + fi] = dWo[ti][r];
                    else if (fi == HL) part[a.poffb[L] + k] = dWo[ti][r];
                }
            }
    }
    if (EDGE) {
#pragma unroll
        for (int t = 0; t < TMAX; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float v1 = dW1x[t][r];
#pragma unroll
                for (int o = 1; o < 16; o <<= 1) v1 += __shfl_xor(v1, o);
                const int f = feat_of(t, r, g);
                if (p == 0 && f < H1) part[a.poffW[0] + f * (1 + E)] = v1;
            }
    }
}

// ---- finishing kernels (d_h: cc_bwd_dh_kernel of cc_backward.hip, through umnn_launch_bwd_dh) ---------------------------
// p0[blk][f][e] = sum_{q in the block's range} dc[q][f] * hext[q][e],  hext[q][E] = 1   (-> dW_1[:, 1:], db_1).  A block owns
// `per` consecutive integrals and a thread one output at a time; fixed summation order.
__global__ __launch_bounds__(256) void cc_bwd_multi_dw0_kernel(const float* __restrict__ dc, const float* __restrict__ h,
                                                               float* __restrict__ p0, long long NI, int d, int E, int H1,
                                                               long long per) {
    const long long q0 = (long long)blockIdx.x * per;
    const long long q1 = min(q0 + per, NI);
    const int nout = H1 * (E + 1);
    for (int o = threadIdx.x; o < nout; o += 256) {
        const int f = o / (E + 1), e = o - f * (E + 1);
        float s = 0.f;
        for (long long q = q0; q < q1; ++q) {
            const long long bi = q / d;
            const float hv = e < E ? h[bi * ((long long)E * d) + (long long)e * d + (q - bi * d)] : 1.f;
            s = fmaf(dc[q * H1 + f], hv, s);
        }
        p0[(size_t)blockIdx.x * nout + o] = s;
    }
}

// dtheta[i] = sum_w partials[w][i]  (+ the first-layer entries from the dw0 partials), slices in a fixed order
__global__ __launch_bounds__(256) void cc_bwd_multi_reduce_kernel(const float* __restrict__ partials, int nparts, int n_params,
                                                                  const float* __restrict__ p0, int nparts0, int E, int H1,
                                                                  int poffW0, int poffb0, float* __restrict__ dtheta) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_params) return;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int w = 0;
    for (; w + 3 < nparts; w += 4) {
        s0 += partials[(size_t)w * n_params + i];
        s1 += partials[(size_t)(w + 1) * n_params + i];
        s2 += partials[(size_t)(w + 2) * n_params + i];
        s3 += partials[(size_t)(w + 3) * n_params + i];
    }
    for (; w < nparts; ++w) s0 += partials[(size_t)w * n_params + i];
    float s = (s0 + s1) + (s2 + s3);
    int o = -1;
    if (i >= poffW0 && i < poffW0 + H1 * (1 + E)) {
        const int f = (i - poffW0) / (1 + E), col = (i - poffW0) - f * (1 + E);
        if (col >= 1) o = f * (E + 1) + (col - 1);
    } else if (i >= poffb0 && i < poffb0 + H1) {
        o = (i - poffb0) * (E + 1) + E;
    }
    if (o >= 0) {
        const int nout = H1 * (E + 1);
        float t0 = 0.f, t1 = 0.f;
        int w2 = 0;
        for (; w2 + 1 < nparts0; w2 += 2) { t0 += p0[(size_t)w2 * nout + o]; t1 += p0[(size_t)(w2 + 1) * nout + o]; }
        if (w2 < nparts0) t0 += p0[(size_t)w2 * nout + o];
        s += t0 + t1;
    }
    dtheta[i] = s;
}

// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------
typedef void (*multi_kernel_t)(const MultiArgs);

struct MultiFwdVariant { int T, KS, P; multi_kernel_t fn; const char* name; };
#define MULTI_FWD(T, KS, P) { T, KS, P, cc_fwd_multi_kernel<T, KS, P>, "cc_fwd_multi<T=" #T ",KS=" #KS ",P=" #P ">" }
static const MultiFwdVariant kMultiFwd[] = {
    MULTI_FWD(2, 8, 1), MULTI_FWD(2, 8, 2), MULTI_FWD(4, 13, 1), MULTI_FWD(4, 13, 2), MULTI_FWD(4, 16, 1), MULTI_FWD(4, 16, 2),
    MULTI_FWD(7, 26, 1), MULTI_FWD(7, 26, 2), MULTI_FWD(8, 32, 1), MULTI_FWD(8, 32, 2),
};

typedef void (*multi_nodes_kernel_t)(const MultiArgs, float*);
struct MultiNodesVariant { int T, KS, P; multi_nodes_kernel_t fn; const char* name; };
#define MULTI_NODES(T, KS, P) { T, KS, P, cc_fwd_multi_nodes_kernel<T, KS, P>, "cc_fwd_multi_nodes<T=" #T ",KS=" #KS ",P=" #P ">" }
static const MultiNodesVariant kMultiNodes[] = {
    MULTI_NODES(2, 8, 1), MULTI_NODES(2, 8, 2), MULTI_NODES(4, 13, 1), MULTI_NODES(4, 13, 2), MULTI_NODES(4, 16, 1), MULTI_NODES(4, 16, 2),
    MULTI_NODES(7, 26, 1), MULTI_NODES(7, 26, 2), MULTI_NODES(8, 32, 1), MULTI_NODES(8, 32, 2),
};

// the backward passes of a family: the EDGE pass holds `edge_nacc` dW layers, every further pass `rest_nacc`
// fn / name [1]: the FX build of the pass (a g_fx cotangent was given), [2]: the node-cotangent build (NC), [0]: the kernel without either
struct MultiBwdVariant { int T, KS, nacc, edge, outw; multi_kernel_t fn[3]; const char* name[3]; };
#define MULTI_BWD(T, KS, N, E, O) { T, KS, N, E, O, {cc_bwd_multi_kernel<T, KS, N, (E) != 0, (O) != 0, false>, cc_bwd_multi_kernel<T, KS, N, (E) != 0, (O) != 0, true>, \
                                                     cc_bwd_multi_kernel<T, KS, N, (E) != 0, (O) != 0, false, true>}, \
                                    {"cc_bwd_multi<T=" #T ",KS=" #KS ",NACC=" #N ",EDGE=" #E ",OUTW=" #O ">", "cc_bwd_multi<T=" #T ",KS=" #KS ",NACC=" #N ",EDGE=" #E ",OUTW=" #O ",FX=1>", \
                                     "cc_bwd_multi<T=" #T ",KS=" #KS ",NACC=" #N ",EDGE=" #E ",OUTW=" #O ",NC=1>"} }
static const MultiBwdVariant kMultiBwd[] = {
    MULTI_BWD(2, 8, 3, 1, 1), MULTI_BWD(2, 8, 3, 0, 0),
    MULTI_BWD(4, 13, 3, 1, 1), MULTI_BWD(4, 13, 3, 0, 0),
    MULTI_BWD(4, 16, 3, 1, 1), MULTI_BWD(4, 16, 3, 0, 0),
    MULTI_BWD(7, 26, 1, 1, 0), MULTI_BWD(7, 26, 0, 1, 1), MULTI_BWD(7, 26, 1, 0, 1), MULTI_BWD(7, 26, 1, 0, 0),
    MULTI_BWD(8, 32, 0, 1, 1), MULTI_BWD(8, 32, 1, 0, 0),
};
static const MultiBwdVariant* multi_bwd_variant(int T, int KS, int nacc, int edge, int outw) {
    for (const MultiBwdVariant& v : kMultiBwd)
        if (v.T == T && v.KS == KS && v.nacc == nacc && v.edge == edge && v.outw == outw) return &v;
    return nullptr;
}
// The passes of a backward over `nimg` hidden images (L - 1), first the EDGE pass: as few as the register file allows.  Up to four
// tiles a pass holds three dW layers next to everything else; at seven tiles one, and the output layer's dW_L then rides in
// the second pass (nets with at most one hidden image: in an EDGE pass without a dW layer); at eight tiles the EDGE pass holds none.
struct MultiPass { const MultiBwdVariant* v; int l_lo, outw; };
static int multi_passes(int T, int KS, int nimg, bool need_theta, MultiPass* out) {
    int n = 0, l = 1;
    if (T <= 4) {
        out[n++] = {multi_bwd_variant(T, KS, 3, 1, 1), l, need_theta}; l += 3;
        for (; need_theta && l <= nimg; l += 3) out[n++] = {multi_bwd_variant(T, KS, 3, 0, 0), l, 0};
    } else if (T == 7 && nimg >= 2) {
        out[n++] = {multi_bwd_variant(T, KS, 1, 1, 0), l, 0}; l += 1;
        for (; need_theta && l <= nimg; l += 1) out[n++] = {multi_bwd_variant(T, KS, 1, 0, l == 2), l, l == 2};
    } else {
        out[n++] = {multi_bwd_variant(T, KS, 0, 1, 1), l, need_theta};
        for (; need_theta && l <= nimg; l += 1) out[n++] = {multi_bwd_variant(T, KS, 1, 0, 0), l, 0};
    }
    return n;
}

// row stride of a row-major image with `cols` used columns: both fragment patterns -- rows on lane&15 with the K index on the
// lane group, and the transpose -- are (nearly) conflict-free for ds_read_b32 when the stride is 14 or 18 modulo 32
static int multi_ld(int cols) {
    int ld = cols;
    while (ld % 32 != 14 && ld % 32 != 18) ++ld;
    return ld;
}

struct MultiPlan {
    MultiArgs a;
    int T, KS;
    size_t fwd_lds;
    int bwd_ok;        // the backward's images and scratch fit the LDS
    int wpb;           // backward: waves per workgroup (as many of 4, 2, 1 as leave room for the wave-private transpose tiles)
};

static int multi_scratch_per_wave(int T, int nacc) { return (nacc + 1) * T * 256 + 256; }
static size_t multi_bwd_lds(const MultiPlan& pl, int nacc, int waves) {
    return (size_t)(pl.a.scratch_off + waves * multi_scratch_per_wave(pl.T, nacc)) * sizeof(float);
}
static const char* const kMultiBwdLdsError = "multi-output backward: weight images exceed 160 KiB of LDS";

// Validates the net, pads it to its family and fills what both directions share.  K = widths[n_linear] in [min_out, 16]
// (min_out = 1: the node-value entry; the output tile is padded to 16 rows whatever K is).
static int multi_plan(const umnn_mlp* net, int E, MultiPlan* pl, int min_out = 2) {
    MultiArgs& a = pl->a;
    memset(&a, 0, sizeof(a));
    int tmax = 0, ksu = 0;
    if (int rc = umnn_prepare_mlp(net, E, &a.m, &tmax, &ksu, UMNN_MAX_OUTPUTS, min_out)) return rc;
    MlpDev& m = a.m;
    const int L = m.n_linear - 1;
    a.K = m.width[L + 1];
    int ksmax = 0;
    for (int l = 1; l <= L; ++l) ksmax = m.ks_in[l] > ksmax ? m.ks_in[l] : ksmax;
    pl->T = 0;
    for (const MultiFamily& f : kMultiFamilies)
        if (tmax <= f.T && ksmax <= f.KS) { pl->T = f.T; pl->KS = f.KS; break; }
    if (!pl->T) return umnn_fail(UMNN_EUNSUPPORTED, "multi-output: no kernel family for this hidden width");
    int off = 0;
    for (int l = 1; l <= L; ++l) { m.t_out[l] = m.t_mfma[l] = pl->T; m.ks_in[l] = pl->KS; }
    for (int l = 1; l < L; ++l) { m.lds_off[l] = off; off += pl->T * pl->KS * 64; }
    m.lds_off[L] = off;
    a.out_off = off;
    pl->fwd_lds = (size_t)(off + pl->KS * 64) * sizeof(float);
    if (pl->fwd_lds > UMNN_LDS_LIMIT) return umnn_fail(UMNN_EUNSUPPORTED, "multi-output: weight images exceed 160 KiB of LDS");
    // backward: row-major images
    int ro = 0;
    const int cols = 4 * pl->KS;      // (columns 4 KS .. 16 T of a W^T fragment run into the next row: padding features)
    for (int l = 1; l < L; ++l) { a.ld[l] = multi_ld(cols); a.roff[l] = ro; ro += 4 * pl->KS * a.ld[l]; ro = (ro + 3) & ~3; }
    a.ld[L] = multi_ld(cols); a.roff[L] = ro; ro += 16 * a.ld[L]; ro = (ro + 3) & ~3;
    a.w1x_off = ro; ro += 16 * pl->T;
    a.scratch_off = ro;
    a.n_params = bwd_param_offsets(m, a.poffW, a.poffb);
    // every pass writes its entries of the same d_theta slices, so all passes run the same waves: sized for the largest scratch
    const int nacc_max = pl->T <= 4 ? 3 : 1;
    pl->wpb = 4;
    while (pl->wpb > 1 && multi_bwd_lds(*pl, nacc_max, pl->wpb) > UMNN_LDS_LIMIT) pl->wpb >>= 1;
    pl->bwd_ok = multi_bwd_lds(*pl, nacc_max, pl->wpb) <= UMNN_LDS_LIMIT;
    return 0;
}

// The forward launch, with (f_nodes non-null: the NODES build, K >= 1, d = 1) or without the node values.
static int multi_forward(const umnn_mlp* net, const float* x0, const float* x, const float* h, const float* cc_w, const float* cc_s,
                         int nb_steps, long long B, int d, int E, int inv_f, float* F, float* f_x, float* f_x0, float* f_nodes,
                         hipStream_t stream) {
    MultiPlan pl;
    if (int rc = multi_plan(net, E, &pl, f_nodes ? 1 : 2)) return rc;
    if (nb_steps < 1) return umnn_fail(UMNN_EINVAL, "forward_multi: nb_steps must be >= 1");
    if (B < 0 || d < 1) return umnn_fail(UMNN_EINVAL, "forward_multi: B must be >= 0 and d >= 1");
    if (B == 0) return 0;
    if (!x || !h || !cc_w || !cc_s || !F) return umnn_fail(UMNN_EINVAL, "forward_multi: x, h, cc_w, cc_s, F must be non-null");
    MultiArgs& a = pl.a;
    a.x0 = x0; a.x = x; a.h = h; a.ccw = cc_w; a.ccs = cc_s; a.F = F; a.fx = f_x; a.fx0 = f_x0;
    a.NI = B * (long long)d; a.d = d; a.E = E; a.n = nb_steps; a.inv_f = inv_f != 0;
    // two point tiles per wave once every SIMD of the device has that much to do
    const long long tiles = (a.NI + 15) / 16;
    const int P = tiles >= 2LL * UMNN_WAVES_PER_BLOCK * umnn_num_cus() ? 2 : 1;
    const long long groups = (tiles + P - 1) / P;
    if (groups > 0x7fffffffLL) return umnn_fail(UMNN_EUNSUPPORTED, "forward_multi: batch too large");
    a.ngroups = (unsigned)groups;
    const unsigned blocks = (a.ngroups + UMNN_WAVES_PER_BLOCK - 1) / UMNN_WAVES_PER_BLOCK;
    const char* name = nullptr;
    if (f_nodes) {
        const MultiNodesVariant* v = nullptr;
        for (const MultiNodesVariant& c : kMultiNodes)
            if (c.T == pl.T && c.KS == pl.KS && c.P == P) v = &c;
        if (!v) return umnn_fail(UMNN_EUNSUPPORTED, "forward_multi_nodes: no kernel variant");
        if (int rc = umnn_allow_lds((const void*)v->fn, pl.fwd_lds)) return rc;
        umnn_prof_begin(stream);
        hipLaunchKernelGGL(v->fn, dim3(blocks), dim3(UMNN_BLOCK), pl.fwd_lds, stream, a, f_nodes);
        name = v->name;
    } else {
        const MultiFwdVariant* v = nullptr;
        for (const MultiFwdVariant& c : kMultiFwd)
            if (c.T == pl.T && c.KS == pl.KS && c.P == P) v = &c;
        if (!v) return umnn_fail(UMNN_EUNSUPPORTED, "forward_multi: no kernel variant");
        if (int rc = umnn_allow_lds((const void*)v->fn, pl.fwd_lds)) return rc;
        umnn_prof_begin(stream);
        hipLaunchKernelGGL(v->fn, dim3(blocks), dim3(UMNN_BLOCK), pl.fwd_lds, stream, a);
        name = v->name;
    }
    umnn_prof_end(stream, umnn_cc_forward_flops_per_integral(net, nb_steps) * (double)a.NI, UMNN_PROF_FORWARD);
    umnn_note_launch(name);
    return umnn_check(hipGetLastError(), "cc_fwd_multi launch");
}

extern "C" int umnn_cc_forward_multi(const umnn_mlp* net, const float* x0, const float* x, const float* h,
                                     const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, int inv_f,
                                     float* F, float* f_x, float* f_x0, void* stream) {
    return multi_forward(net, x0, x, h, cc_w, cc_s, nb_steps, B, d, E, inv_f, F, f_x, f_x0, nullptr, (hipStream_t)stream);
}

extern "C" int umnn_cc_forward_multi_nodes(const umnn_mlp* net, const float* x0, const float* x, const float* h,
                                           const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E,
                                           float* F, float* f_nodes, void* stream) {
    if (d != 1) return umnn_fail(UMNN_EINVAL, "forward_multi_nodes: d must be 1");
    if (B == 0) { MultiPlan pl; return multi_plan(net, E, &pl, 1); }           // (the checks of the net; nothing to launch)
    if (!f_nodes) return umnn_fail(UMNN_EINVAL, "forward_multi_nodes: f_nodes must be non-null");
    return multi_forward(net, x0, x, h, cc_w, cc_s, nb_steps, B, d, E, 0, F, nullptr, nullptr, f_nodes, (hipStream_t)stream);
}

typedef void (*solve_multi_kernel_t)(const SolveMultiArgs);
struct MultiSolveVariant { int T, KS; solve_multi_kernel_t fn; const char* name; };
#define MULTI_SOLVE(T, KS) { T, KS, cc_solve_multi_kernel<T, KS>, "cc_solve_multi<T=" #T ",KS=" #KS ">" }
static const MultiSolveVariant kMultiSolve[] = {
    MULTI_SOLVE(2, 8), MULTI_SOLVE(4, 13), MULTI_SOLVE(4, 16), MULTI_SOLVE(7, 26), MULTI_SOLVE(8, 32),
};

// The forward's plan, images and grid (one 16-row tile per wave); the argument checks of solve_entry (cc_solve.hip).
extern "C" int umnn_cc_solve_multi(const umnn_mlp* net, const float* h, const float* target, const float* coef,
                                   const float* cc_w, const float* cc_s, int nb_steps, long long B, int E,
                                   float lo, float hi, float tol, int max_iter,
                                   float* x, float* F, float* f_x, int* status, void* stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    if (!net) return umnn_fail(UMNN_EINVAL, "net is null");
    if (nb_steps < 1 || max_iter < 1 || max_iter > UMNN_SOLVE_EVALS_MASK)
        return umnn_fail(UMNN_EINVAL, "solve_multi: nb_steps >= 1 and 1 <= max_iter <= 65535");
    if (B < 0) return umnn_fail(UMNN_EINVAL, "solve_multi: B must be >= 0");
    if (!(lo < hi) || !(tol >= 0.f)) return umnn_fail(UMNN_EINVAL, "solve_multi: lo < hi and tol >= 0");
    SolveMultiArgs sa;
    MultiPlan pl;
    if (int rc = multi_plan(net, E, &pl)) return rc;
    if (B == 0) return 0;
    if (!h || !target || !coef || !cc_w || !cc_s || !x)
        return umnn_fail(UMNN_EINVAL, "solve_multi: h, target, coef, cc_w, cc_s, x must be non-null");
    sa.a = pl.a;
    MultiArgs& a = sa.a;
    a.h = h; a.ccw = cc_w; a.ccs = cc_s; a.F = F; a.fx = f_x;
    a.NI = B; a.d = 1; a.E = E; a.n = nb_steps;
    sa.target = target; sa.coef = coef; sa.x = x; sa.status = status;
    sa.lo = lo; sa.hi = hi; sa.tol = tol; sa.max_iter = max_iter;
    const long long tiles = (B + 15) / 16;
    if (tiles > 0x7fffffffLL) return umnn_fail(UMNN_EUNSUPPORTED, "solve_multi: batch too large");
    a.ngroups = (unsigned)tiles;
    const MultiSolveVariant* v = nullptr;
    for (const MultiSolveVariant& c : kMultiSolve)
        if (c.T == pl.T && c.KS == pl.KS) v = &c;
    if (!v) return umnn_fail(UMNN_EUNSUPPORTED, "solve_multi: no kernel variant");
    if (int rc = umnn_allow_lds((const void*)v->fn, pl.fwd_lds)) return rc;
    const unsigned blocks = (a.ngroups + UMNN_WAVES_PER_BLOCK - 1) / UMNN_WAVES_PER_BLOCK;
    umnn_prof_begin(stream);
    hipLaunchKernelGGL(v->fn, dim3(blocks), dim3(UMNN_BLOCK), pl.fwd_lds, stream, sa);
    // algorithmic work: the iteration count is decided inside the launch -- booked at four quadratures per row, like umnn_cc_solve
    umnn_prof_end(stream, umnn_cc_forward_flops_per_integral(net, nb_steps) * 4.0 * (double)B, UMNN_PROF_FORWARD);
    umnn_note_launch(v->name);
    return umnn_check(hipGetLastError(), "cc_solve_multi launch");
}

// workspace: [d_theta slices: 4 waves x CUs][dc: NI x H1][first-layer partials: nparts0 x H1 (E + 1)]
static long long multi_nparts0(long long NI) { const long long c = (NI + 63) / 64; return c < 1024 ? c : 1024; }
static void multi_workspace(const MultiPlan& pl, long long NI, int E, long long* o_dc, long long* o_p0, long long* total) {
    const long long H1 = pl.a.m.width[1];
    long long o = (long long)umnn_num_cus() * 4 * pl.a.n_params * 4; o = (o + 255) & ~255LL;
    *o_dc = o; o += NI * H1 * 4; o = (o + 255) & ~255LL;
    *o_p0 = o; o += multi_nparts0(NI) * H1 * (E + 1) * 4; o = (o + 255) & ~255LL;
    *total = o;
}

static long long multi_workspace_bytes(const umnn_mlp* net, long long B, int d, int E, int min_out) {
    if (B <= 0) return 0;
    MultiPlan pl;
    if (d < 1 || multi_plan(net, E, &pl, min_out)) return -1;
    if (!pl.bwd_ok) { umnn_fail(UMNN_EUNSUPPORTED, kMultiBwdLdsError); return -1; }
    long long o_dc, o_p0, total;
    multi_workspace(pl, B * (long long)d, E, &o_dc, &o_p0, &total);
    return total;
}

extern "C" long long umnn_cc_backward_multi_workspace_bytes(const umnn_mlp* net, long long B, int d, int E) {
    return multi_workspace_bytes(net, B, d, E, 2);
}

// (the same layout and, for K >= 2, the same figure: the node-cotangent entry takes a single output too)
extern "C" long long umnn_cc_backward_multi_nodes_workspace_bytes(const umnn_mlp* net, long long B, int E) {
    return multi_workspace_bytes(net, B, 1, E, 1);
}

// The backward launches: with g (and g_fx) the quadrature's cotangents, or -- `nodes`: the NC build of every pass, K >= 1, no cc_w --
// a cotangent per node, cot_nodes.
static int multi_backward(int nodes, const umnn_mlp* net, const float* x0, const float* x, const float* h, const float* g,
                          const float* g_fx, const float* cot_nodes, const float* cc_w, const float* cc_s, int nb_steps, long long B,
                          int d, int E, int inv_f, float* dx0, float* dx, float* dh, float* dtheta,
                          void* workspace, long long workspace_bytes, hipStream_t stream) {
    MultiPlan pl;
    if (int rc = multi_plan(net, E, &pl, nodes ? 1 : 2)) return rc;
    if (B < 0 || d < 1) return umnn_fail(UMNN_EINVAL, "backward_multi: B must be >= 0 and d >= 1");
    if (nb_steps < 1) return umnn_fail(UMNN_EINVAL, "backward_multi: nb_steps must be >= 1");
    if (!pl.bwd_ok) return umnn_fail(UMNN_EUNSUPPORTED, kMultiBwdLdsError);
    MultiArgs& a = pl.a;
    if (B == 0) {
        if (dtheta) return umnn_check(hipMemsetAsync(dtheta, 0, (size_t)a.n_params * sizeof(float), stream), "memset");
        return 0;
    }
    if (nodes ? (!x || !h || !cot_nodes || !cc_s) : (!x || !h || !g || !cc_w || !cc_s))
        return umnn_fail(UMNN_EINVAL, nodes ? "backward_multi_nodes: x, h, cot_nodes, cc_s must be non-null"
                                                : "backward_multi: x, h, g, cc_w, cc_s must be non-null");
    a.NI = B * (long long)d; a.d = d; a.E = E; a.n = nb_steps; a.inv_f = inv_f != 0;
    long long o_dc, o_p0, total;
    multi_workspace(pl, a.NI, E, &o_dc, &o_p0, &total);
    if (!workspace || workspace_bytes < total)
        return umnn_fail(UMNN_EINVAL, "backward_multi: workspace smaller than umnn_cc_backward_multi_workspace_bytes()");
    const long long tiles = (a.NI + 15) / 16;
    if (tiles > 0x7fffffffLL) return umnn_fail(UMNN_EUNSUPPORTED, "backward_multi: batch too large");
    a.ngroups = (unsigned)tiles;
    char* ws = (char*)workspace;
    a.x0 = x0; a.x = x; a.h = h; a.g = g; a.gfx = g_fx; a.cot = cot_nodes; a.ccw = cc_w; a.ccs = cc_s; a.dx0 = dx0; a.dx = dx;
    // the FX build of every pass; without a g_fx the kernels of umnn_cc_backward_multi; with node cotangents the NC build
    const int fx = nodes ? 2 : g_fx != nullptr;
    a.partials = (float*)ws;
    a.dc = (float*)(ws + o_dc);
    float* p0 = (float*)(ws + o_p0);
    const int L = a.m.n_linear - 1, H1 = a.m.width[1], cus = umnn_num_cus();
    // persistent waves: one workgroup per CU at most
    const int wpb = pl.wpb;
    long long nb = (tiles + wpb - 1) / wpb;
    if (nb > cus) nb = cus;
    const int nblocks = (int)nb, nslices = nblocks * wpb;
    if (int rc = umnn_check(hipMemsetAsync(a.partials, 0, (size_t)nslices * a.n_params * 4, stream), "memset partials")) return rc;

    MultiPass passes[UMNN_MAX_LINEAR + 1];
    const int npasses = multi_passes(pl.T, pl.KS, L - 1, dtheta != nullptr, passes);      // (the layers' dW feed d_theta only)
    for (int pass = 0; pass < npasses; ++pass) {
        const MultiBwdVariant* v = passes[pass].v;
        if (!v) return umnn_fail(UMNN_EUNSUPPORTED, "backward_multi: no kernel variant");
        a.l_lo = passes[pass].l_lo;
        a.outw = passes[pass].outw;
        a.scratch_per_wave = multi_scratch_per_wave(pl.T, v->nacc);
        const size_t lds = multi_bwd_lds(pl, v->nacc, wpb);
        if (int rc = umnn_allow_lds((const void*)v->fn[fx], lds)) return rc;
        if (int rc = umnn_bwd_launch(stream, pass == 0 ? umnn_bwd_flops(net, nb_steps, a.NI) : 0.0, v->name[fx], "cc_bwd_multi launch",
                                     [&] { hipLaunchKernelGGL(v->fn[fx], dim3(nblocks), dim3(64 * wpb), lds, stream, a); })) return rc;
    }

    // ---- finishing kernels
    if (dh)
        if (int rc = umnn_launch_bwd_dh(a.dc, net->W[0], dh, a.NI, d, E, H1, 0, stream)) return rc;
    if (dtheta) {
        const long long np0 = multi_nparts0(a.NI), per = (a.NI + np0 - 1) / np0;
        const int nparts0 = (int)((a.NI + per - 1) / per);
        hipLaunchKernelGGL(cc_bwd_multi_dw0_kernel, dim3(nparts0), dim3(256), 0, stream, a.dc, h, p0, a.NI, d, E, H1, per);
        hipLaunchKernelGGL(cc_bwd_multi_reduce_kernel, dim3((a.n_params + 255) / 256), dim3(256), 0, stream,
                           a.partials, nslices, a.n_params, p0, nparts0, E, H1, a.poffW[0], a.poffb[0], dtheta);
    }
    return umnn_check(hipGetLastError(), "cc_bwd_multi finishing launch");
}

extern "C" int umnn_cc_backward_multi_fx(const umnn_mlp* net, const float* x0, const float* x, const float* h, const float* g,
                                         const float* g_fx, const float* cc_w, const float* cc_s, int nb_steps, long long B, int d,
                                         int E, int inv_f, float* dx0, float* dx, float* dh, float* dtheta,
                                         void* workspace, long long workspace_bytes, void* stream) {
    return multi_backward(0, net, x0, x, h, g, g_fx, nullptr, cc_w, cc_s, nb_steps, B, d, E, inv_f, dx0, dx, dh, dtheta,
                          workspace, workspace_bytes, (hipStream_t)stream);
}

// The backward of a curve: cot_nodes [B][n + 1][K] is the cotangent of f_k(t_j; h) at every node, in the kernel's node order (node 0
// is x).  dx / dx0 receive sum_j (u_j / 2) tau_j and sum_j (1 - u_j / 2) tau_j, tau_j = sum_k cot[j][k] df_k/dt (t_j): what moving a
// limit does through the nodes (no Leibniz term: the caller owns the span factor).  dh, dtheta, the workspace layout, the passes and
// the finishing kernels are the multi-output backward's.
extern "C" int umnn_cc_backward_multi_nodes(const umnn_mlp* net, const float* x0, const float* x, const float* h,
                                            const float* cot_nodes, const float* cc_s, int nb_steps, long long B, int d, int E,
                                            float* dx0, float* dx, float* dh, float* dtheta,
                                            void* workspace, long long workspace_bytes, void* stream) {
    if (d != 1) return umnn_fail(UMNN_EINVAL, "backward_multi_nodes: d must be 1");
    return multi_backward(1, net, x0, x, h, nullptr, nullptr, cot_nodes, nullptr, cc_s, nb_steps, B, d, E, 0,
                          dx0, dx, dh, dtheta, workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int umnn_cc_backward_multi(const umnn_mlp* net, const float* x0, const float* x, const float* h, const float* g,
                                      const float* cc_w, const float* cc_s, int nb_steps, long long B, int d, int E, int inv_f,
                                      float* dx0, float* dx, float* dh, float* dtheta,
                                      void* workspace, long long workspace_bytes, void* stream) {
    return umnn_cc_backward_multi_fx(net, x0, x, h, g, nullptr, cc_w, cc_s, nb_steps, B, d, E, inv_f, dx0, dx, dh, dtheta,
                                     workspace, workspace_bytes, stream);
}
