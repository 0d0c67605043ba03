// Shared by the backward kernels (fp32-MFMA and bf16-split): launch arguments; the device pieces of the fp32-MFMA kernels, single-
// and multi-output (cc_backward.hip, cc_multi.hip); the launch bracket of a main pass.
#pragma once
#include "cc_host.h"

struct BwdArgs {
    MlpDev m;
    int ld[UMNN_MAX_LINEAR];        // row stride (floats) of the row-major image of hidden layer l -> l+1
    int roff[UMNN_MAX_LINEAR];      // float offset of that image in LDS
    int poffW[UMNN_MAX_LINEAR];     // offset of W_l / b_l in the flat theta vector
    int poffb[UMNN_MAX_LINEAR];
    const float* x0;
    const float* x;
    const float* h;
    const float* g;
    const float* gfx;               // nullable
    const float* ccw;
    const float* ccs;
    float* dx0;                     // nullable
    float* dx;                      // nullable
    float* dc;                      // [NI][H1] (EDGE pass)
    float* partials;                // [nwaves][n_params]
    int x_bf16, h_bf16;             // storage of x, x0, g, g_fx, dx, dx0 / of h (and dh): 0 fp32, 1 bf16
    int inv_f;                      // the quadrature integrated 1/f (ParallelNeuralIntegral.py:58-59,70-72): d_theta and d_h
                                    // differentiate 1/f -- node cotangent x (-1/f^2); the Leibniz terms keep f (:120-123)
    long long NI;
    int d, E, n;
    unsigned ngroups;               // tiles of 16 integrals
    int ns;                         // node-range split: a tile's nodes are shared by ns work items (small batches);
                                    // part j writes its dc partial at dc + j*NI*H1 (summed by the finishing kernels)
    int l_lo;                       // this pass accumulates dW for hidden layers l_lo .. l_lo+NACC-1
    int n_params;
    int scratch_off;                // float offset of the per-wave scratch region in LDS
    int scratch_per_wave;           // floats
    const float* z2_saved;          // nullable: hidden layer 2's pre-activations of every node, left by the training forward
                                    // (umnn_flow_stack_block_forward_save) -- the three-stage backward then skips its stage A
    unsigned* scal;                 // 256 B of launch scalars in the workspace (cotangent scale / overflow flag of cc_bwd_ws16_kernel.h)
};

// offsets of W_l / b_l in the flat theta vector (parameters() order); returns the parameter count
inline int bwd_param_offsets(const MlpDev& m, int* poffW, int* poffb) {
    int po = 0;
    for (int l = 0; l < m.n_linear; ++l) {
        poffW[l] = po; po += m.width[l + 1] * m.width[l];
        poffb[l] = po; po += m.width[l + 1];
    }
    return po;
}

// ---- device pieces that cc_bwd_kernel (cc_backward.hip) and cc_bwd_multi_kernel (cc_multi.hip) both call, so the padding rule of
// an image and the kink convention are written once.  Plain pointers and integers: no launch-argument struct, no branch on the
// caller.  Only pieces that leave the instructions of both kernels' tile and node loops as they were are here: the first-layer
// hoist, the K-step loops, the transpose scratch and the d_theta slice write are still written out in each kernel, because as
// shared helpers they re-scheduled those 512-register loops (+1.5 % and +0.9 % on two kernels; profiles/multi_shared/).

// permutation that turns an accumulator row (lane&15 in an A operand) into a feature offset inside a tile
__device__ __forceinline__ int perm16(int rho) { return 4 * (rho & 3) + (rho >> 2); }

// One row-major image of `rows` rows of LD floats: row fo < Hout = [W[fo][0 .. Hin), b[fo], 0 ...], the rows above zero -- but
// for the constant-one feature, row Hout column Hin, where the consumer is another hidden layer (one_row).
__device__ __forceinline__ void stage_rowmajor_image(float* img, const float* __restrict__ W, const float* __restrict__ b, int rows,
                                                     int LD, int Hin, int Hout, bool one_row, int tid, int nthreads) {
    for (int idx = tid; idx < rows * LD; idx += nthreads) {
        const int fo = idx / LD, fi = idx - fo * LD;
        float v = 0.f;
        if (fo < Hout) {
            if (fi < Hin) v = W[fo * Hin + fi];
            else if (fi == Hin) v = b[fo];
        } else if (one_row && fo == Hout && fi == Hin) {
            v = 1.f;
        }
        img[idx] = v;
    }
}

template <int TMAX>
__device__ __forceinline__ unsigned sign_bits(const f32x4 (&v)[TMAX]) {
    unsigned bits = 0;
#pragma unroll
    for (int t = 0; t < TMAX; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) bits |= (v[t][r] > 0.f ? 1u : 0u) << (4 * t + r);
    return bits;
}
// act'(z) of component (t, r) from those bits: the kink belongs to the slope side (z = 0 -> slope)
__device__ __forceinline__ float act_grad_bits(unsigned bits, int t, int r, float slope) { return (bits >> (4 * t + r)) & 1u ? 1.f : slope; }

// One main-pass launch of the backward: profiling bracket (flops: 3 x the forward's for the pass that does the work), the launch
// itself, its name for umnn_last_kernel_name_of(UMNN_PROF_BACKWARD), the launch check.
template <class Launch>
inline int umnn_bwd_launch(hipStream_t stream, double flops, const char* name, const char* what, Launch&& launch) {
    umnn_prof_begin(stream);
    launch();
    umnn_prof_end(stream, flops, UMNN_PROF_BACKWARD);
    umnn_note_launch(name);
    return umnn_check(hipGetLastError(), what);
}
inline double umnn_bwd_flops(const umnn_mlp* net, int n, long long NI) { return 3.0 * umnn_cc_forward_flops_per_integral(net, n) * (double)NI; }
