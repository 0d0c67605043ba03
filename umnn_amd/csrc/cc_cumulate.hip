// Cumulative Clenshaw-Curtis quadrature: the integral up to EVERY node from the node values of one quadrature.
//
//   out[q][n - i][k] = (x_q - x0_q)/2 * sum_j Q[i][j] v[q][j][k]        i, j = 0..n,  k < K <= 16
//
// Q [n+1][n+1] is the antiderivative of the quadrature's interpolant at the nodes (quadrature.cc_cumulative_matrix: row 0 = the
// Clenshaw-Curtis weights, row n = 0); v [NI][n+1][K] the node values cc_fwd_multi_nodes_kernel leaves (node 0 is x), or any other
// values at the nodes.  The output index is reversed, so a curve runs from the lower limit (index 0, exactly 0) to the upper.
//
// Per row this is a [n+1, n+1] x [n+1, K] product on v_mfma_f32_16x16x4_f32 (exact fp32), D[i][k] += A[i][j] B[j][k]:
//   * A fragments from Q, staged once per workgroup in LDS in fragment order, img[(t * KSP + s) * 64 + lane] =
//     Q[16 t + (lane & 15)][4 s + (lane >> 4)], zero beyond n: read with a conflict-free ds_read_b32, no bounds in the loop;
//   * B fragments straight from memory, lane (g, p) of K-step s reads v[q][4 s + g][p]: lanes run along k, and the four lane groups
//     along consecutive nodes, which are adjacent in memory -- coalesced, fully so at K = 16;
//   * the accumulator of tile t, component r of lane (g, p), is node i = 16 t + 4 g + r of output k = p.
// A wave owns one row at a time and strides over the rows; MT = 1, 2, 4 or 8 row tiles of Q (n + 1 <= 16 MT) are template
// constants, the K-steps (padded to a multiple of four, so that four loads are in flight) a launch argument.  Plain vector loads
// and stores, no atomics: two runs are bit-identical.
//
// The adjoint (umnn_cc_cumulate_adjoint, the ADJ build: the same body with another epilogue) is the product alone,
//   out[q][j][k] = sum_i Qt[j][i] g[q][i][k]
// -- no span factor and no reversed index: the host picks the (transposed) table, so that g is taken ascending, as the public
// outputs are, and out lands where the caller wants it (quadrature.device_cumulative_adjoint).
#include "cc_host.h"

struct CumulateArgs {
    const float* Q;
    const float* v;
    const float* x0;                // nullable
    const float* x;
    float* out;
    long long NI;
    int n, K, KSP;
};

constexpr size_t UMNN_CUMULATE_LDS = 64 * 1024;     // Q's image: MT * KSP * 256 bytes, n + 1 <= 128

template <int MT, bool ADJ = false>
__global__ __launch_bounds__(UMNN_BLOCK) void cc_cumulate_kernel(const CumulateArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 4, p = lane & 15;
    const int n = a.n, K = a.K, KSP = a.KSP;

    for (int idx = tid; idx < MT * KSP * 64; idx += UMNN_BLOCK) {
        const int ln = idx & 63, ts = idx >> 6;
        const int s = ts % KSP, t = ts / KSP;
        const int i = 16 * t + (ln & 15), j = 4 * s + (ln >> 4);
        lds[idx] = (i <= n && j <= n) ? a.Q[i * (n + 1) + j] : 0.f;
    }
    __syncthreads();

    const float* img = lds + lane;
    const long long nwaves = (long long)gridDim.x * UMNN_WAVES_PER_BLOCK;
    const long long row = (long long)(n + 1) * K;
    for (long long q = (long long)blockIdx.x * UMNN_WAVES_PER_BLOCK + wid; q < a.NI; q += nwaves) {
        const float* __restrict__ vq = a.v + q * row;
        f32x4 acc[MT];
#pragma unroll
        for (int t = 0; t < MT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s0 = 0; s0 < KSP; s0 += 4) {
            float b[4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int j = 4 * (s0 + c) + g;
                b[c] = (j <= n && p < K) ? vq[j * K + p] : 0.f;
            }
#pragma unroll
            for (int c = 0; c < 4; ++c)
#pragma unroll
                for (int t = 0; t < MT; ++t) acc[t] = mfma16(img[(t * KSP + s0 + c) * 64], b[c], acc[t]);
        }
        float* __restrict__ oq = a.out + q * row;
        if (ADJ) {
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * t + 4 * g + r;
                    if (i <= n && p < K) oq[i * K + p] = acc[t][r];
                }
        } else {
            const float dxv = a.x[q] - (a.x0 ? a.x0[q] : 0.f);
#pragma unroll
            for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int i = 16 * t + 4 * g + r;
                    if (i <= n && p < K) oq[(n - i) * K + p] = acc[t][r] * dxv * 0.5f;
                }
        }
    }
}

typedef void (*cumulate_kernel_t)(const CumulateArgs);
// fn / name [1]: the adjoint build (noted as a backward launch: the launch notes class a kernel by the cc_bwd prefix of its name)
struct CumulateVariant { int MT; cumulate_kernel_t fn[2]; const char* name[2]; };
#define CUMULATE(MT) { MT, {cc_cumulate_kernel<MT>, cc_cumulate_kernel<MT, true>}, {"cc_cumulate<MT=" #MT ">", "cc_bwd_cumulate_adjoint<MT=" #MT ">"} }
static const CumulateVariant kCumulate[] = { CUMULATE(1), CUMULATE(2), CUMULATE(4), CUMULATE(8) };

static int cumulate_launch(const float* Q, const float* values, const float* x0, const float* x, int nb_steps, long long NI,
                           int K, float* out, int adj, hipStream_t stream) {
    if (nb_steps < 1) return umnn_fail(UMNN_EINVAL, adj ? "cumulate_adjoint: nb_steps must be >= 1" : "cumulate: nb_steps must be >= 1");
    if (NI < 0) return umnn_fail(UMNN_EINVAL, adj ? "cumulate_adjoint: NI must be >= 0" : "cumulate: NI must be >= 0");
    if (K < 1 || K > UMNN_MAX_OUTPUTS)
        return umnn_fail(UMNN_EINVAL, adj ? "cumulate_adjoint: K must be between 1 and UMNN_MAX_OUTPUTS" : "cumulate: K must be between 1 and UMNN_MAX_OUTPUTS");
    CumulateArgs a;
    a.n = nb_steps; a.K = K; a.NI = NI;
    a.KSP = (((nb_steps + 1 + 3) / 4) + 3) & ~3;
    const CumulateVariant* v = nullptr;
    for (const CumulateVariant& c : kCumulate)
        if (!v && nb_steps + 1 <= 16 * c.MT) v = &c;
    const size_t lds = v ? (size_t)v->MT * a.KSP * 64 * sizeof(float) : 0;
    if (!v || lds > UMNN_CUMULATE_LDS)
        return umnn_fail(UMNN_EUNSUPPORTED, adj ? "cumulate_adjoint: the table of nb_steps > 127 exceeds the 64 KiB LDS budget"
                                                : "cumulate: the table of nb_steps > 127 exceeds the 64 KiB LDS budget");
    if (NI == 0) return 0;
    if (!Q || !values || (!adj && !x) || !out)
        return umnn_fail(UMNN_EINVAL, adj ? "cumulate_adjoint: Qt, g, out must be non-null" : "cumulate: Q, values, x, out must be non-null");
    a.Q = Q; a.v = values; a.x0 = x0; a.x = x; a.out = out;
    if (int rc = umnn_allow_lds((const void*)v->fn[adj], lds)) return rc;
    // a wave strides over the rows: at least eight per wave once there are that many, so that staging Q is a small part of its work
    long long blocks = (NI + 8 * UMNN_WAVES_PER_BLOCK - 1) / (8 * UMNN_WAVES_PER_BLOCK);
    const long long cap = 8LL * umnn_num_cus();
    if (blocks > cap) blocks = cap;
    umnn_prof_begin(stream);
    hipLaunchKernelGGL(v->fn[adj], dim3((unsigned)blocks), dim3(UMNN_BLOCK), lds, stream, a);
    umnn_prof_end(stream, 2.0 * (nb_steps + 1) * (nb_steps + 1) * K * (double)NI, adj ? UMNN_PROF_BACKWARD : UMNN_PROF_FORWARD);
    umnn_note_launch(v->name[adj]);
    return umnn_check(hipGetLastError(), "cc_cumulate launch");
}

extern "C" int umnn_cc_cumulate(const float* Q, const float* values, const float* x0, const float* x, int nb_steps, long long NI,
                                int K, float* out, void* stream) {
    return cumulate_launch(Q, values, x0, x, nb_steps, NI, K, out, 0, (hipStream_t)stream);
}

extern "C" int umnn_cc_cumulate_adjoint(const float* Qt, const float* g, int nb_steps, long long NI, int K, float* out, void* stream) {
    return cumulate_launch(Qt, g, nullptr, nullptr, nb_steps, NI, K, out, 1, (hipStream_t)stream);
}
