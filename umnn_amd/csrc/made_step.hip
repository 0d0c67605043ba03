// One step of the PROGRESSIVE MADE conditioner of the sequential sampling walk (reference models/UMNN/UMNNMAF.py:195-231 re-runs
// the whole conditioner before every dimension; made.py:68-100 builds the masks this rests on).
//
// With the natural input order, a hidden unit of degree m reads inputs of degree <= m only, so once x_0..x_{j-1} are final every
// unit of degree <= c + j - 1 is final for the rest of the walk.  The host plan (umnn_amd/made.py: MADE.progressive_plan) sorts every
// hidden layer by degree; step j computes the units [lo, hi) of each layer that became ready, stores them in the standing
// activation buffers act_l [B, ld] (degree order), and the E outputs of dimension j into h[b, e*d + j].
//
// Work split: a workgroup of four waves owns 16*RT rows and runs the layers in order.  One unit tile (16 units) at a time:
//   * the K range [0, prefix) is cut into chunks of 16; wave w takes chunks w, w+4, ... and accumulates D[unit][row] on
//     v_mfma_f32_16x16x4_f32 (exact fp32 products, fp32 accumulation): lane (g, rho) loads W'[u0 + rho][16q + 4g .. +3] and
//     a[row rho][16q + 4g .. +3] as one 16-byte load each and issues four MFMAs (slot t pairs k = 16q + 4g + t of the four lane groups);
//   * the four partial tiles meet in LDS and are added in the fixed order ((w0 + w1) + w2) + w3, then bias, ReLU.
// The order of every sum is a function of the prefix alone: it does not depend on B, the grid or RT.
// Hand-off inside a step: units computed in THIS launch are read by the next layer from LDS (two buffers, alternating by layer),
// behind a barrier; units of earlier steps come from the standing buffers an earlier launch on the same stream wrote.  Nothing is
// read back from global memory that this launch wrote.
// Prefix discipline: element k of an operand row is loaded only when k < prefix; columns >= j of x and units outside the prefix are
// never touched (they may hold anything, NaN included).
#include <hip/hip_runtime.h>
#include "cc_host.h"
#include "../../include/umnn_cc.h"

#define MS_LAYERS (UMNN_MADE_MAX_LAYERS + 1)

struct StepDev {
    const float* W[MS_LAYERS];      // layer l's permuted masked weight; the output layer's already offset to dimension j
    const float* b[MS_LAYERS];
    float* act[UMNN_MADE_MAX_LAYERS];
    int ldk[MS_LAYERS];             // K stride of W[l]; act[l] has row stride ldk[l + 1]
    int lo[MS_LAYERS], hi[MS_LAYERS], pre[MS_LAYERS];
    const float* ctx;
    const float* x;
    float* h;
    long long B;
    int n_hidden, d, c, E, j, cap;
};

template <int RT>
__global__ __launch_bounds__(256) void made_step_kernel(const StepDev p) {
    extern __shared__ float lds[];
    float* part = lds;                                  // [4 waves][RT][16 rows][16 units]
    float* hand = lds + 4 * RT * 256;                   // two buffers [16 RT rows][cap], alternating by layer
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, rho = lane & 15;
    const long long row0 = (long long)blockIdx.x * (16 * RT);
    const int cap = p.cap;

    for (int l = 0; l <= p.n_hidden; ++l) {
        const bool last = l == p.n_hidden;
        const int lo = p.lo[l], hi = p.hi[l], K = p.pre[l], ldw = p.ldk[l];
        const float* __restrict__ W = p.W[l];
        const float* __restrict__ bias = p.b[l];
        const int plo = l > 0 ? p.lo[l - 1] : 0;
        const float* prev = hand + ((l + 1) & 1) * (16 * RT * cap);
        float* mine = hand + (l & 1) * (16 * RT * cap);
        const float* __restrict__ src = l > 0 ? p.act[l - 1] : nullptr;
        const int lda = ldw;                            // (act[l - 1]'s row stride is W[l]'s K stride)
        const int vec_end = K < plo ? K : plo;          // [0, vec_end): standing units, whole 16-byte loads
        const int nchunk = (K + 15) >> 4;

        for (int u0 = lo; u0 < hi; u0 += 16) {
            f32x4 acc[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) acc[rt] = f32x4{0.f, 0.f, 0.f, 0.f};
            const int u = u0 + rho;
            const bool uok = u < hi;
            const float* wrow = W + (long long)(uok ? u : lo) * ldw;
            for (int q = wave; q < nchunk; q += 4) {
                const int k = 16 * q + 4 * g;
                f32x4 a = f32x4{0.f, 0.f, 0.f, 0.f};
                if (uok && k < K) a = *reinterpret_cast<const f32x4*>(wrow + k);        // (k < K <= ldw, both multiples of 4 apart)
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
                    const int rl = rt * 16 + rho;
                    const long long row = row0 + rl;
                    f32x4 v = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (row < p.B) {
                        if (l > 0 && k + 4 <= vec_end) {
                            v = *reinterpret_cast<const f32x4*>(src + row * lda + k);
                        } else {
#pragma unroll
                            for (int t = 0; t < 4; ++t) {
                                const int kk = k + t;
                                if (kk < K) {
                                    if (l == 0) v[t] = kk < p.c ? p.ctx[row * p.c + kk] : p.x[row * p.d + (kk - p.c)];
                                    else v[t] = kk >= plo ? prev[rl * cap + (kk - plo)] : src[row * lda + kk];
                                }
                            }
                        }
                    }
#pragma unroll
                    for (int t = 0; t < 4; ++t) acc[rt] = mfma16(a[t], v[t], acc[rt]);
                }
            }
            // D[unit 4g + v][row rho] -> part[wave][rt][row rho][unit 4g .. 4g + 3]
#pragma unroll
            for (int rt = 0; rt < RT; ++rt)
                *reinterpret_cast<f32x4*>(part + (wave * RT + rt) * 256 + rho * 16 + 4 * g) = acc[rt];
            __syncthreads();
            {
                const int r = tid >> 4, ui = tid & 15, uu = u0 + ui;
                if (uu < hi) {
                    const float bv = bias[uu];
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        float s = ((part[(0 * RT + rt) * 256 + tid] + part[(1 * RT + rt) * 256 + tid]) + part[(2 * RT + rt) * 256 + tid])
                                  + part[(3 * RT + rt) * 256 + tid];
                        s += bv;
                        const int rl = rt * 16 + r;
                        const long long row = row0 + rl;
                        if (!last) {
                            s = fmaxf(s, 0.f);
                            mine[rl * cap + (uu - lo)] = s;
                            if (row < p.B) p.act[l][row * p.ldk[l + 1] + uu] = s;
                        } else if (row < p.B) {
                            p.h[row * ((long long)p.E * p.d) + (long long)uu * p.d + p.j] = s;
                        }
                    }
                }
            }
            __syncthreads();
        }
    }
}

static const size_t MS_LDS_MAX = 64 * 1024;
static size_t ms_lds_bytes(int rt, int cap) { return (size_t)(4 * rt * 256 + 2 * 16 * rt * cap) * sizeof(float); }

extern "C" int umnn_made_step(const umnn_made_plan* plan, int j, const float* context, const float* x, float* const* act, float* h,
                              long long B, int row_tiles, void* stream) {
    if (!plan) return umnn_fail(UMNN_EINVAL, "made_step: plan must be non-null");
    const int nh = plan->n_hidden, d = plan->d, c = plan->c, E = plan->E;
    if (nh < 1 || nh > UMNN_MADE_MAX_LAYERS) return umnn_fail(UMNN_EUNSUPPORTED, "made_step: 1..8 hidden layers");
    if (d < 1 || c < 0 || E < 1 || B < 0) return umnn_fail(UMNN_EINVAL, "made_step: bad shape");
    if (j < 0 || j >= d) return umnn_fail(UMNN_EINVAL, "made_step: j outside [0, d)");
    if (row_tiles != 0 && row_tiles != 1 && row_tiles != 2 && row_tiles != 4) return umnn_fail(UMNN_EINVAL, "made_step: row_tiles 0|1|2|4");
    if (!plan->steps) return umnn_fail(UMNN_EINVAL, "made_step: plan tables must be non-null");
    for (int l = 0; l <= nh; ++l) {
        if (l < nh && plan->width[l] < 1) return umnn_fail(UMNN_EINVAL, "made_step: bad hidden width");
        const int Kl = l == 0 ? c + d : plan->width[l - 1];
        if (plan->ldk[l] < Kl || (plan->ldk[l] & 3)) return umnn_fail(UMNN_EINVAL, "made_step: ldk[l] must be a multiple of 4, >= the layer's input width");
    }
    StepDev p;
    p.cap = 1;
    const int* st = plan->steps + (size_t)j * (nh + 1) * 3;
    for (int l = 0; l <= nh; ++l) {
        const int N = l < nh ? plan->width[l] : E, Kmax = l == 0 ? c + j : p.hi[l - 1];
        p.lo[l] = st[3 * l]; p.hi[l] = st[3 * l + 1]; p.pre[l] = st[3 * l + 2];
        if (p.lo[l] < 0 || p.lo[l] > p.hi[l] || p.hi[l] > N || p.pre[l] < 0 || p.pre[l] > Kmax)
            return umnn_fail(UMNN_EINVAL, "made_step: step table out of range (new units within the layer; prefix within the computed units)");
        if (l < nh && p.hi[l] - p.lo[l] > UMNN_MADE_STEP_MAX_NEW)
            return umnn_fail(UMNN_EUNSUPPORTED, "made_step: more new units in one step than the LDS hand-off holds");
        if (l < nh && ((p.hi[l] - p.lo[l]) | 1) > p.cap) p.cap = (p.hi[l] - p.lo[l]) | 1;
    }
    if (p.lo[nh] != 0 || p.hi[nh] != E) return umnn_fail(UMNN_EINVAL, "made_step: the output entry of the step table must be [0, E)");
    if (B == 0) return 0;
    if (!x || !h || !act || (c > 0 && !context)) return umnn_fail(UMNN_EINVAL, "made_step: x, h, act (and context when c > 0) must be non-null");
    for (int l = 0; l <= nh; ++l)
        if (!plan->W[l] || !plan->b[l] || (l < nh && !act[l])) return umnn_fail(UMNN_EINVAL, "made_step: weights, biases and activation buffers must be non-null");
    int rt = row_tiles ? row_tiles : (B >= 32768 ? 4 : B >= 8192 ? 2 : 1);
    while (rt > 1 && ms_lds_bytes(rt, p.cap) > MS_LDS_MAX) rt >>= 1;
    if (ms_lds_bytes(rt, p.cap) > MS_LDS_MAX) return umnn_fail(UMNN_EUNSUPPORTED, "made_step: LDS hand-off too large");
    const long long groups = (B + 16 * rt - 1) / (16 * rt);
    if (groups > 0x7fffffffLL) return umnn_fail(UMNN_EUNSUPPORTED, "made_step: batch too large");
    for (int l = 0; l <= nh; ++l) {
        p.W[l] = plan->W[l]; p.b[l] = plan->b[l]; p.ldk[l] = plan->ldk[l];
        if (l < nh) p.act[l] = act[l];
    }
    p.W[nh] += (size_t)j * E * plan->ldk[nh];
    p.b[nh] += (size_t)j * E;
    p.ctx = context; p.x = x; p.h = h; p.B = B;
    p.n_hidden = nh; p.d = d; p.c = c; p.E = E; p.j = j;
    const size_t lds = ms_lds_bytes(rt, p.cap);
    hipStream_t s = (hipStream_t)stream;
    if (rt == 4) { hipLaunchKernelGGL(made_step_kernel<4>, dim3((unsigned)groups), dim3(256), lds, s, p); umnn_note_made_launch("made_step<RT=4>"); }
    else if (rt == 2) { hipLaunchKernelGGL(made_step_kernel<2>, dim3((unsigned)groups), dim3(256), lds, s, p); umnn_note_made_launch("made_step<RT=2>"); }
    else { hipLaunchKernelGGL(made_step_kernel<1>, dim3((unsigned)groups), dim3(256), lds, s, p); umnn_note_made_launch("made_step<RT=1>"); }
    return umnn_check(hipGetLastError(), "made_step launch");
}
