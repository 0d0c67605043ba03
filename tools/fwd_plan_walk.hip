// Walks cases of tests/_fwd_plan_cases.py through the launch plan of the forward, the bracket search and the Newton solve
// (umnn_amd/csrc/cc_fwd_plan.h) as a stand-alone host program, so that the header can run under the host sanitizers; it launches
// nothing and needs no GPU.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/fwd_plan_walk.hip umnn_amd/csrc/cc_api.hip -fsanitize=address,undefined -o /tmp/fwd_plan_walk && /tmp/fwd_plan_walk
//
// Exit status 0: every case planned the kernel name, P, ns and grid the table expects (B - 1 and B + 1 of each case were planned too),
// and every variant of the fp16 tables sits at the same index of the bf16 tables.
#include <cstdio>
#include <cstring>

#include "../umnn_amd/csrc/cc_fwd_plan.h"

struct Case {
    const char* id;
    int job, n_hidden, hid[7];
    long long B;
    int d, n, E;
    bool alias, z2;
    FwdOptions o;          // fwd_precision, fwd_p, fwd_ns, fwd_tail, fwd_pipe, fwd_pad, fwd_pad_min
    const char* name;
    int P, ns;
    unsigned blocks;
};
#define OPT(prec, p, ns, tail, pipe, pad) {prec, p, ns, tail, pipe, pad, 1}
#define DEFAULTS OPT(UMNN_PRECISION_F16X3, -1, -1, -1, 1, 1)
#define PREC(prec) OPT(prec, -1, -1, -1, 1, 1)
#define FWD FWD_JOB_FORWARD
static const Case kCases[] = {
    {"c3", FWD, 4, {50, 50, 50, 50}, 8192, 63, 100, 30, false, false, DEFAULTS, "cc_fwd_f16<T=4,PARTS=2,P=2,EXACT=1,LIVE=13,PIPE>", 2, 1, 4032},
    {"few-tiles", FWD, 4, {50, 50, 50, 50}, 37, 3, 20, 30, false, false, DEFAULTS, "cc_fwd_f16<T=4,PARTS=2,P=1,EXACT=1,LIVE=13>", 1, 4, 7},
    {"pipe-2048-tiles", FWD, 4, {50, 50, 50, 50}, 2048, 16, 4, 30, false, false, DEFAULTS, "cc_fwd_f16<T=4,PARTS=2,P=2,EXACT=1,LIVE=13,PIPE>", 2, 1, 256},
    {"pipe-2047-tiles", FWD, 4, {50, 50, 50, 50}, 2047, 16, 4, 30, false, false, DEFAULTS, "cc_fwd_f16<T=4,PARTS=2,P=1,EXACT=1,LIVE=13>", 1, 2, 1024},
    {"few-nodes", FWD, 4, {50, 50, 50, 50}, 37, 3, 2, 30, false, false, DEFAULTS, "cc_fwd_f16<T=4,PARTS=2,P=1,EXACT=1,LIVE=13>", 1, 1, 2},
    {"bf16x6-8192-tiles", FWD, 4, {50, 50, 50, 50}, 8192, 16, 4, 30, false, false, PREC(UMNN_PRECISION_BF16X6), "cc_fwd_bf16<T=4,PARTS=3,P=2,EXACT=1,LIVE=13>", 2, 1, 1024},
    {"bf16x6-8191-tiles", FWD, 4, {50, 50, 50, 50}, 8191, 16, 4, 30, false, false, PREC(UMNN_PRECISION_BF16X6), "cc_fwd_bf16<T=4,PARTS=3,P=1,EXACT=1,LIVE=13>", 1, 1, 2048},
    {"aliased", FWD, 4, {50, 50, 50, 50}, 37, 3, 20, 30, true, false, DEFAULTS, "cc_fwd_bf16<T=4,PARTS=2,P=1,EXACT=1,LIVE=13>", 1, 4, 7},
    {"fp32-c3", FWD, 4, {50, 50, 50, 50}, 8192, 63, 100, 30, false, false, PREC(UMNN_PRECISION_FP32), "cc_fwd<T=4,KS=13,P=2,TAIL=1>", 2, 1, 4032},
    {"fp32-width-51", FWD, 4, {51, 51, 51, 51}, 37, 3, 20, 30, false, false, PREC(UMNN_PRECISION_FP32), "cc_fwd<T=4,KS=13,P=1,TAIL=0>", 1, 4, 7},
    {"fp32-tail=0", FWD, 4, {50, 50, 50, 50}, 37, 3, 20, 30, false, false, OPT(UMNN_PRECISION_FP32, -1, -1, 0, 1, 1), "cc_fwd<T=4,KS=13,P=1,TAIL=0>", 1, 4, 7},
    {"one-hidden-layer", FWD, 1, {50}, 37, 3, 20, 30, false, false, DEFAULTS, "cc_fwd<T=4,KS=13,P=1,TAIL=1>", 1, 4, 7},
    {"pipe32", FWD, 4, {50, 50, 50, 50}, 8192, 63, 100, 30, false, false, OPT(UMNN_PRECISION_BF16X3, -1, -1, -1, 2, 1), "cc_fwd_bf16<32x32x16,PARTS=2,P=2,EXACT=1,LIVE=26,PIPE32>", 2, 1, 4032},
    {"pipe32-f16x3", FWD, 4, {50, 50, 50, 50}, 8192, 63, 100, 30, false, false, OPT(UMNN_PRECISION_F16X3, -1, -1, -1, 2, 1), "cc_fwd_f16<T=4,PARTS=2,P=2,EXACT=1,LIVE=13,PIPE>", 2, 1, 4032},
    {"wide-100", FWD, 3, {100, 100, 100}, 65536, 2, 20, 30, false, false, DEFAULTS, "cc_fwd_f16<T=7,PARTS=2,P=1,EXACT=1,LIVE=26,WAVES=8>", 1, 1, 1024},
    {"wide-100-ns2", FWD, 3, {100, 100, 100}, 600, 16, 20, 30, false, false, DEFAULTS, "cc_fwd_f16<T=7,PARTS=2,P=1,EXACT=1,LIVE=26,WAVES=8>", 1, 2, 150},
    {"wide-100-p-forced", FWD, 3, {100, 100, 100}, 37, 3, 20, 30, false, false, OPT(UMNN_PRECISION_F16X3, 2, -1, -1, 1, 1), "cc_fwd_f16<T=8,PARTS=2,P=2,EXACT=0,LIVE=0>", 2, 4, 4},
    {"wide-first", FWD, 5, {100, 50, 50, 50, 50}, 100, 784, 20, 30, false, false, DEFAULTS, "cc_fwd_f16<T1=7,TREST=4,PARTS=2,P=1,EXACT=1,LIVE=13>", 1, 1, 1225},
    {"wide-first-z2", FWD, 5, {100, 50, 50, 50, 50}, 40, 784, 20, 30, false, true, DEFAULTS, "cc_fwd_f16<T1=7,TREST=4,PARTS=2,P=1,EXACT=1,LIVE=13>", 1, 1, 490},
    {"wide-first-z2-fp32", FWD, 5, {100, 50, 50, 50, 50}, 40, 784, 20, 30, false, true, PREC(UMNN_PRECISION_FP32), "", 0, 0, 0},
    {"two-tiles", FWD, 2, {20, 20}, 37, 3, 20, 30, false, false, DEFAULTS, "cc_fwd_f16<T=2,PARTS=2,P=1,EXACT=0,LIVE=0>", 1, 4, 7},
    {"padded", FWD, 4, {48, 60, 36, 50}, 37, 3, 20, 30, false, false, DEFAULTS, "cc_fwd_f16<T=4,PARTS=2,P=1,EXACT=1,LIVE=0>", 1, 4, 7},
    {"pad=0", FWD, 4, {48, 60, 36, 50}, 37, 3, 20, 30, false, false, OPT(UMNN_PRECISION_F16X3, -1, -1, -1, 1, 0), "cc_fwd_f16<T=4,PARTS=2,P=1,EXACT=0,LIVE=0>", 1, 4, 7},
    {"ns-forced", FWD, 4, {50, 50, 50, 50}, 2048, 16, 4, 30, false, false, OPT(UMNN_PRECISION_F16X3, -1, 2, -1, 1, 1), "cc_fwd_f16<T=4,PARTS=2,P=1,EXACT=1,LIVE=13>", 1, 2, 1024},
    {"images-exceed-lds", FWD, 7, {120, 120, 120, 120, 120, 120, 120}, 37, 3, 20, 4, false, false, DEFAULTS, "", 0, 0, 0},
    {"search-50x4", FWD_JOB_SEARCH, 4, {50, 50, 50, 50}, 10, 3, 20, 4, false, false, DEFAULTS, "cc_invert_f16<T=4,EXACT=1,LIVE=13>", 1, 4, 10},
    {"search-513-tiles", FWD_JOB_SEARCH, 4, {50, 50, 50, 50}, 513, 3, 20, 4, false, false, DEFAULTS, "cc_invert_f16<T=4,EXACT=1,LIVE=13>", 1, 1, 129},
    {"search-100x3", FWD_JOB_SEARCH, 3, {100, 100, 100}, 10, 3, 20, 4, false, false, DEFAULTS, "cc_invert_f16<T=7,EXACT=1,LIVE=26,WAVES=8>", 1, 8, 10},
    {"search-wide-first", FWD_JOB_SEARCH, 3, {100, 50, 50}, 10, 3, 20, 4, false, false, DEFAULTS, "cc_invert_f16<T1=7,TREST=4,LIVE=13>", 1, 4, 10},
    {"search-bf16x6", FWD_JOB_SEARCH, 4, {50, 50, 50, 50}, 10, 3, 20, 4, false, false, PREC(UMNN_PRECISION_BF16X6), "cc_invert_bf16<T=4,PARTS=3,EXACT=1,LIVE=13>", 1, 4, 10},
    {"solve-fp32-100x3", FWD_JOB_SOLVE, 3, {100, 100, 100}, 37, 3, 20, 4, false, false, PREC(UMNN_PRECISION_FP32), "cc_solve_f16<T=7,EXACT=1,LIVE=26,WAVES=8>", 1, 8, 3},
    {"solve-scratch-does-not-fit", FWD_JOB_SOLVE, 4, {120, 120, 100, 70}, 37, 3, 20, 4, false, false, DEFAULTS, "cc_solve_f16<T=8,EXACT=0,LIVE=0>", 1, 1, 1},
    {"solve-one-hidden-layer", FWD_JOB_SOLVE, 1, {50}, 37, 3, 20, 4, false, false, DEFAULTS, "", 0, 0, 0},
};

static FwdPlan plan_of(const Case& c, long long B, const float* dummy) {
    umnn_mlp net;
    memset(&net, 0, sizeof(net));
    net.n_linear = c.n_hidden + 1;
    net.widths[0] = 1 + c.E;
    for (int l = 0; l < c.n_hidden; ++l) net.widths[l + 1] = c.hid[l];
    net.widths[c.n_hidden + 1] = 1;
    for (int l = 0; l < net.n_linear; ++l) { net.W[l] = dummy; net.b[l] = dummy; }
    net.hidden_act = UMNN_ACT_LEAKY_RELU;
    net.out_act = UMNN_OUT_ELU_PLUS_ONE;
    MlpDev m;
    int tmax = 0, ksu = 0;
    FwdPlan none{};
    none.error = UMNN_EINVAL; none.name = "";
    if (umnn_prepare_mlp(&net, c.E, &m, &tmax, &ksu)) return none;
    const FwdCall call = c.job == FWD_JOB_FORWARD ? fwd_call_forward(B * c.d, c.n, c.alias, c.z2)
                         : c.job == FWD_JOB_SEARCH ? fwd_call_search(B, c.n) : fwd_call_solve(B, c.n);
    return fwd_plan(m, tmax, ksu, call, c.o, 256);
}

int main() {
    const float dummy = 0.f;
    int bad = 0;
    for (const Case& c : kCases) {
        const FwdPlan pl = plan_of(c, c.B, &dummy);
        const char* name = pl.error ? "" : pl.name;
        const bool ok = !strcmp(name, c.name) && (pl.error || (pl.P == c.P && pl.ns == c.ns && pl.blocks == c.blocks && pl.lds_bytes <= UMNN_LDS_LIMIT));
        if (c.B > 1) (void)plan_of(c, c.B - 1, &dummy);
        (void)plan_of(c, c.B + 1, &dummy);
        printf("%-28s %-58s P %d ns %d blocks %u  %s\n", c.id, name, pl.P, pl.ns, pl.blocks, ok ? "ok" : "MISMATCH");
        bad += !ok;
    }
    printf("%d cases, %d mismatches\n", (int)(sizeof(kCases) / sizeof(kCases[0])), bad);
    return bad ? 1 : 0;
}
