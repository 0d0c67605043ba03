// Walks the case table of tests/_bwd_plan_cases.py through the backward's launch plan (umnn_amd/csrc/cc_bwd_plan.h: shape plan + route)
// as a stand-alone host program, so that the header can run under the host sanitizers; it launches nothing and needs no GPU.
//
//   hipcc --offload-arch=gfx950 -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/bwd_plan_walk.hip umnn_amd/csrc/cc_api.hip -fsanitize=address,undefined -o /tmp/bwd_plan_walk && /tmp/bwd_plan_walk
//
// Exit status 0: every case routed to the kernel name the table expects (and every B - 1 neighbour was planned too).
#include <cstdio>
#include <cstring>

#include "../umnn_amd/csrc/cc_bwd_plan.h"

struct Case {
    const char* id;
    int n_hidden, hid[5];
    long long B;
    int d, n;
    const char* name;
    int E, flags, out_act;
    BwdOptions o;          // bwd_precision, bwd_ws, bwd_ws16, bwd_swp, bwd_ns, front_bwd2
};
#define DEFAULTS {UMNN_PRECISION_BF16X3, 1, 1, 1, -1, 1}
#define FP32 {UMNN_PRECISION_FP32, 1, 1, 1, -1, 1}
#define WS16(v) {UMNN_PRECISION_BF16X3, 1, v, 1, -1, 1}
#define ELU UMNN_OUT_ELU_PLUS_ONE
static const Case kCases[] = {
    {"boundary-f16", 4, {50, 50, 50, 50}, 1024, 16, 127, "cc_bwd_f16<L=4,LIVE=13,WS>", 30, 0, ELU, DEFAULTS},
    {"boundary-n126", 4, {50, 50, 50, 50}, 1024, 16, 126, "cc_bwd_bf16<L=4,LIVE=13,WS>", 30, 0, ELU, DEFAULTS},
    {"boundary-B1023", 4, {50, 50, 50, 50}, 1023, 16, 127, "cc_bwd_bf16<L=4,LIVE=13,SWP>", 30, 0, ELU, DEFAULTS},
    {"boundary-f16-E6", 4, {50, 50, 50, 50}, 1024, 16, 127, "cc_bwd_f16<L=4,LIVE=13,WS>", 6, 0, ELU, DEFAULTS},
    {"ws16=2-n256", 4, {50, 50, 50, 50}, 300, 63, 256, "cc_bwd_bf16<L=4,LIVE=13,WS>", 30, 0, ELU, WS16(2)},
    {"ws16=2-n255", 4, {50, 50, 50, 50}, 300, 63, 255, "cc_bwd_f16<L=4,LIVE=13,WS>", 30, 0, ELU, WS16(2)},
    {"ws16=2-inv_f", 4, {50, 50, 50, 50}, 300, 63, 20, "cc_bwd_bf16<L=4,LIVE=13,WS>", 30, UMNN_PLAN_INV_F, ELU, WS16(2)},
    {"ws16=2-sigmoid", 4, {50, 50, 50, 50}, 300, 63, 20, "cc_bwd_bf16<L=4,LIVE=13,WS>", 30, 0, UMNN_OUT_SIGMOID, WS16(2)},
    {"default-300x63", 4, {50, 50, 50, 50}, 300, 63, 120, "cc_bwd_f16<L=4,LIVE=13,WS>", 30, 0, ELU, DEFAULTS},
    {"ws16=0", 4, {50, 50, 50, 50}, 300, 63, 120, "cc_bwd_bf16<L=4,LIVE=13,WS>", 30, 0, ELU, WS16(0)},
    {"ws=0", 4, {50, 50, 50, 50}, 300, 63, 120, "cc_bwd_bf16<L=4,LIVE=13,SWP>", 30, 0, ELU, {UMNN_PRECISION_BF16X3, 0, 0, 1, -1, 1}},
    {"swp=0", 4, {50, 50, 50, 50}, 300, 63, 120, "cc_bwd_bf16<L=4,EDGE=1,LIVE=13>", 30, 0, ELU, {UMNN_PRECISION_BF16X3, 0, 0, 0, -1, 1}},
    {"three-hidden", 3, {50, 50, 50}, 300, 63, 20, "cc_bwd_bf16<L=3,LIVE=13,SWP>", 30, 0, ELU, DEFAULTS},
    {"small-batch", 4, {50, 50, 50, 50}, 64, 63, 20, "cc_bwd_bf16<L=4,LIVE=13,SWP>", 30, 0, ELU, DEFAULTS},
    {"mixed-widths", 4, {48, 60, 36, 50}, 300, 63, 20, "cc_bwd_bf16<L=4,LIVE=0,WS>", 30, 0, ELU, DEFAULTS},
    {"two-tiles", 2, {20, 20}, 9, 3, 12, "cc_bwd<T=2,NACC=3,EDGE=1,KS=0>", 4, 0, ELU, DEFAULTS},
    {"fp32-50x4", 4, {50, 50, 50, 50}, 300, 63, 20, "cc_bwd<T=4,NACC=3,EDGE=1,KS=13>", 30, 0, ELU, FP32},
    {"fp32-pad17", 2, {66, 60}, 9, 3, 12, "cc_bwd<T=5,NACC=2,EDGE=1,KS=17>", 4, 0, ELU, FP32},
    {"fp32-pad26", 3, {100, 80, 70}, 9, 3, 12, "cc_bwd<T=7,NACC=1,EDGE=0,KS=26>", 4, 0, ELU, FP32},
    {"fp32-pad26-two", 2, {70, 90}, 9, 3, 12, "cc_bwd<T=7,NACC=1,EDGE=1,KS=26>", 4, 0, ELU, FP32},
    {"fp32-pad32", 3, {120, 112, 116}, 9, 3, 12, "cc_bwd<T=8,NACC=1,EDGE=0,KS=32>", 4, 0, ELU, FP32},
    {"pad26-default", 3, {100, 80, 70}, 9, 3, 12, "cc_bwd<T=7,NACC=1,EDGE=0,KS=26>", 4, 0, ELU, DEFAULTS},
    {"deep-wide-generic", 5, {100, 80, 70, 90, 70}, 9, 3, 12, "cc_bwd<T=7,NACC=1,EDGE=0,KS=0>", 4, 0, ELU, DEFAULTS},
    {"deep-wide-none", 4, {120, 112, 116, 124}, 9, 3, 12, "", 4, 0, ELU, DEFAULTS},
    {"front", 5, {100, 50, 50, 50, 50}, 40, 784, 12, "cc_bwd_bf16<L=4,LIVE=13,WS,FRONT>", 30, 0, ELU, DEFAULTS},
    {"front-ws=0", 5, {100, 50, 50, 50, 50}, 40, 784, 12, "cc_bwd_bf16<L=4,EDGE=1,LIVE=13,FRONT>", 30, 0, ELU, {UMNN_PRECISION_BF16X3, 0, 1, 1, -1, 1}},
    {"front-ws16=2", 5, {100, 50, 50, 50, 50}, 40, 784, 12, "cc_bwd_f16<L=4,LIVE=13,WS,FRONT>", 30, 0, ELU, WS16(2)},
    {"front-fp32", 5, {100, 50, 50, 50, 50}, 40, 784, 12, "cc_bwd_bf16x6<L=4,EDGE=1,LIVE=13,FRONT>", 30, 0, ELU, FP32},
    {"front-g_fx", 5, {100, 50, 50, 50, 50}, 40, 784, 12, "cc_bwd_bf16<L=4,LIVE=13,WS,FRONT>", 30, UMNN_PLAN_G_FX, ELU, DEFAULTS},
    {"front-z2-saved", 5, {100, 50, 50, 50, 50}, 40, 784, 12, "cc_bwd_bf16<L=4,LIVE=13,WS,FRONT>", 30, UMNN_PLAN_Z2_SAVED, ELU, DEFAULTS},
    {"front-few-tiles", 5, {100, 50, 50, 50, 50}, 9, 3, 12, "cc_bwd_bf16<L=4,EDGE=1,LIVE=13,FRONT>", 4, 0, ELU, DEFAULTS},
    {"front-many-nodes", 5, {100, 50, 50, 50, 50}, 1, 1, 2000, "cc_bwd<T=7,NACC=1,EDGE=0,KS=0>", 4, 0, ELU, DEFAULTS},   // scratch below one tile at this n: the fp32 passes
};

// shape plan + route of (c, B); "" where the call would return an error
static const char* plan_name(const Case& c, long long B, const float* dummy) {
    umnn_mlp net;
    memset(&net, 0, sizeof(net));
    net.n_linear = c.n_hidden + 1;
    net.widths[0] = 1 + c.E;
    for (int l = 0; l < c.n_hidden; ++l) net.widths[l + 1] = c.hid[l];
    net.widths[c.n_hidden + 1] = 1;
    for (int l = 0; l < net.n_linear; ++l) { net.W[l] = dummy; net.b[l] = dummy; }
    net.hidden_act = UMNN_ACT_LEAKY_RELU;
    net.out_act = c.out_act;
    MlpDev m;
    int tmax = 0, ksu = 0;
    if (umnn_prepare_mlp(&net, c.E, &m, &tmax, &ksu)) return "";
    BwdShapePlan pl{};
    if (bwd_plan_shape(&pl, m, tmax, ksu, B, c.d, c.E, 256, c.o.bwd_ns)) return "";
    const BwdRoute rt = bwd_route(pl, c.n, (c.flags & UMNN_PLAN_INV_F) != 0, (c.flags & UMNN_PLAN_G_FX) != 0,
                                  (c.flags & UMNN_PLAN_Z2_SAVED) != 0, true, c.o);
    return rt.error ? "" : rt.name;
}

int main() {
    const float dummy = 0.f;
    int bad = 0;
    for (const Case& c : kCases) {
        const char* name = plan_name(c, c.B, &dummy);
        const bool ok = !strcmp(name, c.name);
        if (c.B > 1) (void)plan_name(c, c.B - 1, &dummy);
        printf("%-20s %-44s %s\n", c.id, name, ok ? "ok" : "MISMATCH");
        bad += !ok;
    }
    printf("%d cases, %d mismatches\n", (int)(sizeof(kCases) / sizeof(kCases[0])), bad);
    return bad ? 1 : 0;
}
