// Phase timing of k_frames_seq at the config-2 shape (65,536 frames of 1 KiB,
// one session, decode with the ordered look-back), diagnostic build
// (-DZMQG_SEQ_STAMPS=1): per wave, s_memtime at entry (0), before window 0
// (1), after it (2), at the start of step t (3+t), after step t's keystream
// (24+t), at the end of the loop (60) and of the kernel (61); for steps 1..7
// also when the window's input words are in registers (44+t), when the next
// window's DMA has been issued (52+t) and when the stores have (36+t).
// The phase before window 0 in its parts: the kernel's first instruction
// (20), every line of its arguments there (21), group B issued (22), the
// header checked (23; the stamped build pins S and the nonce there, the
// product build does not, so the split around it is the stamped kernel's);
// in window 0, its keystream done (24) and its other words there (63).
// STAMP_REPS launches per direction back to back (the clock settles), the
// last one stamped.  Prints one JSON line of medians over the waves, in
// s_memtime ticks.
// Build: hipcc -O3 -std=c++17 --offload-arch=gfx950 -DZMQG_SEQ_STAMPS=1 -o tools/bin/seq_stamps tools/seq_stamps.hip
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>
#include "../libzmq_amd/csrc/curve_frames.hpp"
#ifndef STAMP_REPS
#define STAMP_REPS 200
#endif
using namespace zmqg;
struct StampNoBig {
    const uint8_t *zflags = nullptr;
    const unsigned long long *res_src = nullptr;
    unsigned long long *res_dst = nullptr;
    __device__ void operator()(uint32_t, unsigned long long *, uint64_t) const {}
};

#define CHECK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)

int main(int argc, char **argv)
{
    const char *label = argc > 1 ? argv[1] : "build";
    const uint32_t n = 65536, P = 1024, W = P + 33;
    std::vector<uint32_t> sid(n, 0), len(n, P), wl(n, W);
    std::vector<uint64_t> nonce(n), ioff(n), ooff(n);
    std::vector<uint8_t> flags(n, 0);
    for (uint32_t i = 0; i < n; ++i) {
        nonce[i] = 3 + i;
        ioff[i] = (uint64_t) i * P;
        ooff[i] = (uint64_t) i * W;
    }
    auto dev = [](const void *h, size_t b) {
        void *d = nullptr;
        if (hipMalloc(&d, b + 256) != hipSuccess || hipMemcpy(d, h, b, hipMemcpyHostToDevice) != hipSuccess)
            return (void *) nullptr;
        return d;
    };
    uint32_t *d_sid = (uint32_t *) dev(sid.data(), 4 * n), *d_len = (uint32_t *) dev(len.data(), 4 * n),
             *d_wl = (uint32_t *) dev(wl.data(), 4 * n);
    uint64_t *d_nonce = (uint64_t *) dev(nonce.data(), 8 * n), *d_ioff = (uint64_t *) dev(ioff.data(), 8 * n),
             *d_ooff = (uint64_t *) dev(ooff.data(), 8 * n);
    uint8_t *d_flags = (uint8_t *) dev(flags.data(), n);
    uint8_t *d_pay, *d_wire, *d_back, *d_fl;
    int32_t *d_st;
    CHECK(hipMalloc(&d_pay, (size_t) n * P + 256));
    CHECK(hipMemset(d_pay, 0x3c, (size_t) n * P + 256));
    CHECK(hipMalloc(&d_wire, (size_t) n * W + 256));
    CHECK(hipMalloc(&d_back, (size_t) n * P + 256));
    CHECK(hipMalloc(&d_fl, n));
    CHECK(hipMalloc(&d_st, 4 * n));
    DevSession *d_ses;
    CHECK(hipMalloc(&d_ses, sizeof(DevSession)));
    CHECK(hipMemset(d_ses, 0x11, sizeof(DevSession)));
    ZState *d_zs;
    CHECK(hipMalloc(&d_zs, sizeof(ZState)));
    ZState z0{};
    z0.epoch = 1;
    CHECK(hipMemcpy(d_zs, &z0, sizeof z0, hipMemcpyHostToDevice));
    const uint32_t nwg = n / kFramesBS;
    const size_t nwaves = n / 64;
    // replay state of the one-session decode: peer nonce, per-frame excl, look-back arrays
    unsigned long long *d_v, *d_clk;
    const size_t lbw = 8 * (size_t) nwg; // (each look-back array: at most 8 words per workgroup)
    CHECK(hipMalloc(&d_v, 8 * (2 + n + 4 * lbw)));
    CHECK(hipMemset(d_v, 0, 8 * (2 + n + 4 * lbw)));
    CHECK(hipMalloc(&d_clk, 8 * 64 * nwaves));
    CHECK(hipMemset(d_clk, 0, 8 * 64 * nwaves));
    ReplayOut rp{};
    const dim3 grid(nwg);
    printf("{\"label\": \"%s\", \"shape\": \"65536 x 1024 B, one session\", \"unit\": \"s_memtime ticks, median over %zu waves\"",
           label, nwaves);
    for (int dec = 0; dec < 2; ++dec) {
        CHECK(hipMemset(d_clk, 0, 8 * 64 * nwaves));
        if (dec) {
            rp.peer = d_v;
            rp.excl = d_v + 2;
            rp.lb_flag = d_v + 2 + n;
            rp.lb_agg = rp.lb_flag + lbw;
            rp.lb_inc = rp.lb_agg + lbw;
            rp.lb_rec = rp.lb_inc + lbw;
            rp.ordered = 1;
        }
        for (int rep = 0; rep < STAMP_REPS; ++rep) {
            rp.clk = rep == STAMP_REPS - 1 ? d_clk : nullptr;
            if (!dec) {
                hipLaunchKernelGGL((k_frames_seq<false, StampNoBig>), grid, dim3(kFramesBS), 0, 0, n, d_sid, d_nonce,
                                   d_flags, d_ioff, d_len, d_pay, d_ooff, d_wire, d_ses, 1u, 0xffffffffu, nullptr,
                                   nullptr, rp, StampNoBig{}, d_zs, FrameCtl{});
            } else {
                CHECK(hipMemsetAsync(d_v, 0, 8, 0)); // (the peer nonce: every launch sees a fresh batch)
                hipLaunchKernelGGL((k_frames_seq<true, StampNoBig>), grid, dim3(kFramesBS), 0, 0, n, d_sid,
                                   (const uint64_t *) nullptr, (const uint8_t *) nullptr, d_ooff, d_wl, d_wire, d_ioff,
                                   d_back, d_ses, 1u, 0xffffffffu, d_fl, d_st, rp, StampNoBig{}, d_zs, FrameCtl{});
            }
        }
        CHECK(hipDeviceSynchronize());
        std::vector<unsigned long long> c(64 * nwaves);
        CHECK(hipMemcpy(c.data(), d_clk, 8 * 64 * nwaves, hipMemcpyDeviceToHost));
        if (dec) {
            std::vector<int32_t> st(n);
            CHECK(hipMemcpy(st.data(), d_st, 4 * n, hipMemcpyDeviceToHost));
            size_t bad = 0;
            for (uint32_t i = 0; i < n; ++i)
                bad += st[i] != 0;
            if (bad)
                return printf("\ndecode: %zu frames with a status\n", bad), 2;
        }
        // median over waves of slot b - slot a
        auto med = [&](int a, int b) {
            std::vector<long long> v;
            for (size_t w = 0; w < nwaves; ++w)
                if (c[64 * w + a] && c[64 * w + b])
                    v.push_back((long long) (c[64 * w + b] - c[64 * w + a]));
            if (v.empty())
                return -1ll;
            std::sort(v.begin(), v.end());
            return v[v.size() / 2];
        };
        printf(", \"%s\": {\"total\": %lld, \"entry_to_window0\": %lld, \"window0\": %lld, \"window0_to_step1\": %lld, "
               "\"steps_2_15_mean\": %.1f, \"step16\": %lld, \"loop_end_to_exit\": %lld, ",
               dec ? "decode" : "encode", med(0, 61), med(0, 1), med(1, 2), med(2, 4), med(5, 19) / 14.0, med(19, 60),
               med(60, 61));
        // the phase before window 0 in its parts: the kernel arguments (the
        // first instruction to all of their lines there), group A (to group
        // B issued), group B's head (to the header checks done), the set-up;
        // then window 0's keystream and the wait for window 0's other words
        printf("\"first_instruction_to_window0\": %lld, \"entry_parts\": {\"kernel_arguments\": %lld, "
               "\"arguments_to_first_stamp\": %lld, \"group_a\": %lld, \"group_b_head\": %lld, "
               "\"setup\": %lld, \"keystream0\": %lld, \"barrier_and_words\": %lld}, \"steps\": [",
               med(20, 1), med(20, 21), med(21, 0), med(0, 22), med(22, 23), med(23, 1), med(1, 24), med(24, 63));
        for (int t = 1; t <= 7; ++t)
            printf("%s{\"t\": %d, \"compute_before_wait\": %lld, \"wait_to_input_ready\": %lld, \"xor_dma_issue\": %lld, "
                   "\"store_issue\": %lld, \"step\": %lld}",
                   t > 1 ? ", " : "", t, med(3 + t, 24 + t), med(24 + t, 44 + t), med(44 + t, 52 + t),
                   med(52 + t, 36 + t), med(3 + t, 4 + t));
        printf("]}");
    }
    printf("}\n");
    return 0;
}
