// Diagnostic build of csrc/glue.hip: in-kernel cycle stamps of tmix_lora_down, tmix_lora_mix4 (weight-stationary) and decay_lora
// at the 30-minute shape (B = 1, T = 44 998, C = 512, two directions) on random data, in the plain loop (PAFC_TMIX_PIPE=0, the
// loop of the kernels before the prefetch) and with the next tile's loads in flight.  Per wave and trip the kernels write
// {tile start, cycles between "loads issued" and "first use of loaded data", arithmetic done, stores issued} through ordinary
// stores into a buffer of their own (TMIX_ST_* in glue.hip, compiled only with -DPAFC_TMIX_STAMPS); this prints the medians.
// The figure that decides: the share of a tile's time a wave spends between "loads issued" and "first use".
//   hipcc -O3 -std=c++17 --offload-arch=gfx950 -DPAFC_TMIX_STAMPS -I include -I paper_accurate_fast_cheap_amd/csrc \
//         tools/micro/tmix_front_stamps.cpp -o tools/micro/bin/tmix_front_stamps
//   tools/micro/bin/tmix_front_stamps [plain|pipe|both] [B T]
#include "../../paper_accurate_fast_cheap_amd/csrc/glue.hip"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

static unsigned short bf16_rne(float f) {
    unsigned u; memcpy(&u, &f, 4);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (unsigned short)(u >> 16);
}
static float gauss() {
    const float a = (rand() + 1.0f) / ((float)RAND_MAX + 2.0f), b = (rand() + 1.0f) / ((float)RAND_MAX + 2.0f);
    return sqrtf(-2.f * logf(a)) * cosf(6.2831853f * b);
}
static unsigned short *random_bf16(size_t n, float scale, float shift = 0.f) {
    std::vector<unsigned short> h(n);
    for (size_t i = 0; i < n; ++i) h[i] = bf16_rne(scale * gauss() + shift);
    unsigned short *d = nullptr;
    if (hipMalloc(&d, n * 2) != hipSuccess || hipMemcpy(d, h.data(), n * 2, hipMemcpyHostToDevice) != hipSuccess) {
        printf("allocation of %zu bytes failed\n", n * 2);
        exit(1);
    }
    return d;
}
static double median(std::vector<double> &v) {
    if (v.empty()) return 0;
    std::nth_element(v.begin(), v.begin() + v.size() / 2, v.end());
    return v[v.size() / 2];
}

constexpr long CAP_WAVES = 8192;       // mix4: 128 x 8 x 2 blocks of 4 waves; the other two: one block of 8 waves per CU
static unsigned long long *g_dev = nullptr;
constexpr size_t N_STAMPS = (size_t)CAP_WAVES * pafc::TMIX_STAMP_TRIPS * 4;

template <typename F> static void stamped(const char *kernel, const char *form, F &&launch) {
    float ms = 0;
    hipEvent_t e0, e1;
    hipEventCreate(&e0); hipEventCreate(&e1);
    for (int rep = 0; rep < 3; ++rep) {        // the last of three launches is the one whose stamps are read
        hipMemset(g_dev, 0, N_STAMPS * 8);
        hipEventRecord(e0, 0);
        const int rc = launch();
        hipEventRecord(e1, 0);
        if (rc != 0 || hipEventSynchronize(e1) != hipSuccess) { printf("%s %s: rc %d / %s\n", kernel, form, rc, hipGetErrorString(hipGetLastError())); exit(1); }
        hipEventElapsedTime(&ms, e0, e1);
    }
    std::vector<unsigned long long> h(N_STAMPS);
    hipMemcpy(h.data(), g_dev, N_STAMPS * 8, hipMemcpyDeviceToHost);
    std::vector<double> tile, wait, arith, store, share, trips;
    for (long w = 0; w < CAP_WAVES; ++w) {
        int n = 0;
        for (int tr = 0; tr < pafc::TMIX_STAMP_TRIPS; ++tr) {
            const unsigned long long *s = &h[((size_t)w * pafc::TMIX_STAMP_TRIPS + tr) * 4];
            if (s[0] == 0 || s[3] <= s[0]) continue;
            ++n;
            const double tt = (double)(s[3] - s[0]);
            tile.push_back(tt); wait.push_back((double)s[1]);
            arith.push_back((double)(s[2] - s[0]) - (double)s[1]); store.push_back((double)(s[3] - s[2]));
            share.push_back(100.0 * (double)s[1] / tt);
        }
        if (n) trips.push_back(n);
    }
    printf("%-22s %-5s %7.1f us with stamps | %5zu waves, median %1.0f stamped trips | medians per tile (clocks): tile %7.0f  "
           "loads issued -> first use %7.0f (%4.1f %% of the tile)  to arithmetic done %7.0f  to stores issued %7.0f\n",
           kernel, form, ms * 1e3, trips.size(), median(trips), median(tile), median(wait), median(share), median(arith), median(store));
}

int main(int argc, char **argv) {
    const char *which = argc > 1 ? argv[1] : "both";
    const int B = argc > 2 ? atoi(argv[2]) : 1, T = argc > 3 ? atoi(argv[3]) : 44998;
    const int C = 512, nd = 2;
    const long rows = (long)B * T;
    srand(11);
    unsigned short *x = random_bf16((size_t)rows * C, 1.f), *maa_x = random_bf16((size_t)nd * C, 0.5f);
    unsigned short *w1n = random_bf16((size_t)nd * 128 * C, 1.5f / sqrtf((float)C)), *t = random_bf16((size_t)nd * rows * 128, 0.5f);
    unsigned short *w2t = random_bf16((size_t)nd * 4 * C * 32, 0.2f), *maa = random_bf16((size_t)nd * 4 * C, 0.5f);
    unsigned short *d1n = random_bf16((size_t)nd * 64 * C, 2.f / sqrtf((float)C)), *d2n = random_bf16((size_t)nd * C * 64, 0.3f);
    unsigned short *bias = random_bf16((size_t)nd * C, 1.f, -3.f), *zw = random_bf16((size_t)nd * rows * C, 1.f);
    unsigned short *tout, *z, *w;
    if (hipMalloc(&tout, (size_t)nd * rows * 128 * 2) != hipSuccess || hipMalloc(&z, (size_t)4 * nd * rows * C * 2) != hipSuccess ||
        hipMalloc(&w, (size_t)nd * rows * C * 2) != hipSuccess || hipMalloc(&g_dev, N_STAMPS * 8) != hipSuccess) {
        printf("allocation failed\n");
        return 1;
    }
    const long cap = CAP_WAVES;
    hipMemcpyToSymbol(HIP_SYMBOL(pafc::g_tmix_stamps), &g_dev, sizeof(g_dev));
    hipMemcpyToSymbol(HIP_SYMBOL(pafc::g_tmix_stamp_waves), &cap, sizeof(cap));
    printf("B %d T %d C %d, %d directions; a tile is 16 rows; stamps of each wave's first %d trips\n", B, T, C, nd, pafc::TMIX_STAMP_TRIPS);
    for (int pipe = 0; pipe < 2; ++pipe) {
        if ((pipe == 0 && !strcmp(which, "pipe")) || (pipe == 1 && !strcmp(which, "plain"))) continue;
        setenv("PAFC_TMIX_PIPE", pipe ? "1" : "0", 1);
        const char *form = pipe ? "pipe" : "plain";
        stamped("tmix_lora_down<8>", form, [&] { return pafc_tmix_lora_down_bf16_prev(B, T, C, 128, nd, 0, x, maa_x, w1n, nullptr, tout, 0); });
        stamped("tmix_lora_mix4_ws<4,1>", form, [&] { return pafc_tmix_lora_mix4_bf16_prev(B, T, C, nd, 0, x, t, w2t, maa, nullptr, z, 0); });
        stamped("decay_lora", form, [&] { return pafc_decay_lora_bf16(rows, C, 64, nd, zw, d1n, d2n, bias, w, 0); });
    }
    return 0;
}
