// Stand-alone host check of the fbank entry points' pure host pieces (csrc/fbank_host.h: frame arithmetic, the streaming carry
// plan, argument validation).  No HIP, no device: build it with the host compiler and sanitizers and run it,
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include tools/fbank_host_check.cpp -o check && ./check
// Exit status 0 and "fbank host check ok" mean every case held.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../paper_accurate_fast_cheap_amd/csrc/fbank_host.h"

namespace fh = pafc::fbank_host;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                            \
        }                                                                            \
    } while (0)

int main() {
    // frame arithmetic
    CHECK(fh::num_frames(0) == 0 && fh::num_frames(399) == 0 && fh::num_frames(400) == 1 && fh::num_frames(559) == 1);
    CHECK(fh::num_frames(560) == 2 && fh::num_frames(400 + 160 * 63) == 64 && fh::num_frames(32123) == 199);

    // the carry plan: every carry length against a set of packet sizes
    const long ns[] = {0, 1, 159, 160, 161, 399, 400, 10240};
    for (int c = 0; c < fh::CARRY; ++c)
        for (long n : ns) {
            long frames = -1;
            int c_next = -1;
            CHECK(fh::stream_plan(c, n, &frames, &c_next) == PAFC_OK);
            CHECK(frames == fh::num_frames(c + n));
            CHECK(c_next >= 0 && c_next < fh::CARRY && c_next == c + n - fh::SHIFT * frames);
            if (frames == 0) CHECK(c_next == c + n && c_next < fh::WIN);
        }
    CHECK(fh::stream_plan(-1, 5, nullptr, nullptr) == PAFC_ERR_BAD_DIMS);
    CHECK(fh::stream_plan(fh::CARRY, 5, nullptr, nullptr) == PAFC_ERR_BAD_DIMS);
    CHECK(fh::stream_plan(0, -1, nullptr, nullptr) == PAFC_ERR_BAD_DIMS);
    CHECK(fh::stream_plan(0, 0x7fffffffL * 160 + 400, nullptr, nullptr) == PAFC_ERR_BAD_DIMS);   // frames past int32
    CHECK(fh::stream_plan(3, 7, nullptr, nullptr) == PAFC_OK);                                    // outputs are optional

    // a stream cut into packets: the frames add up and the carry is a real tail (simulated on a host array)
    unsigned long long rng = 12345;
    auto next = [&](int mod) { rng = rng * 6364136223846793005ULL + 1442695040888963407ULL; return (int)((rng >> 33) % mod); };
    for (long S = 0; S <= 3000; S += 7) {
        std::vector<float> x(S), carry(fh::CARRY, -1.f);
        for (long i = 0; i < S; ++i) x[i] = (float)i;
        long pos = 0, total = 0;
        int c = 0;
        while (pos < S) {
            long n = 1 + next(700);
            if (n > S - pos) n = S - pos;
            long frames;
            int c_next;
            CHECK(fh::stream_plan(c, n, &frames, &c_next) == PAFC_OK);
            // frame f of this packet starts at absolute sample pos - c + 160 f: the frames continue where the last packet stopped
            CHECK(pos - c == fh::SHIFT * total);
            std::vector<float> cat(carry.begin(), carry.begin() + c);
            cat.insert(cat.end(), x.begin() + pos, x.begin() + pos + n);
            for (int j = 0; j < c_next; ++j) carry[j] = cat[cat.size() - c_next + j];
            pos += n;
            total += frames;
            c = c_next;
            for (int j = 0; j < c; ++j) CHECK(carry[j] == (float)(pos - c + j));
        }
        CHECK(total == fh::num_frames(S));
    }

    // argument validation (addresses are never dereferenced)
    const void *one = (const void *)16;
    long t_max = 0;
    CHECK(fh::tables_null(one, one, nullptr, one, one) && !fh::tables_null(one, one, one, one, one));
    CHECK(fh::batch_check(nullptr, 800, 2, 800, false, 80, one, PAFC_F32, &t_max) == PAFC_ERR_NULL_POINTER);
    CHECK(fh::batch_check(one, 800, 2, 800, true, 80, one, PAFC_F32, &t_max) == PAFC_ERR_NULL_POINTER);
    CHECK(fh::batch_check(one, 800, 2, 800, false, 80, nullptr, PAFC_F32, &t_max) == PAFC_ERR_NULL_POINTER);
    CHECK(fh::batch_check(one, 800, 0, 800, false, 80, one, PAFC_F32, &t_max) == PAFC_ERR_BAD_DIMS);
    CHECK(fh::batch_check(one, 800, 70000, 800, false, 80, one, PAFC_F32, &t_max) == PAFC_ERR_BAD_DIMS);
    CHECK(fh::batch_check(one, 800, 2, 800, false, 129, one, PAFC_F32, &t_max) == PAFC_ERR_BAD_DIMS);
    CHECK(fh::batch_check(one, 799, 2, 800, false, 80, one, PAFC_F32, &t_max) == PAFC_ERR_BAD_DIMS);      // ld_wave < max_samples
    CHECK(fh::batch_check(one, 399, 2, 399, false, 80, one, PAFC_F32, &t_max) == PAFC_ERR_BAD_DIMS);      // T_max == 0
    CHECK(fh::batch_check(one, 1L << 40, 2, 1L << 40, false, 80, one, PAFC_F32, &t_max) == PAFC_ERR_BAD_DIMS);   // past int32
    CHECK(fh::batch_check(one, 800, 2, 800, false, 80, one, 7, &t_max) == PAFC_ERR_DTYPE);
    CHECK(fh::batch_check(one, 900, 2, 800, false, 80, one, PAFC_BF16, &t_max) == PAFC_OK && t_max == 3);

    long frames = 0;
    int c_next = 0;
    CHECK(fh::stream_check(nullptr, 0, one, 500, 500, 2, false, 80, 0.f, one, PAFC_F32, 80, 0, &frames, &c_next) == PAFC_ERR_NULL_POINTER);
    CHECK(fh::stream_check(one, 0, one, 500, 500, 2, true, 80, 0.f, one, PAFC_F32, 80, 0, &frames, &c_next) == PAFC_ERR_NULL_POINTER);
    CHECK(fh::stream_check(one, 0, one, 500, 500, 0, false, 80, 0.f, one, PAFC_F32, 80, 0, &frames, &c_next) == PAFC_ERR_BAD_DIMS);
    CHECK(fh::stream_check(one, 560, one, 500, 500, 2, false, 80, 0.f, one, PAFC_F32, 80, 0, &frames, &c_next) == PAFC_ERR_BAD_DIMS);
    CHECK(fh::stream_check(one, 0, one, 500, 500, 2, false, 80, 1.f, one, PAFC_F32, 80, 0, &frames, &c_next) == PAFC_ERR_UNSUPPORTED);
    CHECK(fh::stream_check(one, 0, one, 500, 500, 2, false, 80, 0.f, one, 9, 80, 0, &frames, &c_next) == PAFC_ERR_DTYPE);
    CHECK(fh::stream_check(one, 0, nullptr, 500, 500, 2, false, 80, 0.f, one, PAFC_F32, 80, 0, &frames, &c_next) == PAFC_ERR_NULL_POINTER);
    CHECK(fh::stream_check(one, 0, one, 499, 500, 2, false, 80, 0.f, one, PAFC_F32, 80, 0, &frames, &c_next) == PAFC_ERR_BAD_DIMS);
    CHECK(fh::stream_check(one, 0, one, 500, 500, 2, false, 80, 0.f, nullptr, PAFC_F32, 80, 0, &frames, &c_next) == PAFC_ERR_NULL_POINTER);
    CHECK(fh::stream_check(one, 0, one, 500, 500, 2, false, 80, 0.f, one, PAFC_F32, 79, 0, &frames, &c_next) == PAFC_ERR_BAD_DIMS);   // row too short
    CHECK(fh::stream_check(one, 0, one, 500, 500, 2, false, 80, 0.f, one, PAFC_F32, 160, 2, &frames, &c_next) == PAFC_ERR_BAD_DIMS);  // first_frame past it
    CHECK(fh::stream_check(one, 0, one, 500, 500, 2, false, 80, 0.f, one, PAFC_F32, 240, 2, &frames, &c_next) == PAFC_OK && frames == 1 && c_next == 340);
    CHECK(fh::stream_check(one, 10, one, 100, 100, 2, false, 80, 0.f, nullptr, PAFC_F32, 0, 0, &frames, &c_next) == PAFC_OK && frames == 0 && c_next == 110);
    CHECK(fh::stream_check(one, 10, nullptr, 0, 0, 2, false, 80, 0.f, nullptr, PAFC_F32, 0, 0, &frames, &c_next) == PAFC_OK && frames == 0 && c_next == 10);

    // ragged rows of a slot pool: the host copy of the descriptor table {slot, c, n, first_frame} is read here, all of it
    long most = -1;
    bool any_new = false;
    const int rows[] = {3, 0, 1000, 0, 1, 399, 160, 7, 4, 17, 0, 3};
    CHECK(fh::stream_rows_check(one, 5, rows, one, 3, one, 2000, 2000, false, 80, 0.f, one, PAFC_BF16, 96, &most, &any_new) == PAFC_OK);
    CHECK(most == 4 && any_new);
    CHECK(fh::stream_rows_check(one, 5, rows, one, 3, one, 2000, 2000, false, 80, 0.f, nullptr, PAFC_F32, 96, &most, &any_new) == PAFC_ERR_NULL_POINTER);
    CHECK(fh::stream_rows_check(one, 5, rows, one, 3, nullptr, 2000, 2000, false, 80, 0.f, one, PAFC_F32, 96, &most, &any_new) == PAFC_ERR_NULL_POINTER);
    CHECK(fh::stream_rows_check(one, 5, nullptr, one, 3, one, 2000, 2000, false, 80, 0.f, one, PAFC_F32, 96, &most, &any_new) == PAFC_ERR_NULL_POINTER);
    CHECK(fh::stream_rows_check(one, 4, rows, one, 3, one, 2000, 2000, false, 80, 0.f, one, PAFC_F32, 96, &most, &any_new) == PAFC_ERR_BAD_DIMS);    // slot 4 of 4
    CHECK(fh::stream_rows_check(one, 5, rows, one, 3, one, 2000, 999, false, 80, 0.f, one, PAFC_F32, 96, &most, &any_new) == PAFC_ERR_BAD_DIMS);     // n > n_max
    CHECK(fh::stream_rows_check(one, 5, rows, one, 3, one, 1999, 2000, false, 80, 0.f, one, PAFC_F32, 96, &most, &any_new) == PAFC_ERR_BAD_DIMS);    // ld_chunk
    CHECK(fh::stream_rows_check(one, 5, rows, one, 3, one, 2000, 2000, false, 80, 0.f, one, PAFC_F32, 3, &most, &any_new) == PAFC_ERR_BAD_DIMS);     // 4 frames, ring of 3
    CHECK(fh::stream_rows_check(one, 5, rows, one, 3, one, 2000, 2000, false, 80, 0.5f, one, PAFC_F32, 96, &most, &any_new) == PAFC_ERR_UNSUPPORTED);
    const int twice[] = {2, 0, 100, 0, 2, 0, 100, 0};
    CHECK(fh::stream_rows_check(one, 5, twice, one, 2, one, 100, 100, false, 80, 0.f, one, PAFC_F32, 96, &most, &any_new) == PAFC_ERR_BAD_DIMS);
    const int idle[] = {0, 17, 0, 3, 4, 0, 0, 0};
    CHECK(fh::stream_rows_check(one, 5, idle, one, 2, nullptr, 0, 0, false, 80, 0.f, nullptr, PAFC_F32, 96, &most, &any_new) == PAFC_OK && !any_new && most == 0);
    const int grow[] = {1, 100, 50, 9};                                              // no frame: the carry update alone, no out needed
    CHECK(fh::stream_rows_check(one, 5, grow, one, 1, one, 50, 50, false, 80, 0.f, nullptr, PAFC_F32, 96, &most, &any_new) == PAFC_OK && any_new && most == 0);

    std::puts("fbank host check ok");
    return 0;
}
