// The host side of the dead-read rule and of the streamed loop's bookkeeping (pyspecsdr_amd/csrc/pss_live.h) as a stand-alone program for
// the host sanitizers — the code is plain C++ and never sees a GPU:
//     g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/check_live_host.cpp -o check_live_host && ./check_live_host
// The cases are those of tests/test_live_frames.py: frames of 1, 2, 3, 29, 1024 and 1025 samples, all +0.0 / -0.0 / mixed, one live word
// (1.0, +-denormal, NaN, inf) at the first and last five word positions and at words 127 / 128 / 129, batches of 0, 1, 255, 256, 257 frames,
// the index list's tail left alone, frames at an address that is only byte-aligned.  Each is compared with a float comparison (x == 0).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../pyspecsdr_amd/csrc/pss_live.h"

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);       \
            failures++;                                                 \
        }                                                               \
    } while (0)

static void run(const std::vector<uint32_t> &words, long nf, int n, size_t byte_offset)
{
    // exactly-sized heap blocks: a read or write past either end is the sanitizer's to find
    std::vector<unsigned char> raw(words.size() * 4 + byte_offset);
    if (!words.empty()) memcpy(raw.data() + byte_offset, words.data(), words.size() * 4);
    const float *iq = reinterpret_cast<const float *>(raw.data() + byte_offset);
    std::vector<uint8_t> live((size_t)nf, 9);
    std::vector<int32_t> idx((size_t)nf, -7);
    const long count = pss_live::live_frames(iq, nf, n, live.data(), idx.data());
    long want = 0;
    for (long f = 0; f < nf; f++) {
        bool any = false;
        for (int w = 0; w < 2 * n; w++) {
            float x;
            memcpy(&x, &words[(size_t)f * 2 * n + w], 4);
            any = any || !(x == 0.0f);
        }
        CHECK(live[f] == (any ? 1 : 0));
        if (any) {
            CHECK(want < nf && idx[want] == (int32_t)f);
            want++;
        }
    }
    CHECK(count == want);
    for (long k = want; k < nf; k++) CHECK(idx[k] == -7);
    CHECK(pss_live::live_frames(iq, nf, n, nullptr, nullptr) == want);
}

int main()
{
    const int lengths[] = {1, 2, 3, 29, 1024, 1025};
    const uint32_t kinds[] = {0x3f800000u, 0x00000001u, 0x80000001u, 0x7fc00000u, 0x7f800000u};
    for (int n : lengths) {
        const int words = 2 * n;
        std::vector<int> pos;
        for (int p = 0; p < words; p++)
            if (p < 5 || p >= words - 5 || (p >= 127 && p <= 129)) pos.push_back(p);
        for (int fill = 0; fill < 3; fill++) {
            auto zero = [&](long f, int w) { return fill == 0 ? 0u : fill == 1 ? 0x80000000u : (((w & 1) ^ (f & 1)) ? 0x80000000u : 0u); };
            const long nf = 2 * (long)pos.size() + 1;
            std::vector<uint32_t> buf((size_t)nf * words);
            for (long f = 0; f < nf; f++)
                for (int w = 0; w < words; w++) buf[(size_t)f * words + w] = zero(f, w);
            run(buf, nf, n, 0);   // all dead
            for (uint32_t bits : kinds) {
                std::vector<uint32_t> b2 = buf;
                for (size_t j = 0; j < pos.size(); j++) b2[(2 * j + 1) * words + pos[j]] = bits;
                run(b2, nf, n, 0);
                run(b2, nf, n, 1);   // any address
            }
        }
    }
    unsigned seed = 5;
    for (long nf : {0L, 1L, 255L, 256L, 257L}) {
        std::vector<uint32_t> buf((size_t)nf * 6, 0u);
        for (long f = 0; f < nf; f++) {
            seed = seed * 1664525u + 1013904223u;
            if (seed >> 31) buf[(size_t)f * 6 + (seed >> 8) % 6] = 1u;
        }
        run(buf, nf, 3, 0);
    }
    // the cursor between chunks: dead frames advance nothing, the phase follows the live frames alone
    pss_live::Cursor c;
    c.held = -3.0, c.phase = 1;
    c.advance(8, 5, -20.0, 3);
    CHECK(c.n_live == 8 && c.n_open == 5 && c.held == -20.0 && c.phase == 0);
    c.advance(0, 0, c.held, 3);
    CHECK(c.n_live == 8 && c.n_open == 5 && c.held == -20.0 && c.phase == 0);
    c.advance(5, 5, 1.5, 0);
    CHECK(c.n_live == 13 && c.n_open == 10 && c.held == 1.5 && c.phase == 0);
    c.phase = 2;
    c.advance(2147483647L, 0, 0.0, 3);   // the phase is reduced in `long`: no int overflow
    CHECK(c.phase == (2 + 2147483647L) % 3);
    std::printf(failures ? "%d checks failed\n" : "live-frame host checks passed\n", failures);
    return failures ? 1 : 0;
}
