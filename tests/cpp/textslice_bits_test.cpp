// Host check of flock_amd/csrc/textslice_bits.hpp: the class masks of a chunk against a byte-by-byte loop, select64 / highest64 / clip_word against a
// bit-by-bit loop, and the k-th set bit of a row that spans several words the way the streaming kernel composes it (popcount per word, select inside).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "textslice_bits.hpp"

using namespace flockgpu::slicebits;

static uint64_t state = 0x9e3779b97f4a7c15ull;
static uint64_t next() {
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return state;
}

static int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            if (failures++ < 10) std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); \
        }                                                               \
    } while (0)

static int naive_select(uint64_t x, int k) {
    for (int b = 0; b < 64; ++b)
        if ((x >> b) & 1u) {
            if (k == 0) return b;
            --k;
        }
    return 64;
}

int main() {
    // select64 / highest64: every single bit, all ones, sparse and dense random words, every k
    std::vector<uint64_t> words = {0, 1, ~uint64_t(0), uint64_t(1) << 63, 0x8000000000000001ull, 0x00000000ffffffffull, 0xffffffff00000000ull, 0x5555555555555555ull};
    for (int b = 0; b < 64; ++b) words.push_back(uint64_t(1) << b);
    for (int i = 0; i < 20000; ++i) {
        uint64_t x = next();
        if (i % 3 == 1) x &= next() & next();
        if (i % 3 == 2) x |= next() | next();
        words.push_back(x);
    }
    for (uint64_t x : words) {
        const int pc = popcount64(x);
        int naive_pc = 0;
        for (int b = 0; b < 64; ++b) naive_pc += (int)((x >> b) & 1u);
        CHECK(pc == naive_pc);
        for (int k = -1; k <= 64; ++k) CHECK(select64(x, k) == (k < 0 ? 64 : naive_select(x, k)));
        if (x) {
            int hi = 63;
            while (!((x >> hi) & 1u)) --hi;
            CHECK(highest64(x) == hi);
        }
    }
    // clip_word: every (a, b) against a bit loop, for words at lo = 0 and lo = 128
    for (int rep = 0; rep < 40; ++rep) {
        const uint64_t x = rep == 0 ? ~uint64_t(0) : next();
        for (int64_t lo : {int64_t(0), int64_t(128)})
            for (int64_t a = lo - 3; a < lo + 64; ++a)
                for (int64_t b = (a < lo ? lo : a) + 1; b <= lo + 70; ++b) {
                    uint64_t want = 0;
                    for (int64_t p = lo; p < lo + 64; ++p)
                        if (p >= a && p < b) want |= x & (uint64_t(1) << (p - lo));
                    CHECK(clip_word(x, lo, a, b) == want);
                }
    }
    // the masks of a chunk: random bytes biased towards the delimiter, the set's characters and every UTF-8 byte class
    AsciiSet set{0, 0};
    const char *chars = " \t,x~\x7f";
    for (const char *c = chars; *c; ++c) ascii_set_add(set, (uint8_t)*c);
    ascii_set_add(set, 0);
    for (uint32_t c = 0; c < 256; ++c) CHECK(ascii_set_has(set, c) == (c == 0 || (c < 128 && c != 0 && std::strchr(chars, (int)c) != nullptr)));
    const uint8_t pool[] = {' ', '\t', ',', 'x', '~', 0x7f, 0, 'a', '/', 0x80, 0xbf, 0xc3, 0xe2, 0xf0, 0xff, 0xa9};
    for (int rep = 0; rep < 200000; ++rep) {
        uint8_t bytes[16];
        for (auto &b : bytes) b = (next() & 3) ? pool[next() % sizeof(pool)] : (uint8_t)next();
        uint32_t w[4];
        std::memcpy(w, bytes, 16);   // (little-endian, as the kernel's dwords)
        const uint8_t delim = (rep & 1) ? pool[next() % sizeof(pool)] : (uint8_t)next();
        uint32_t lead = 0, equal = 0, outside = 0;
        for (int k = 0; k < 16; ++k) {
            lead |= (uint32_t)((bytes[k] & 0xc0) != 0x80) << k;
            equal |= (uint32_t)(bytes[k] == delim) << k;
            outside |= (uint32_t)!ascii_set_has(set, bytes[k]) << k;
        }
        CHECK(chunk_mask<kLead>(w[0], w[1], w[2], w[3], delim, set) == lead);
        CHECK(chunk_mask<kEqual>(w[0], w[1], w[2], w[3], delim, set) == equal);
        CHECK(chunk_mask<kOutside>(w[0], w[1], w[2], w[3], delim, set) == outside);
    }
    // the k-th set bit of a range over several words, as the row pass composes it
    for (int rep = 0; rep < 3000; ++rep) {
        uint64_t m[6];
        for (auto &x : m) x = (rep % 4 == 0) ? next() & next() & next() : next();
        const int64_t a = (int64_t)(next() % 300), b = a + 1 + (int64_t)(next() % (384 - a));
        std::vector<int64_t> pos;
        for (int64_t p = a; p < b; ++p)
            if ((m[p >> 6] >> (p & 63)) & 1u) pos.push_back(p);
        for (uint32_t target = 0; target <= pos.size() + 2; ++target) {
            uint32_t c = 0;
            int64_t found = -1, last = -1;
            for (int w = (int)(a >> 6); w <= (int)((b - 1) >> 6); ++w) {
                const int64_t lo = (int64_t)w << 6;
                const uint64_t x = clip_word(m[w], lo, a, b);
                const uint32_t p = (uint32_t)popcount64(x);
                if (target - c - 1u < p) found = lo + select64(x, (int)(target - c - 1u));
                if (x) last = lo + highest64(x);
                c += p;
            }
            CHECK(c == pos.size());
            CHECK(found == (target >= 1 && target <= pos.size() ? pos[target - 1] : -1));
            CHECK(last == (pos.empty() ? -1 : pos.back()));
        }
    }
    if (failures) {
        std::printf("textslice_bits_test: %d checks FAILED\n", failures);
        return 1;
    }
    std::printf("textslice_bits_test: ok\n");
    return 0;
}
