// flock_amd/csrc/textenc.hpp on the CPU: the byte classes of all 256 bytes in each of a dword's four positions -- and, for CSV, under every delimiter --
// against a naive switch; what a byte becomes in a JSON string against a table written out by hand; the per-value extra-byte formulas against a byte loop
// on pseudo-random values; the row-length formula against strlen of a row built naively with snprintf.
// Prints "textenc_test: ok <checks>" and exits 0, or the first difference and exits 1.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "textenc.hpp"

using namespace flockgpu;

static long g_checks = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        ++g_checks;                       \
        if (!(cond)) {                    \
            std::printf("textenc_test: "); \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            return 1;                     \
        }                                 \
    } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_state ^= g_state << 13;
    g_state ^= g_state >> 7;
    g_state ^= g_state << 17;
    return g_state;
}

// the rules, naively
static int naive_json_extra(unsigned b) {
    switch (b) {
        case '"': case '\\': case 0x08: case 0x0C: case 0x0A: case 0x0D: case 0x09: return 1;
        default: return b < 0x20 ? 5 : 0;
    }
}
static std::string naive_json_byte(unsigned b) {
    switch (b) {
        case '"': return "\\\"";
        case '\\': return "\\\\";
        case 0x08: return "\\b";
        case 0x0C: return "\\f";
        case 0x0A: return "\\n";
        case 0x0D: return "\\r";
        case 0x09: return "\\t";
        default: break;
    }
    if (b < 0x20) {
        char buf[8];
        std::snprintf(buf, sizeof buf, "\\u%04x", b);
        return buf;
    }
    return std::string(1, (char)b);
}
static bool naive_csv_special(unsigned b, unsigned delim) {
    switch (b) {
        case '"': case '\n': case '\r': return true;
        default: return b == delim;
    }
}

static std::string naive_json_value(const std::string &s) {
    std::string o = "\"";
    for (unsigned char ch : s) o += naive_json_byte(ch);
    return o + "\"";
}
static std::string naive_csv_value(const std::string &s, unsigned delim) {
    bool quote = s.empty();
    for (unsigned char ch : s) quote = quote || naive_csv_special(ch, delim);
    if (!quote) return s;
    std::string o = "\"";
    for (unsigned char ch : s) {
        o += (char)ch;
        if (ch == '"') o += '"';
    }
    return o + "\"";
}

static int check_classes() {
    for (unsigned b = 0; b < 256; ++b) {
        CHECK((int)textenc::json_extra(b) == naive_json_extra(b), "json_extra(0x%02x) = %u", b, textenc::json_extra(b));
        CHECK(textenc::json_is_class(b) == (naive_json_extra(b) != 0) && textenc::json_is_long(b) == (naive_json_extra(b) == 5), "json class of 0x%02x", b);
        uint8_t out[6];
        const uint32_t n = textenc::json_escape(b, out);
        CHECK(std::string(reinterpret_cast<char *>(out), n) == naive_json_byte(b), "json_escape(0x%02x)", b);
        for (int k = 0; k < 4; ++k) {
            for (unsigned other : {0x61u, 0x00u, 0x22u, 0xFFu, 0x1Fu, 0x20u}) {   // the neighbours must not leak into byte k's bit
                const uint32_t w = (0x01010101u * other & ~(0xFFu << (8 * k))) | (b << (8 * k));
                uint32_t cls, lng;
                textenc::json_class4(w, &cls, &lng);
                uint32_t want_cls = 0, want_lng = 0;
                for (int j = 0; j < 4; ++j) {
                    const unsigned x = j == k ? b : other;
                    want_cls |= (naive_json_extra(x) != 0 ? 1u : 0u) << j;
                    want_lng |= (naive_json_extra(x) == 5 ? 1u : 0u) << j;
                }
                CHECK(cls == want_cls && lng == want_lng, "json_class4(0x%08x) = %x / %x, want %x / %x", w, cls, lng, want_cls, want_lng);
            }
        }
    }
    for (unsigned delim = 0; delim < 128; ++delim) {
        if (delim == '"' || delim == '\r' || delim == '\n') continue;
        for (unsigned b = 0; b < 256; ++b) {
            CHECK(textenc::csv_is_special(b, delim) == naive_csv_special(b, delim), "csv_is_special(0x%02x, 0x%02x)", b, delim);
            for (int k = 0; k < 4; ++k) {
                const unsigned other = k & 1 ? 0x61u : delim;
                const uint32_t w = (0x01010101u * other & ~(0xFFu << (8 * k))) | (b << (8 * k));
                uint32_t quo, spc, want_quo = 0, want_spc = 0;
                textenc::csv_class4(w, delim, &quo, &spc);
                for (int j = 0; j < 4; ++j) {
                    const unsigned x = j == k ? b : other;
                    want_quo |= (x == '"' ? 1u : 0u) << j;
                    want_spc |= (naive_csv_special(x, delim) ? 1u : 0u) << j;
                }
                CHECK(quo == want_quo && spc == want_spc, "csv_class4(0x%08x, 0x%02x) = %x / %x, want %x / %x", w, delim, quo, spc, want_quo, want_spc);
            }
        }
    }
    return 0;
}

// a pseudo-random value over an alphabet that is rich in class bytes
static std::string random_value() {
    static const unsigned char alphabet[] = {',', '|', '"', '\n', '\r', '\\', '\t', 0x00, 0x08, 0x0C, 0x1F, 0x7F, '/', 0xC3, 0xA9, 0xF0, 0x9F, 'a', 'b', 'c', ' ', '0', '9'};
    const size_t len = rnd() % 41;
    const bool plain = rnd() % 3 == 0;
    std::string s;
    for (size_t i = 0; i < len; ++i) s += (char)(plain ? 'a' + rnd() % 26 : alphabet[rnd() % sizeof alphabet]);
    return s;
}

// the value's class counts through the dword masks, as the class pass takes them (the tail of the last dword padded and masked off)
static void counts_of(const std::string &s, TextFormat f, unsigned delim, uint32_t *a, uint32_t *b) {
    *a = *b = 0;
    for (size_t i = 0; i < s.size(); i += 4) {
        uint32_t w = 0, live = 0;
        for (size_t k = 0; k < 4 && i + k < s.size(); ++k) {
            w |= (uint32_t)(unsigned char)s[i + k] << (8 * k);
            live |= 1u << k;
        }
        uint32_t x, y;
        if (f == TextFormat::Json) textenc::json_class4(w, &x, &y);
        else textenc::csv_class4(w, delim, &x, &y);
        *a += (uint32_t)__builtin_popcount(x & live);
        *b += (uint32_t)__builtin_popcount(y & live);
    }
}

static int check_values() {
    for (int it = 0; it < 20000; ++it) {
        const std::string s = random_value();
        const unsigned delim = it & 1 ? '|' : ',';
        uint32_t a, b;
        counts_of(s, TextFormat::Json, 0, &a, &b);
        const uint32_t jx = textenc::json_extra_of(a, b);
        uint32_t loop = 0;
        for (unsigned char ch : s) loop += (uint32_t)naive_json_extra(ch);
        CHECK(jx == loop, "json extra of a value of %zu bytes: %u, a byte loop says %u", s.size(), jx, loop);
        CHECK(textenc::json_utf8_len((uint32_t)s.size(), jx) == naive_json_value(s).size(), "json_utf8_len");
        CHECK(textenc::utf8_len(TextFormat::Json, true, (uint32_t)s.size(), jx) == naive_json_value(s).size() && textenc::utf8_len(TextFormat::Json, false, 7, 3) == 4, "utf8_len json");
        counts_of(s, TextFormat::Csv, delim, &a, &b);
        const uint32_t cx = textenc::csv_extra_of(a, b);
        const std::string want = naive_csv_value(s, delim);
        CHECK(textenc::csv_utf8_len((uint32_t)s.size(), cx) == want.size(), "csv_utf8_len of a value of %zu bytes: %llu, built naively %zu", s.size(),
              (unsigned long long)textenc::csv_utf8_len((uint32_t)s.size(), cx), want.size());
        CHECK(textenc::csv_utf8_quoted((uint32_t)s.size(), cx) == (want.size() != s.size() || s.empty()), "csv_utf8_quoted");
        CHECK(textenc::utf8_len(TextFormat::Csv, false, 7, 3) == 0, "a NULL is an empty field");
    }
    return 0;
}

// one row of (Int32, Int64, UInt64, Timestamp(ms), Utf8) built naively against the formulas
static int check_rows() {
    const char *names[5] = {"a", "we\"ird,name", "u", "t", "s"};
    const int32_t types[5] = {kTextInt32, kTextInt64, kTextUInt64, kTextTimestampMs, kTextUtf8};
    const int64_t edge[] = {0, -1, 1, 9, 10, -10, INT32_MIN, INT32_MAX, INT64_MIN, INT64_MAX, kNumTextTsMin, kNumTextTsMax, 999, 1000};
    for (int it = 0; it < 4000; ++it) {
        for (int fmt = 0; fmt < 2; ++fmt) {
            const TextFormat f = fmt ? TextFormat::Csv : TextFormat::Json;
            const int n_cols = it % 7 == 0 ? 1 : 5;
            const int first = n_cols == 1 ? it % 5 : 0;
            std::string row;
            uint64_t pre = 0, vals = 0;
            for (int c = 0; c < n_cols; ++c) {
                const int t = first + c;
                std::string p;
                if (f == TextFormat::Json) p = std::string(c ? "," : "{") + naive_json_value(names[t]) + ":";
                else if (c) p = ",";
                pre += p.size();
                row += p;
                const bool valid = rnd() % 5 != 0;
                uint64_t bits = it % 3 == 0 ? (uint64_t)edge[rnd() % (sizeof edge / sizeof *edge)] : rnd() >> (rnd() % 64);
                char buf[40] = "";
                std::string text;
                if (types[t] == kTextUtf8) {
                    const std::string s = random_value();
                    uint32_t a, b;
                    counts_of(s, f, ',', &a, &b);
                    const uint32_t extra = f == TextFormat::Json ? textenc::json_extra_of(a, b) : textenc::csv_extra_of(a, b);
                    vals += textenc::utf8_len(f, valid, (uint32_t)s.size(), extra);
                    text = !valid ? (fmt ? "" : "null") : fmt ? naive_csv_value(s, ',') : naive_json_value(s);
                } else {
                    if (types[t] == kTextInt32) bits = (uint64_t)(int64_t)(int32_t)bits;
                    if (types[t] == kTextTimestampMs) bits = (uint64_t)(kNumTextTsMin + (int64_t)(bits % (uint64_t)(kNumTextTsMax - kNumTextTsMin + 1)));
                    vals += textenc::num_len(f, types[t], valid, bits);
                    if (types[t] == kTextUInt64) {
                        std::snprintf(buf, sizeof buf, "%" PRIu64, bits);
                    } else if (types[t] == kTextTimestampMs && fmt) {
                        const NumText<6> x = numtext_ts((int64_t)bits);   // (the layout itself is numtext_test's to check; here: the LENGTH)
                        for (uint32_t i = 0; i < x.len; ++i) buf[i] = (char)numtext_byte(x, i);
                    } else {
                        std::snprintf(buf, sizeof buf, "%" PRId64, (int64_t)bits);
                    }
                    text = !valid ? (fmt ? "" : "null") : buf;
                }
                row += text;
            }
            if (f == TextFormat::Json) row += "}\n";
            else row += row.empty() ? "\"\"\n" : "\n";
            CHECK(textenc::row_len(f, pre, vals) == std::strlen(row.c_str()) || row.find('\0') != std::string::npos, "row_len(%d): %llu, the row built naively has %zu bytes: %s", fmt,
                  (unsigned long long)textenc::row_len(f, pre, vals), row.size(), row.c_str());
            CHECK(textenc::row_len(f, pre, vals) == row.size(), "row_len(%d): %llu against %zu bytes", fmt, (unsigned long long)textenc::row_len(f, pre, vals), row.size());
        }
    }
    return 0;
}

int main() {
    if (check_classes() || check_values() || check_rows()) return 1;
    std::printf("textenc_test: ok %ld\n", g_checks);
    return 0;
}
