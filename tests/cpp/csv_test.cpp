// flock_amd/csrc/csv.hpp on the CPU (g++ with the address and undefined-behaviour sanitizers): the field walk over a table of records -- every quote rule
// of A-CSV2, the failures, the unquoting copy -- the Float64 conversion of A-CSV5 against strtod over the exact range (significands up to 2^53, every
// exponent from -22 to 22, points and zeros in every place) and its refusals one step outside, and the nine-digit fraction of A-CSV4.  Every text lies
// in a heap buffer of exactly its own size: a read past a record or a value is a sanitizer finding.
// Prints "csv_test: ok <checks>" and exits 0, or the first difference and exits 1.
#include <algorithm>
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "csv.hpp"

using namespace flockgpu;

static long g_checks = 0;

#define CHECK(cond, ...)              \
    do {                              \
        ++g_checks;                   \
        if (!(cond)) {                \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            return 1;                 \
        }                             \
    } while (0)

struct Exact {   // the bytes of `s` in a buffer of their own size
    std::vector<uint8_t> b;
    explicit Exact(const std::string &s) : b(s.begin(), s.end()) {}
    const uint8_t *p() const { return b.data(); }
    int32_t n() const { return (int32_t)b.size(); }
};

// the whole record walked as csv.hip's lane walks it: the unquoted fields joined by 0x1F, or "!<code>@<column>"
static std::string walk(const std::string &record, char delim) {
    const Exact x(record);
    std::string out;
    int32_t p = 0;
    for (int f = 0;; ++f) {
        CsvField fl;
        const uint32_t rc = csv_next_field(x.p(), p, x.n(), (uint32_t)(uint8_t)delim, &fl);
        if (rc != kCsvOk) return "!" + std::to_string(rc) + "@" + std::to_string(f);
        std::vector<uint8_t> v((size_t)fl.ulen);
        if (fl.dq) {
            if (csv_unquote(x.p(), fl.begin, fl.end, v.data()) != fl.ulen) return "!unquote@" + std::to_string(f);
        } else {
            if (fl.end - fl.begin != fl.ulen) return "!ulen@" + std::to_string(f);
            if (fl.ulen) std::memcpy(v.data(), x.p() + fl.begin, (size_t)fl.ulen);
        }
        if (f) out.push_back('\x1f');
        out.append(v.begin(), v.end());
        if (fl.next >= x.n()) return out;
        p = fl.next + 1;
    }
}

static int test_walk() {
    struct Row { const char *record; char delim; const char *want; };
    const Row rows[] = {
        {"a,b,c", ',', "a\x1f" "b\x1f" "c"},
        {"a", ',', "a"},
        {"", ',', ""},
        {",", ',', "\x1f"},
        {"a,,", ',', "a\x1f\x1f"},
        {"\"\"", ',', ""},
        {"\"\",\"\"", ',', "\x1f"},
        {"\"a,b\",c", ',', "a,b\x1f" "c"},
        {"\"say \"\"hi\"\"\",x", ',', "say \"hi\"\x1fx"},
        {"\"\"\"\"", ',', "\""},
        {"\"\"\"\"\"\"", ',', "\"\""},
        {"\"line\nbreak\",\"cr\r\nlf\"", ',', "line\nbreak\x1f" "cr\r\nlf"},
        {"1|x y|2.5|", '|', "1\x1fx y\x1f" "2.5\x1f"},
        {"a\t\"b\tc\"", '\t', "a\x1f" "b\tc"},
        {"a,b|c", '|', "a,b\x1f" "c"},
        {" \"a\"", ',', "!3@0"},              // a quote that does not BEGIN the field
        {"ab\"c,d", ',', "!3@0"},
        {"x,a\rb", ',', "!2@1"},
        {"\"a\"b,c", ',', "!4@0"},
        {"x,\"a\" ,c", ',', "!4@1"},
        {"x,\"a\"\r", ',', "!4@1"},
        {"\"abc", ',', "!5@0"},
        {"x,y,\"abc\"\"", ',', "!5@2"},
        {"\"", ',', "!5@0"},
        {"x,\"", ',', "!5@1"},
    };
    for (const Row &r : rows) {
        const std::string got = walk(r.record, r.delim);
        CHECK(got == r.want, "walk(%s): got '%s', want '%s'", r.record, got.c_str(), r.want);
    }
    return 0;
}

static bool f64(const std::string &s, double *out) {
    const Exact x(s);
    return csv_f64(x.p(), x.n(), out);
}

static int check_f64_exact(const std::string &s) {
    double got = 0.0;
    CHECK(f64(s, &got), "csv_f64 refuses '%s' inside the exact range", s.c_str());
    const double want = std::strtod(s.c_str(), nullptr);
    CHECK(std::memcmp(&got, &want, sizeof got) == 0, "csv_f64('%s') = %.17g, strtod gives %.17g", s.c_str(), got, want);
    uint64_t bits = 0;
    const Exact x(s);
    CHECK(csv_value(kCsvFloat64, x.p(), x.n(), &bits) == kCsvOk && std::memcmp(&bits, &want, sizeof bits) == 0, "csv_value(Float64, '%s')", s.c_str());
    return 0;
}

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return g_rng;
}

static int test_f64() {
    const uint64_t top = uint64_t(1) << 53;
    std::vector<uint64_t> ws = {0, 1, 2, 9, 10, 15, 123, 1000, 999999, top, top - 1, top - 2, 4503599627370497ull, 7403891444206238ull, 4071835519823214ull};
    for (int i = 0; i < 3000; ++i) ws.push_back(rnd() % (top + 1));
    for (int i = 0; i < 1000; ++i) ws.push_back(rnd() % 1000000);
    for (uint64_t w : ws) {
        if (w && w % 10 == 0) ++w;   // (zeros at the significand's end move the exponent: they have their own texts below)
        const std::string d = std::to_string(w);
        for (int e = -22; e <= 22; ++e) {
            const std::string es = std::to_string(e);
            if (check_f64_exact(d + "e" + es) || check_f64_exact("-" + d + "E" + (e >= 0 ? "+" : "") + es)) return 1;
        }
        // the point in every place, zeros in front and behind; the folded exponent stays in range
        for (size_t cut = 0; cut <= d.size(); ++cut) {
            const std::string whole = cut == d.size() ? "0" : d.substr(0, d.size() - cut), frac = cut == 0 ? "0" : d.substr(d.size() - cut);
            if (check_f64_exact(whole + "." + frac) || check_f64_exact("+00" + whole + "." + frac + "000")) return 1;
            if (check_f64_exact(whole + "." + frac + "e" + std::to_string(-22 + (int)cut)) || check_f64_exact(whole + "." + frac + "e22")) return 1;
        }
        if (check_f64_exact(d) || check_f64_exact("0." + std::string(22 - std::min<size_t>(22, d.size()), '0') + d)) return 1;
        // trailing zeros are folded into the exponent
        if (w % 10) {
            if (check_f64_exact(d + std::string(22, '0')) || check_f64_exact(d + "000e19") || check_f64_exact(d + "0000000000.0000e-32")) return 1;
        }
    }
    for (const char *s : {"0", "-0", "0.0", "-0.000", "0e999", "-0e-999", "000", "8.5", "3e-1", "0.3", "1e22", "1E-22", "9007199254740992e22", "1234567890123450000000"})
        if (check_f64_exact(s)) return 1;
    double got = 0.0;
    CHECK(f64("-0", &got) && std::signbit(got) && got == 0.0, "-0 is minus zero");
    for (const char *s : {"", "+", "-", ".", "1.", ".5", "e5", "1e", "1e+", "1e-", "1.e5", "1.5.2", "1e5.0", "1e5e5", "--1", "+-1", " 1", "1 ", "1_0", "0x10", "0x1p3", "inf", "-inf",
                          "nan", "NaN", "Infinity", "1,5", "1d5", "9007199254740993", "90071992547409920.1", "123456789012345678", "1e23", "1e-23", "9007199254740992e23",
                          "10e22", "0.1e-22", "4.9e-324", "1e308", "1e400", "100000000000000000000000", "0.00000000000000000000001", "1e99999999999999999999",
                          "1e-99999999999999999999"}) {
        CHECK(!f64(s, &got), "csv_f64 takes '%s'", s);
        const Exact x(s);
        uint64_t bits = 0;
        if (x.n()) CHECK(csv_value(kCsvFloat64, x.p(), x.n(), &bits) == kCsvErrFloat, "csv_value(Float64, '%s')", s);
    }
    return 0;
}

static int test_ts_and_ints() {
    struct Row { const char *s; bool ok; int64_t ms; };
    const Row rows[] = {
        {"2020-11-01 00:11:32.6250", true, 1604189492625ll},
        {"2020-11-01 00:11:32.625", true, 1604189492625ll},
        {"2020-11-01 00:11:32.62", true, 1604189492620ll},
        {"2020-11-01 00:11:32.6", true, 1604189492600ll},
        {"2020-11-01 00:11:32", true, 1604189492000ll},
        {"2020-11-01T00:11:32.123456789", true, 1604189492123ll},
        {"2020-11-01 00:11:32.99999", true, 1604189492999ll},
        {"1969-12-31 23:59:59.999999999", true, -1ll},
        {"2020-11-01", true, 1604188800000ll},
        {"2020-11-01 00:11:32.1234567890", false, 0},
        {"2020-11-01 00:11:32.12x4", false, 0},
        {"2020-11-01 00:11:32.1234 ", false, 0},
        {"2020-11-01 00:11:3.212345", false, 0},
        {"2020-11-01 00:11:32:1234", false, 0},
        {"2020-11-01 00:11:32.", false, 0},
        {"2020-13-01 00:11:32.6250", false, 0},
        {"2020-02-30 00:00:00.0000", false, 0},
        {"2020-11-01 00:11", true, 1604189460000ll},
    };
    for (const Row &r : rows) {
        const Exact x(r.s);
        int64_t ms = 0;
        const bool ok = csv_ts(x.p(), x.n(), &ms);
        CHECK(ok == r.ok && (!ok || ms == r.ms), "csv_ts('%s'): %d %lld", r.s, (int)ok, (long long)ms);
        uint64_t bits = 0;
        CHECK((csv_value(kCsvTimestampMs, x.p(), x.n(), &bits) == kCsvOk) == r.ok && (!r.ok || (int64_t)bits == r.ms), "csv_value(Timestamp, '%s')", r.s);
    }
    struct IntRow { int32_t type; const char *s; bool ok; uint64_t bits; };
    const IntRow ints[] = {
        {kCsvInt32, "2147483647", true, 2147483647ull}, {kCsvInt32, "2147483648", false, 0}, {kCsvInt32, "-2147483648", true, (uint64_t)-2147483648ll},
        {kCsvInt32, "+7", true, 7}, {kCsvInt64, "-9223372036854775808", true, 0x8000000000000000ull}, {kCsvInt64, "9223372036854775808", false, 0},
        {kCsvUInt64, "18446744073709551615", true, ~0ull}, {kCsvUInt64, "18446744073709551616", false, 0}, {kCsvUInt64, "-0", false, 0},
        {kCsvInt32, "0000000000000000000000000000000000000042", true, 42}, {kCsvInt64, "1.0", false, 0}, {kCsvInt32, "1 ", false, 0}, {kCsvInt32, "-", false, 0},
    };
    for (const IntRow &r : ints) {
        const Exact x(r.s);
        uint64_t bits = 0;
        const uint32_t rc = csv_value(r.type, x.p(), x.n(), &bits);
        CHECK((rc == kCsvOk) == r.ok && (rc == kCsvOk || rc == kCsvErrValue) && (!r.ok || bits == r.bits), "csv_value(%d, '%s'): %u %" PRIu64, r.type, r.s, rc, bits);
    }
    return 0;
}

int main() {
    if (test_walk() || test_f64() || test_ts_and_ints()) return 1;
    std::printf("csv_test: ok %ld\n", g_checks);
    return 0;
}
