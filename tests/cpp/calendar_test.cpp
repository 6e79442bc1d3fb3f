// flock_amd/csrc/calendar.hpp on the CPU: every day from 1600-01-01 to 2400-12-31 against a from-scratch day count (walking the calendar day by day
// with the Gregorian leap rule), the round trip days -> civil -> days, every unit of date_trunc / date_part on each of those days, and +-1 ms around
// each day, month and year boundary.  Prints "ok <days>" and exits 0, or the first difference and exits 1.
#include <cstdio>
#include <cstdlib>

#include "calendar.hpp"

using namespace flockgpu::cal;

static bool leap(int y) { return (y % 4 == 0 && y % 100 != 0) || y % 400 == 0; }
static int month_days(int y, int m) {
    static const int d[] = {31, 28, 31, 30, 31, 30, 31, 31, 30, 31, 30, 31};
    return m == 2 && leap(y) ? 29 : d[m - 1];
}
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            std::printf(__VA_ARGS__);     \
            std::printf("\n");            \
            return 1;                     \
        }                                 \
    } while (0)

int main() {
    // days of 1600-01-01 since 1970-01-01, counted year by year
    int64_t day = 0;
    for (int y = 1969; y >= 1600; --y) day -= leap(y) ? 366 : 365;
    // 1970-01-01 was a Thursday (Sunday = 0: 4); walk the weekday along
    int dow = (int)(((day % 7) + 7 + 4) % 7);
    int64_t n = 0, week_start = 0;
    bool have_week = false;
    for (int y = 1600; y <= 2400; ++y) {
        const int64_t year_start = day;
        int doy = 1;
        for (int m = 1; m <= 12; ++m) {
            const int64_t month_start = day;
            for (int d = 1; d <= month_days(y, m); ++d, ++day, ++doy, dow = (dow + 1) % 7, ++n) {
                if (dow == 1 || !have_week) {   // a Monday begins a week (the first days before the first Monday: found by walking back)
                    week_start = day - ((dow + 6) % 7);
                    have_week = true;
                }
                const Civil c = civil_from_days(day);
                CHECK(c.year == y && c.month == m && c.day == d, "civil_from_days(%lld) = %lld-%d-%d, want %d-%d-%d", (long long)day, (long long)c.year, c.month, c.day, y, m, d);
                CHECK(days_from_civil(y, m, d) == day, "days_from_civil(%d-%d-%d) = %lld, want %lld", y, m, d, (long long)days_from_civil(y, m, d), (long long)day);
                const int64_t ms0 = day * kMsPerDay;
                // three moments of the day: its first millisecond, 13:47:09.123 and its last millisecond -- the day before's last one is this loop's previous turn
                const int64_t at[3] = {ms0, ms0 + 13 * kMsPerHour + 47 * kMsPerMinute + 9 * kMsPerSecond + 123, ms0 + kMsPerDay - 1};
                const int hh[3] = {0, 13, 23}, mm[3] = {0, 47, 59}, ss[3] = {0, 9, 59}, frac[3] = {0, 123, 999};
                for (int k = 0; k < 3; ++k) {
                    const int64_t t = at[k];
                    CHECK(date_part_rt(Year, t) == y && date_part_rt(Month, t) == m && date_part_rt(Day, t) == d, "date_part y/m/d at %lld", (long long)t);
                    CHECK(date_part_rt(Hour, t) == hh[k] && date_part_rt(Minute, t) == mm[k] && date_part_rt(Second, t) == ss[k], "date_part h/m/s at %lld", (long long)t);
                    CHECK(date_part_rt(Dow, t) == dow, "dow at %lld = %d, want %d", (long long)t, date_part_rt(Dow, t), dow);
                    CHECK(date_part_rt(Doy, t) == doy, "doy at %lld = %d, want %d", (long long)t, date_part_rt(Doy, t), doy);
                    CHECK(date_trunc_rt(Second, t) == t - frac[k], "trunc second at %lld", (long long)t);
                    CHECK(date_trunc_rt(Minute, t) == t - frac[k] - ss[k] * kMsPerSecond, "trunc minute at %lld", (long long)t);
                    CHECK(date_trunc_rt(Hour, t) == ms0 + hh[k] * kMsPerHour, "trunc hour at %lld", (long long)t);
                    CHECK(date_trunc_rt(Day, t) == ms0, "trunc day at %lld", (long long)t);
                    CHECK(date_trunc_rt(Week, t) == week_start * kMsPerDay, "trunc week at %lld = %lld, want %lld", (long long)t, (long long)date_trunc_rt(Week, t), (long long)(week_start * kMsPerDay));
                    CHECK(date_trunc_rt(Month, t) == month_start * kMsPerDay, "trunc month at %lld", (long long)t);
                    CHECK(date_trunc_rt(Year, t) == year_start * kMsPerDay, "trunc year at %lld", (long long)t);
                }
            }
        }
    }
    // hand-worked
    CHECK(date_trunc_rt(Day, -1) == -86400000LL, "date_trunc(day, -1)");
    CHECK(date_trunc_rt(Second, -1) == -1000 && date_trunc_rt(Year, -1) == -365 * kMsPerDay, "date_trunc before 1970");
    CHECK(date_part_rt(Year, -1) == 1969 && date_part_rt(Month, -1) == 12 && date_part_rt(Day, -1) == 31 && date_part_rt(Hour, -1) == 23 && date_part_rt(Second, -1) == 59,
          "date_part at -1 ms");
    CHECK(date_part_rt(Dow, 0) == 4 && date_part_rt(Doy, 0) == 1, "1970-01-01 is a Thursday, day 1");
    CHECK(date_trunc_rt(Week, 0) == -3 * kMsPerDay, "the week of 1970-01-01 began on Monday 1969-12-29");
    CHECK(date_trunc_rt(Minute, 1436918400123LL) == 1436918400000LL && date_part_rt(Doy, 1436918400123LL) == 196, "2015-07-15T00:00:00.123");
    std::printf("ok %lld\n", (long long)n);
    return 0;
}
