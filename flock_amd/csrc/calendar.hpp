// Calendar arithmetic of the time functions (valprog.hpp A-F4..A-F6): milliseconds since 1970-01-01T00:00:00Z <-> civil date in the proleptic
// Gregorian calendar, UTC.  Compiles on the host and on the device (every division is by a compile-time constant: a multiply-high, no division
// loop); tests/cpp/calendar_test.cpp checks it against a from-scratch day count.  The days <-> civil conversions are the era / day-of-era /
// year-of-era scheme (400-year eras of 146097 days that begin on 1 March, so the leap day is an era's last day).  Only the split of a day count into
// (era, day of era) and of a millisecond count into (day, millisecond of day) is 64-bit arithmetic; everything inside an era or a day fits 32 bits and is
// computed there (a 64-bit division by a constant is a four-multiply multiply-high on the device, a 32-bit one a single multiply).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FG_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define FG_HD inline
#endif

namespace flockgpu {
namespace cal {

constexpr int64_t kMsPerSecond = 1000, kMsPerMinute = 60000, kMsPerHour = 3600000, kMsPerDay = 86400000;

enum Unit : uint8_t { Second = 0, Minute, Hour, Day, Week, Month, Year, Dow, Doy, kUnits };

// floor(a / d) for a constant d > 0 (C++ `/` truncates towards zero)
template <int64_t D> FG_HD int64_t floor_div(int64_t a) {
    const int64_t q = a / D;
    return q - ((a % D) < 0 ? 1 : 0);
}

struct Civil {
    int64_t year;
    int32_t month, day;   // 1..12, 1..31
};

// days since 1970-01-01 of year-month-day
FG_HD int64_t days_from_civil(int64_t y, int32_t m, int32_t d) {
    y -= m <= 2 ? 1 : 0;
    const int64_t era = floor_div<400>(y);
    const uint32_t yoe = (uint32_t)(y - era * 400);                                        // [0, 399]
    const uint32_t doy = (153u * (uint32_t)(m > 2 ? m - 3 : m + 9) + 2u) / 5u + (uint32_t)d - 1u;   // [0, 365], the year beginning on 1 March
    const uint32_t doe = yoe * 365u + yoe / 4u - yoe / 100u + doy;                         // [0, 146096]
    return era * 146097 + (int64_t)doe - 719468;
}

FG_HD Civil civil_from_days(int64_t z) {
    z += 719468;
    const int64_t era = floor_div<146097>(z);
    const uint32_t doe = (uint32_t)(z - era * 146097);                                   // [0, 146096]
    const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;      // [0, 399]
    const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);                     // [0, 365]
    const uint32_t mp = (5u * doy + 2u) / 153u;                                          // [0, 11], March = 0
    Civil c;
    c.day = (int32_t)(doy - (153u * mp + 2u) / 5u + 1u);
    c.month = (int32_t)(mp < 10u ? mp + 3u : mp - 9u);
    c.year = (int64_t)yoe + era * 400 + (c.month <= 2 ? 1 : 0);
    return c;
}

// date_trunc(unit, ms): the start of the second / minute / hour / day / ISO week (Monday) / month / year that holds `ms`; towards minus
// infinity before 1970
template <int U> FG_HD int64_t date_trunc(int64_t ms) {
    if (U == Second) return floor_div<kMsPerSecond>(ms) * kMsPerSecond;
    if (U == Minute) return floor_div<kMsPerMinute>(ms) * kMsPerMinute;
    if (U == Hour) return floor_div<kMsPerHour>(ms) * kMsPerHour;
    const int64_t days = floor_div<kMsPerDay>(ms);
    if (U == Day) return days * kMsPerDay;
    if (U == Week) {   // 1970-01-01 was a Thursday: Monday = 0 puts it at 3
        const int64_t dow = (days + 3) - floor_div<7>(days + 3) * 7;
        return (days - dow) * kMsPerDay;
    }
    const Civil c = civil_from_days(days);
    return days_from_civil(c.year, U == Month ? c.month : 1, 1) * kMsPerDay;
}

// date_part(unit, ms): year, month 1..12, day 1..31, hour 0..23, minute, whole seconds 0..59, dow (Sunday = 0), doy (1 January = 1)
template <int U> FG_HD int32_t date_part(int64_t ms) {
    const int64_t days = floor_div<kMsPerDay>(ms);
    const uint32_t in_day = (uint32_t)(ms - days * kMsPerDay);   // [0, 86399999]
    if (U == Hour) return (int32_t)(in_day / (uint32_t)kMsPerHour);
    if (U == Minute) return (int32_t)((in_day / (uint32_t)kMsPerMinute) % 60u);
    if (U == Second) return (int32_t)((in_day / (uint32_t)kMsPerSecond) % 60u);
    if (U == Dow) return (int32_t)((days + 4) - floor_div<7>(days + 4) * 7);
    const Civil c = civil_from_days(days);
    if (U == Year) return (int32_t)c.year;
    if (U == Month) return c.month;
    if (U == Day) return c.day;
    return (int32_t)(days - days_from_civil(c.year, 1, 1) + 1);   // Doy
}

// the same by a run-time unit (host: tests, constant folding)
FG_HD int64_t date_trunc_rt(int unit, int64_t ms) {
    switch (unit) {
        case Second: return date_trunc<Second>(ms);
        case Minute: return date_trunc<Minute>(ms);
        case Hour: return date_trunc<Hour>(ms);
        case Day: return date_trunc<Day>(ms);
        case Week: return date_trunc<Week>(ms);
        case Month: return date_trunc<Month>(ms);
        default: return date_trunc<Year>(ms);
    }
}
FG_HD int32_t date_part_rt(int unit, int64_t ms) {
    switch (unit) {
        case Year: return date_part<Year>(ms);
        case Month: return date_part<Month>(ms);
        case Day: return date_part<Day>(ms);
        case Hour: return date_part<Hour>(ms);
        case Minute: return date_part<Minute>(ms);
        case Second: return date_part<Second>(ms);
        case Dow: return date_part<Dow>(ms);
        default: return date_part<Doy>(ms);
    }
}

}  // namespace cal
}  // namespace flockgpu
