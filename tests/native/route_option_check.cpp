// The parser of the option device_regime (pick_ik_amd/csrc/pik_route_ops.hpp): "1", "" and NULL switch the device-side
// choice of the regime on, "0" off, everything else is refused.  Host only: compiled by tests/test_device_regime_cpu.py
// as HIP host code (the header reaches hip_runtime.h), no device needed to run it.
#include <cstdio>

#include "../../pick_ik_amd/csrc/pik_route_ops.hpp"

int main() {
    int bad = 0;
    auto expect = [&](const char* text, bool ok, int value) {
        int got = -7;
        const bool r = pik::parse_device_regime(text, &got);
        if (r != ok || (ok && got != value) || (!ok && got != -7)) {
            std::printf("parse_device_regime(%s): accepted %d value %d, expected accepted %d value %d\n",
                        text ? text : "NULL", (int)r, got, (int)ok, value);
            ++bad;
        }
    };
    expect("1", true, 1);
    expect("0", true, 0);
    expect("", true, 1);
    expect(nullptr, true, 1);
    for (const char* t : {"2", "-1", "01", "10", "1 ", " 1", "on", "off", "true", "adaptive", "0x0", "1,0"}) expect(t, false, 0);
    // the routed launcher's state lies behind the counter blocks and does not overlap them
    static_assert(pik::ROUTE_OFF_VC == pik::COUNTER_BLOCK * pik::N_SLOTS, "behind the N_SLOTS blocks");
    static_assert(pik::ROUTE_OFF_LOADS == pik::ROUTE_OFF_VC + pik::ROUTE_VC_BLOCK * pik::N_SLOTS, "loads behind the counters");
    static_assert(pik::COUNTERS_BYTES == pik::ROUTE_OFF_RECORD + pik::ROUTE_RECORD_BLOCK * pik::N_SLOTS, "records last");
    if (bad) return 1;
    std::printf("route option check OK\n");
    return 0;
}
