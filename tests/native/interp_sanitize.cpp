// The host side of the interpolation header (pick_ik_amd/csrc/pik_interp.hpp) under the sanitizers: a stand-alone
// program, built by tests/test_cartesian_cpu.py with -fsanitize=address,undefined and run directly.  It interpolates
// generated motions of every frame mode -- ordinary ones, rotations of 0 and next to pi, negated quaternions, steps
// far too small (the count saturates), infinities and NaNs -- into buffers of exactly P * W * 7 doubles, with guard
// values behind them, and checks what must hold whatever the inputs: the count is at least the minimum, rows behind
// the steps repeat the target, the last waypoint of a path is its target.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <vector>

#include "../../pick_ik_amd/csrc/pik_interp.hpp"

namespace {

uint64_t state = 0x9e3779b97f4a7c15ull;
double uniform() { // xorshift64*: [0, 1)
    state ^= state >> 12;
    state ^= state << 25;
    state ^= state >> 27;
    return (double)((state * 0x2545f4914f6cdd1dull) >> 11) * (1.0 / 9007199254740992.0);
}

void unit_quat(double* q) {
    double n = 0.0;
    for (int i = 0; i < 4; ++i) {
        q[i] = 2.0 * uniform() - 1.0;
        n += q[i] * q[i];
    }
    n = std::sqrt(n > 0.0 ? n : 1.0);
    for (int i = 0; i < 4; ++i) q[i] /= n;
}

int failures = 0;
void expect(bool ok, const char* what, int i) {
    if (!ok && failures++ < 10) std::printf("case %d: %s\n", i, what);
}

} // namespace

int main() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const int cases = 20000;
    for (int i = 0; i < cases; ++i) {
        const int W = 1 + (int)(uniform() * 12.0);
        const int frame = i % 3;
        double a[7], t[7];
        for (int e = 0; e < 3; ++e) {
            a[e] = 2.0 * uniform() - 1.0;
            t[e] = (frame == 0 ? a[e] : 0.0) + 0.6 * (uniform() - 0.5);
        }
        unit_quat(a + 3);
        unit_quat(t + 3);
        pik_interp::Motion m = {frame, 1 + (int)(uniform() * 4.0), 0.02 + 0.2 * uniform(), 0.05 + uniform()};
        switch (i % 11) {
        case 1: for (int e = 3; e < 7; ++e) t[e] = frame == 1 ? (e == 3 ? 1.0 : 0.0) : a[e]; break; // no rotation
        case 2: for (int e = 3; e < 7; ++e) t[e] = -t[e]; break;
        case 3: m.max_translation = 1e-300; break;                                                  // the count saturates
        case 4: m.max_rotation = 0.0; break;
        case 5: t[0] = inf; break;
        case 6: t[4] = nan; break;
        case 7: a[1] = nan; break;
        case 8: m.max_translation = -1.0; break;
        case 9: for (int e = 0; e < 7; ++e) t[e] = frame == 0 ? a[e] : (e == 3 ? 1.0 : 0.0); break; // start = target
        default: break;
        }
        const double guard = -12345.0;
        std::vector<double> goals((size_t)W * 7 + 1, guard);
        double aa[7], tt[7];
        for (int e = 0; e < 7; ++e) {
            aa[e] = a[e];
            tt[e] = t[e];
        }
        const int n = pik_interp::interpolate_path(m, W, aa, tt, goals.data());
        expect(goals[(size_t)W * 7] == guard, "wrote behind its rows", i);
        expect(n >= m.min_steps, "fewer steps than the minimum", i);
        double b[7];
        pik_interp::resolve_target(frame, aa, tt, b);
        bool finite = true;
        for (int e = 0; e < 7; ++e) finite = finite && std::isfinite(b[e]) && std::isfinite(a[e]);
        if (!finite) continue;
        for (int k = 0; k < W; ++k) {
            const bool target_row = n > W || k >= n - 1; // (the last waypoint has pct = 1)
            if (!target_row) continue;
            for (int e = 0; e < 3; ++e) expect(goals[7 * k + e] == b[e], "a row behind the steps is not the target", i);
        }
    }
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("interp sanitize OK (%d cases)\n", cases);
    return 0;
}
