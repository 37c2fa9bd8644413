// pik_interp.hpp -- the waypoints of a Cartesian motion (pikamd_interpolate_poses, include/pick_ik_amd.h): the
// resolved target, MoveIt's step count and the interpolated pose of every waypoint, as computeCartesianPath has them.
//
// The arithmetic lives here once and is compiled twice: for the host into pik_amd.hip (pikamd_interpolate_poses) and
// for the device into the prepare kernel of pik_cartesian.hpp.  Both give the same bits in every flavour: every
// function body is compiled with fp contract(off), square roots and quotients are the IEEE ones, and sine, cosine and
// arctangent are the fixed forms below (sums of a few exactly stated terms, no library call) -- the pattern of the
// restart draw in pik_search.hpp.  Nothing here is read by pik_inst.hip.
//
// Accuracy (tests/test_cartesian_cpu.py, against a 50-digit restatement): DESIGN.md section 3.
#pragma once

#include <cstdint>

#if !defined(PIK_HD)
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PIK_HD __host__ __device__ __forceinline__
#else
#define PIK_HD inline
#endif
#endif

namespace pik_interp {

constexpr int FRAME_GLOBAL = 0, FRAME_TIP = 1, FRAME_OFFSET = 2; // PIKAMD_CARTESIAN_*
constexpr int STEPS_MAX = 2147483647;                            // INT32_MAX

// what pikamd_cartesian carries, for one call
struct Motion {
    int frame;
    int min_steps; // resolved: never 0
    double max_translation, max_rotation;
};

PIK_HD double abs_f64(double x) { return x < 0.0 ? -x : x; }

// sin x and cos x for 0 <= x <= pi/4 (plus a rounding): the Taylor sums through x^17 and x^18, Horner in x^2
PIK_HD double sin_small(double x) {
#pragma clang fp contract(off)
    const double z = x * x;
    double p = -1.0 / 355687428096000.0; // 1 / 17!
    p = p * z + 1.0 / 1307674368000.0;
    p = p * z - 1.0 / 6227020800.0;
    p = p * z + 1.0 / 39916800.0;
    p = p * z - 1.0 / 362880.0;
    p = p * z + 1.0 / 5040.0;
    p = p * z - 1.0 / 120.0;
    p = p * z + 1.0 / 6.0;
    const double xz = x * z;
    return x - xz * p;
}
PIK_HD double cos_small(double x) {
#pragma clang fp contract(off)
    const double z = x * x;
    double p = -1.0 / 6402373705728000.0; // 1 / 18!
    p = p * z + 1.0 / 20922789888000.0;
    p = p * z - 1.0 / 87178291200.0;
    p = p * z + 1.0 / 479001600.0;
    p = p * z - 1.0 / 3628800.0;
    p = p * z + 1.0 / 40320.0;
    p = p * z - 1.0 / 720.0;
    p = p * z + 1.0 / 24.0;
    const double zz = z * z;
    const double half = 0.5 * z;
    return (1.0 - half) + zz * p;
}
constexpr double PIO2_HI = 1.5707963267948966, PIO2_LO = 6.123233995736766e-17, PIO4 = 0.7853981633974483;

// sin x for 0 <= x <= pi/2 (plus a rounding): above pi/4 the cosine of the complement
PIK_HD double sin_quarter(double x) {
#pragma clang fp contract(off)
    if (x <= PIO4) return sin_small(x);
    const double c = (PIO2_HI - x) + PIO2_LO;
    return cos_small(c);
}

// atan t for 0 <= t <= 1: t = c + ..., c = i / 8 the nearest eighth, atan t = atan c + atan((t - c) / (1 + t c)); the
// second argument is at most 1/16 and its arctangent the Taylor sum through r^19
PIK_HD double atan_unit(double t) {
#pragma clang fp contract(off)
    if (!(t >= 0.0) || !(t <= 1.0)) return t; // (a NaN is carried through)
    const int i = (int)(8.0 * t + 0.5);
    const double c = 0.125 * (double)i;
    const double base = i == 0   ? 0.0
                        : i == 1 ? 0.12435499454676144
                        : i == 2 ? 0.24497866312686414
                        : i == 3 ? 0.35877067027057225
                        : i == 4 ? 0.4636476090008061
                        : i == 5 ? 0.5585993153435624
                        : i == 6 ? 0.6435011087932844
                        : i == 7 ? 0.7188299996216245
                                 : 0.7853981633974483;
    const double num = t - c;
    const double den = 1.0 + t * c;
    const double r = num / den;
    const double z = r * r;
    double p = 1.0 / 19.0;
    p = 1.0 / 17.0 - p * z;
    p = 1.0 / 15.0 - p * z;
    p = 1.0 / 13.0 - p * z;
    p = 1.0 / 11.0 - p * z;
    p = 1.0 / 9.0 - p * z;
    p = 1.0 / 7.0 - p * z;
    p = 1.0 / 5.0 - p * z;
    p = 1.0 / 3.0 - p * z;
    const double rz = r * z;
    const double tail = r - rz * p;
    return base + tail;
}

// atan2(y, x) for y >= 0 and x >= 0; (0, 0) and anything that is not a number: 0 + the NaN carried through
PIK_HD double atan2_quadrant(double y, double x) {
#pragma clang fp contract(off)
    if (y <= x) {
        if (!(x > 0.0)) return y + x; // (0, 0): 0; a NaN stays one
        return atan_unit(y / x);
    }
    if (!(y > x)) return y + x; // (a NaN)
    const double a = atan_unit(x / y);
    return (PIO2_HI - a) + PIO2_LO;
}

// Hamilton product a (x) b, w x y z
PIK_HD void quat_mul(const double (&a)[4], const double (&b)[4], double (&o)[4]) {
#pragma clang fp contract(off)
    o[0] = ((a[0] * b[0] - a[1] * b[1]) - a[2] * b[2]) - a[3] * b[3];
    o[1] = ((a[0] * b[1] + a[1] * b[0]) + a[2] * b[3]) - a[3] * b[2];
    o[2] = ((a[0] * b[2] - a[1] * b[3]) + a[2] * b[0]) + a[3] * b[1];
    o[3] = ((a[0] * b[3] + a[1] * b[2]) - a[2] * b[1]) + a[3] * b[0];
}

// R(q) v with Eigen's toRotationMatrix (no normalisation), rows summed left to right
PIK_HD void quat_rotate(const double (&q)[4], const double (&v)[3], double (&o)[3]) {
#pragma clang fp contract(off)
    const double tx = 2.0 * q[1], ty = 2.0 * q[2], tz = 2.0 * q[3];
    const double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0];
    const double txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
    const double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
    o[0] = ((1.0 - (tyy + tzz)) * v[0] + (txy - twz) * v[1]) + (txz + twy) * v[2];
    o[1] = ((txy + twz) * v[0] + (1.0 - (txx + tzz)) * v[1]) + (tyz - twx) * v[2];
    o[2] = ((txz - twy) * v[0] + (tyz + twx) * v[1]) + (1.0 - (txx + tyy)) * v[2];
}

// the resolved target b of a motion from pose a (7 doubles: position, quaternion w x y z)
PIK_HD void resolve_target(int frame, const double (&a)[7], const double (&t)[7], double (&b)[7]) {
#pragma clang fp contract(off)
    const double qa[4] = {a[3], a[4], a[5], a[6]};
    if (frame == FRAME_TIP) {
        const double qt[4] = {t[3], t[4], t[5], t[6]};
        const double tt[3] = {t[0], t[1], t[2]};
        double r[3], q[4];
        quat_rotate(qa, tt, r);
        quat_mul(qa, qt, q);
        b[0] = a[0] + r[0];
        b[1] = a[1] + r[1];
        b[2] = a[2] + r[2];
        b[3] = q[0];
        b[4] = q[1];
        b[5] = q[2];
        b[6] = q[3];
    } else if (frame == FRAME_OFFSET) {
        b[0] = a[0] + t[0];
        b[1] = a[1] + t[1];
        b[2] = a[2] + t[2];
        b[3] = a[3];
        b[4] = a[4];
        b[5] = a[5];
        b[6] = a[6];
    } else {
        for (int k = 0; k < 7; ++k) b[k] = t[k];
    }
}

// floor(dist / limit) as a step count; -1: the quotient is not finite or not below 2^31
PIK_HD long long steps_of(double dist, double limit) {
#pragma clang fp contract(off)
    if (!(limit > 0.0)) return 0;
    const double q = dist / limit;
    if (!(q < 2147483648.0) || !(q >= 0.0)) return -1;
    return (long long)__builtin_floor(q);
}

// MoveIt's step count of the motion a -> b (CartesianInterpolator::computeCartesianPath)
PIK_HD int step_count(const Motion& m, const double (&a)[7], const double (&b)[7]) {
#pragma clang fp contract(off)
    const double dx = b[0] - a[0], dy = b[1] - a[1], dz = b[2] - a[2];
    const double trans = __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
    const double qa[4] = {a[3], a[4], a[5], a[6]};
    const double qbc[4] = {b[3], -b[4], -b[5], -b[6]};
    double d[4];
    quat_mul(qa, qbc, d);
    const double vn = __builtin_sqrt((d[1] * d[1] + d[2] * d[2]) + d[3] * d[3]);
    const double rot = 2.0 * atan2_quadrant(vn, abs_f64(d[0]));
    const long long ts = steps_of(trans, m.max_translation), rs = steps_of(rot, m.max_rotation);
    if (ts < 0 || rs < 0) return STEPS_MAX;
    long long n = (ts > rs ? ts : rs) + 1;
    if (n < (long long)m.min_steps) n = m.min_steps;
    return n > (long long)STEPS_MAX ? STEPS_MAX : (int)n;
}

// Eigen's slerp scales of the motion a -> b: waypoint k is s0(k) qa + s1(k) qb.  What does not depend on k.
struct Slerp {
    double theta, sin_theta; // (linear: not read)
    bool linear, negate;
};
PIK_HD Slerp slerp_begin(const double (&a)[7], const double (&b)[7]) {
#pragma clang fp contract(off)
    Slerp s;
    const double d = ((a[3] * b[3] + a[4] * b[4]) + a[5] * b[5]) + a[6] * b[6];
    const double ad = abs_f64(d);
    s.negate = d < 0.0;
    s.linear = !(ad < 1.0 - 2.220446049250313e-16); // |d| >= 1 - 2^-52 (a NaN: linear, and it is carried through)
    s.theta = 0.0;
    s.sin_theta = 1.0;
    if (!s.linear) {
        // acos|d| = atan2(sqrt((1 - |d|)(1 + |d|)), |d|)
        const double y = __builtin_sqrt((1.0 - ad) * (1.0 + ad));
        s.theta = atan2_quadrant(y, ad);
        s.sin_theta = sin_quarter(s.theta);
    }
    return s;
}

// waypoint k of n (0 <= k < n) of the motion a -> b
PIK_HD void waypoint(const Slerp& s, const double (&a)[7], const double (&b)[7], int k, int n, double (&o)[7]) {
#pragma clang fp contract(off)
    const double pct = (double)((long long)k + 1) / (double)n;
    const double rest = 1.0 - pct;
    o[0] = pct * b[0] + rest * a[0];
    o[1] = pct * b[1] + rest * a[1];
    o[2] = pct * b[2] + rest * a[2];
    double s0 = rest, s1 = pct;
    if (!s.linear) {
        s0 = sin_quarter(rest * s.theta) / s.sin_theta;
        s1 = sin_quarter(pct * s.theta) / s.sin_theta;
    }
    if (s.negate) s1 = -s1;
    o[3] = s0 * a[3] + s1 * b[3];
    o[4] = s0 * a[4] + s1 * b[4];
    o[5] = s0 * a[5] + s1 * b[5];
    o[6] = s0 * a[6] + s1 * b[6];
}

// One path of pikamd_interpolate_poses: the step count and the W rows of `goals` (row stride 7).  Rows k >= n, and
// every row of a path with n > W, hold b.
PIK_HD int interpolate_path(const Motion& m, int W, const double (&a)[7], const double (&t)[7], double* goals) {
    double b[7];
    resolve_target(m.frame, a, t, b);
    const int n = step_count(m, a, b);
    const Slerp s = slerp_begin(a, b);
    for (int k = 0; k < W; ++k) {
        double o[7];
        if (n <= W && k < n) {
            waypoint(s, a, b, k, n, o);
        } else {
            for (int e = 0; e < 7; ++e) o[e] = b[e];
        }
        for (int e = 0; e < 7; ++e) goals[7 * (long long)k + e] = o[e];
    }
    return n;
}

} // namespace pik_interp
