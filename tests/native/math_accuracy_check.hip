// Dense accuracy of the kernels' own transcendentals (pick_ik_amd/csrc/pik_math.hpp): sincos_f64 (with and without
// the 2 pi fold), fold_2pi, sincos_delta, atan2_pos, angle_of and matrix_to_quat, over the ranges and edges where such
// code goes wrong, against x87 long double references (64-bit significand).  Built once per flavour with that
// flavour's flags (tests/test_gpu_math_accuracy.py): no define = product / fast (the inline-assembly Horner steps on
// the device), -DPIK_STRICT -DPIK_EXACT_FMA = exact-fma (the coefficients from constant memory), -DPIK_STRICT = strict.
//
// Compiled by hipcc, every input is evaluated on the device AND on the host from the same source; the device results
// must be bit-identical to the host's (a NaN only has to be a NaN).  Compiled by a plain C++ compiler (no __HIPCC__)
// it is the host half alone (tests/test_host_math_cpu.py), without the device comparison.
//
// usage: math_accuracy_check [n_per_range]        one JSON line per (function, range): n, device_mismatch (-1: no
// device pass), max_ulp / max_abs against the reference, and the worst inputs with their results.
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#endif

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../pick_ik_amd/csrc/pik_host.hpp"

using namespace pik;

enum Op { SINCOS_FOLD, SINCOS_NOFOLD, FOLD, DELTA, ATAN2, ANGLE, M2Q };
static const int NIN = 9, NOUT = 4;

PIK_HD void eval(int op, MT m, const double* a, double* r) {
    switch (op) {
        case SINCOS_FOLD: sincos_f64<true>(m, a[0], r[0], r[1]); break;
        case SINCOS_NOFOLD: sincos_f64<false>(m, a[0], r[0], r[1]); break;
        case FOLD: r[0] = fold_2pi(m, a[0]); break;
        case DELTA: sincos_delta(a[0], a[1], a[2], r[0], r[1]); break;
        case ATAN2: r[0] = atan2_pos(m, a[0], a[1]); break;
        case ANGLE: {
            const double d[4] = {a[0], a[1], a[2], a[3]};
            double vn;
            r[0] = angle_of(m, d, vn);
            break;
        }
        default: {
            const double R[9] = {a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8]};
            double q[4];
            matrix_to_quat(R, q);
            for (int k = 0; k < 4; ++k) r[k] = q[k];
        }
    }
}

#if defined(__HIPCC__)
__global__ void run(int op, int nin, const MathTab* tab, const double* in, double* out, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    // the kernels read the table through the constant address space (scalar loads), as the library does
    const PIK_CONSTANT MathTab* m = (const PIK_CONSTANT MathTab*)(tab);
    double r[NOUT] = {0.0, 0.0, 0.0, 0.0};
    eval(op, *m, in + nin * i, r);
    for (int k = 0; k < NOUT; ++k) out[NOUT * i + k] = r[k];
}
#endif

#if !defined(__HIP_DEVICE_COMPILE__) // (the rest is the host program: the device pass sees the table in address space 4)
typedef long double LD;

struct Rng {
    uint64_t s;
    double u() { // [0, 1)
        s += 0x9E3779B97F4A7C15ull;
        uint64_t z = s;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        return (double)(z >> 11) * (1.0 / 9007199254740992.0);
    }
    double logu(double lo, double hi) { return std::exp(std::log(lo) + (std::log(hi) - std::log(lo)) * u()); }
    double sign() { return u() < 0.5 ? -1.0 : 1.0; }
    long long i(long long lo, long long hi) { return lo + (long long)(u() * (double)(hi - lo + 1)); }
};

// x moved by j ulps away from zero (j < 0: towards it); x != 0, and the result keeps the sign of x
static double step_ulps(double x, long long j) {
    int64_t b;
    std::memcpy(&b, &x, 8);
    b += j;
    std::memcpy(&x, &b, 8);
    return x;
}

// the double ulp at the magnitude of a (long double) reference value
static LD ulp_of(LD r) {
    r = fabsl(r);
    if (r < 2.2250738585072014e-308L) return 4.9406564584124654e-324L;
    int e;
    frexpl(r, &e);
    return ldexpl(1.0L, e - 53);
}

static const LD PI_L = 3.14159265358979323846264338327950288L;
// 2 pi = C1 + C2 + C3 + C4: C1..C3 with at most 16 significant bits, so that k Ci is exact in long double for
// |k| < 2^48 (|x| < 1.7e15); C4 = the rest to 64 bits
static const LD TWO_PI_C1 = 0x1.921ep+2L, TWO_PI_C2 = 0x1.b544p-14L, TWO_PI_C3 = 0x1.0b4p-32L,
                TWO_PI_C4 = 2.156121143263247621157894121379875021164e-14L;

struct Range {
    std::string fn, name;
    int op, nout, nin;
    std::vector<double> in;  // nin per point
    std::vector<LD> ref;     // NOUT per point
    bool absolute_only = false;
};

static void add(Range& r, const double* a, const LD* ref) {
    for (int k = 0; k < r.nin; ++k) r.in.push_back(a[k]);
    for (int k = 0; k < r.nout; ++k) r.ref.push_back(ref[k]);
}

static void sincos_point(Range& r, double x) {
    const LD ref[2] = {sinl((LD)x), cosl((LD)x)};
    add(r, &x, ref);
}

static const int N_GROUPS = 8;
// the ranges of one group (generated group by group: a range of 10^7 points holds ~0.5 GB)
static std::vector<Range> make_ranges(int group, long long n, const MathTab& mt) {
    std::vector<Range> out;
    for (int fold = 1; fold >= 0; --fold) {
        if (group != 1 - fold) continue;
        const int op = fold ? SINCOS_FOLD : SINCOS_NOFOLD;
        const std::string fn = fold ? "sincos_f64<true>" : "sincos_f64<false>";
        Rng g{0x5151ull + (uint64_t)fold};
        Range a{fn, "pi", op, 2, 1}, b{fn, "65536", op, 2, 1}, c{fn, "tiny", op, 2, 1}, d{fn, "near_k_pi_2", op, 2, 1},
            e{fn, "fold_switch_below", op, 2, 1}, e2{fn, "fold_switch_above", op, 2, 1};
        e2.absolute_only = true;
        for (long long i = 0; i < n; ++i) {
            sincos_point(a, PI_L * (2.0 * g.u() - 1.0));
            sincos_point(b, 65536.0 * (2.0 * g.u() - 1.0));
            sincos_point(c, g.sign() * g.logu(1e-300, 1e-1));
            const double k = g.sign() * (double)g.i(1, 41720);
            sincos_point(d, step_ulps((double)((LD)k * (PI_L / 2)), g.i(-4, 4)));
            // 65536 and its neighbours (2^22 ulps = 6e-5 rad on either side), both signs: |x| <= 65536 is reduced
            // directly, above it is folded first (the fold-free form serves |x| <= 65536 + pi without folding)
            const long long j = g.i(-(1ll << 22), 1ll << 22);
            sincos_point(j <= 0 ? e : e2, g.sign() * step_ulps(65536.0, j));
        }
        out.push_back(a); out.push_back(b); out.push_back(c); out.push_back(d); out.push_back(e); out.push_back(e2);
        if (fold) {
            Range f{fn, "beyond_fold", op, 2, 1};
            f.absolute_only = true;
            for (long long i = 0; i < n; ++i) sincos_point(f, g.sign() * g.logu(65536.0, 1e15));
            out.push_back(f);
        }
    }
    if (group == 2) { // fold_2pi: x - 2 pi rint(x / 2 pi), the reference with the kernel's own k and an exact product k (2 pi)
        Rng g{0xF01Dull};
        Range f{"fold_2pi", "beyond_fold", FOLD, 1, 1};
        f.absolute_only = true;
        for (long long i = 0; i < n; ++i) {
            const double x = g.sign() * g.logu(65536.0, 1e15);
            const double k = std::rint(x * mt.v[0]);
            // the first three differences are exact (their results fit 64 bits); the last rounds once: ~4e-19
            const LD ref = ((((LD)x - (LD)k * TWO_PI_C1) - (LD)k * TWO_PI_C2) - (LD)k * TWO_PI_C3) - (LD)k * TWO_PI_C4;
            add(f, &x, &ref);
        }
        out.push_back(f);
    }
    if (group == 3) { // sincos_delta from sincos_f64's values: theta in [-pi, pi], |d| <= 1e-3 (the line-search step bound)
        Rng g{0xDE17Aull};
        Range r{"sincos_delta", "step_1e-3", DELTA, 2, 3};
        r.absolute_only = true;
        for (long long i = 0; i < n; ++i) {
            const double th = (double)(PI_L * (2.0 * g.u() - 1.0));
            const double d = (i & 1) ? 1e-3 * (2.0 * g.u() - 1.0) : g.sign() * g.logu(1e-12, 1e-3);
            double a[3];
            sincos_f64<true>(mt, th, a[0], a[1]);
            a[2] = d;
            const LD ref[2] = {sinl(th) * cosl(d) + cosl(th) * sinl(d), cosl(th) * cosl(d) - sinl(th) * sinl(d)};
            add(r, a, ref);
        }
        out.push_back(r);
    }
    if (group == 4) { // atan2 (y, x >= 0)
        Rng g{0xA7A2ull};
        Range a{"atan2_pos", "loguniform_1e-300_1e3", ATAN2, 1, 2}, b{"atan2_pos", "loguniform_1e-8_1e2", ATAN2, 1, 2},
            s{"atan2_pos", "switch_points", ATAN2, 1, 2}, z{"atan2_pos", "zero", ATAN2, 1, 2};
        const double sw[6] = {1.0, 0.41421356237309503, 7.0 / 16, 11.0 / 16, 19.0 / 16, 39.0 / 16};
        for (long long i = 0; i < n; ++i) {
            double p[2] = {g.logu(1e-300, 1e3), g.logu(1e-300, 1e3)};
            LD ref = atan2l(p[0], p[1]);
            add(a, p, &ref);
            p[0] = g.logu(1e-8, 1e2);
            p[1] = g.logu(1e-8, 1e2);
            ref = atan2l(p[0], p[1]);
            add(b, p, &ref);
            const double x = g.logu(1e-3, 1e3);
            p[1] = x;
            p[0] = step_ulps(x * sw[g.i(0, 5)], g.i(-8, 8));
            if (i & 1) std::swap(p[0], p[1]);
            ref = atan2l(p[0], p[1]);
            add(s, p, &ref);
            const double v = g.logu(1e-300, 1e3);
            p[0] = (i & 1) ? 0.0 : v;
            p[1] = (i & 1) ? v : 0.0;
            ref = atan2l(p[0], p[1]);
            add(z, p, &ref);
        }
        out.push_back(a); out.push_back(b); out.push_back(s); out.push_back(z);
    }
    if (group == 5) { // angle_of: relative quaternions of angle theta in [1e-9, pi], w of either sign
        Rng g{0xA261Eull};
        Range r{"angle_of", "1e-9_pi", ANGLE, 1, 4};
        for (long long i = 0; i < n; ++i) {
            const LD th = g.logu(1e-9, (double)PI_L);
            LD ax[3] = {g.u() - 0.5, g.u() - 0.5, g.u() - 0.5};
            const LD an = sqrtl(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
            const LD sh = sinl(th / 2) / an;
            const double d[4] = {(double)(g.sign() * cosl(th / 2)), (double)(ax[0] * sh), (double)(ax[1] * sh),
                                 (double)(ax[2] * sh)};
            const LD v0 = d[1], v1 = d[2], v2 = d[3];
            const LD ref = 2 * atan2l(sqrtl(v0 * v0 + v1 * v1 + v2 * v2), fabsl((LD)d[0]));
            add(r, d, &ref);
        }
        out.push_back(r);
    }
    if (group >= 6) { // matrix_to_quat: rotations near angle pi, near trace 0 (the W / non-W switch), near ties of the diagonal
        Rng g{0x3A7Bull};
        const char* names[4] = {"near_pi", "near_trace_0", "diagonal_ties", "random"};
        for (int kind = 2 * (group - 6); kind < 2 * (group - 6) + 2; ++kind) {
            Range r{"matrix_to_quat", names[kind], M2Q, 4, 9};
            r.absolute_only = true;
            for (long long i = 0; i < n; ++i) {
                LD th, ax[3];
                if (kind == 2) { // two (or three) equal axis components: equal diagonal elements
                    const LD a = g.u() * 2 - 1, t = (i % 3 == 0) ? 0.0L : (LD)g.sign() * g.logu(1e-15, 1e-3);
                    ax[0] = a;
                    ax[1] = (g.u() < 0.5 ? a : -a) * (1 + t);
                    ax[2] = (i % 5 == 0) ? a : (LD)(g.u() * 2 - 1);
                } else {
                    for (LD& v : ax) v = g.u() * 2 - 1;
                }
                if (kind == 0) th = PI_L - ((i % 7 == 0) ? 0.0L : (LD)g.logu(1e-12, 1e-1));
                else if (kind == 1) th = 2 * PI_L / 3 + g.sign() * g.logu(1e-16, 1e-3);
                else th = PI_L * g.u();
                const LD an = sqrtl(ax[0] * ax[0] + ax[1] * ax[1] + ax[2] * ax[2]);
                const LD w = cosl(th / 2), s = sinl(th / 2) / an;
                const LD x = ax[0] * s, y = ax[1] * s, z = ax[2] * s;
                const double R[9] = {(double)(1 - 2 * (y * y + z * z)), (double)(2 * (x * y - w * z)), (double)(2 * (x * z + w * y)),
                                     (double)(2 * (x * y + w * z)), (double)(1 - 2 * (x * x + z * z)), (double)(2 * (y * z - w * x)),
                                     (double)(2 * (x * z - w * y)), (double)(2 * (y * z + w * x)), (double)(1 - 2 * (x * x + y * y))};
                const LD ref[4] = {w, x, y, z};
                add(r, R, ref);
            }
            out.push_back(r);
        }
    }
    return out;
}

static bool same_bits(double a, double b) {
    if (std::isnan(a) && std::isnan(b)) return true;
    uint64_t x, y;
    std::memcpy(&x, &a, 8);
    std::memcpy(&y, &b, 8);
    return x == y;
}

static void print_vec(const char* key, const double* v, int n) {
    std::printf(", \"%s\": [", key);
    for (int k = 0; k < n; ++k) std::printf("%s\"%a\"", k ? ", " : "", v[k]);
    std::printf("]");
}

int main(int argc, char** argv) {
    const long long n = argc > 1 ? std::atoll(argv[1]) : 1000000;
    if (n < 8) return 2;
    MathTab mt;
    fill_math_tab(mt);
#if defined(__HIPCC__)
    MathTab* dtab = nullptr;
    double *din = nullptr, *dout = nullptr;
    if (hipMalloc(&dtab, sizeof mt) != hipSuccess || hipMalloc(&din, 8 * NIN * n) != hipSuccess ||
        hipMalloc(&dout, 8 * NOUT * n) != hipSuccess)
        return 2;
    if (hipMemcpy(dtab, &mt, sizeof mt, hipMemcpyHostToDevice) != hipSuccess) return 2;
#endif
    std::vector<double> host((size_t)NOUT * n), dev((size_t)NOUT * n);
    for (int group = 0; group < N_GROUPS; ++group)
    for (const Range& r : make_ranges(group, n, mt)) {
        const int nin = r.nin, nout = r.nout;
        const long long m = (long long)r.in.size() / nin;
        for (long long i = 0; i < m; ++i) {
            double* o = &host[(size_t)(NOUT * i)];
            o[0] = o[1] = o[2] = o[3] = 0.0;
            eval(r.op, mt, &r.in[(size_t)(nin * i)], o);
        }
        long long mismatch = -1;
#if defined(__HIPCC__)
        if (m > n || hipMemcpy(din, r.in.data(), 8 * nin * m, hipMemcpyHostToDevice) != hipSuccess) return 3;
        hipLaunchKernelGGL(run, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, r.op, nin, dtab, din, dout, m);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 4;
        if (hipMemcpy(dev.data(), dout, 8 * NOUT * m, hipMemcpyDeviceToHost) != hipSuccess) return 3;
        mismatch = 0;
        for (long long i = 0; i < m; ++i) {
            bool same = true;
            for (int k = 0; k < r.nout; ++k) same = same && same_bits(dev[(size_t)(NOUT * i + k)], host[(size_t)(NOUT * i + k)]);
            mismatch += !same;
        }
#endif
        LD max_ulp = 0, max_abs = 0;
        long long wu = 0, wa = 0, nonfinite = 0;
        for (long long i = 0; i < m; ++i) {
            const double* o = &host[(size_t)(NOUT * i)];
            const LD* ref = &r.ref[(size_t)(nout * i)];
            LD e_abs = 0, e_ulp = 0;
            if (r.op == M2Q) { // up to the sign of the quaternion
                LD ep = 0, em = 0;
                for (int k = 0; k < 4; ++k) {
                    ep = fmaxl(ep, fabsl((LD)o[k] - ref[k]));
                    em = fmaxl(em, fabsl((LD)o[k] + ref[k]));
                }
                e_abs = fminl(ep, em);
                e_ulp = e_abs / ulp_of(1.0L);
            } else {
                for (int k = 0; k < r.nout; ++k) {
                    if (!std::isfinite(o[k])) { ++nonfinite; continue; }
                    const LD d = fabsl((LD)o[k] - ref[k]);
                    e_abs = fmaxl(e_abs, d);
                    e_ulp = fmaxl(e_ulp, d / ulp_of(ref[k]));
                }
            }
            if (e_ulp > max_ulp) { max_ulp = e_ulp; wu = i; }
            if (e_abs > max_abs) { max_abs = e_abs; wa = i; }
        }
        std::printf("{\"fn\": \"%s\", \"range\": \"%s\", \"n\": %lld, \"device_mismatch\": %lld, \"nonfinite\": %lld, "
                    "\"max_ulp\": %.6Lg, \"max_abs\": %.6Lg", r.fn.c_str(), r.name.c_str(), m, mismatch, nonfinite, max_ulp, max_abs);
        print_vec("worst_ulp_in", &r.in[(size_t)(nin * wu)], nin);
        print_vec("worst_ulp_out", &host[(size_t)(NOUT * wu)], r.nout);
        print_vec("worst_abs_in", &r.in[(size_t)(nin * wa)], nin);
        print_vec("worst_abs_out", &host[(size_t)(NOUT * wa)], r.nout);
        std::printf("}\n");
        std::fflush(stdout);
    }
    { // special values: +-0 keep their sign / cos 1, +-inf and NaN give NaN (and return)
        const double sp[5] = {0.0, -0.0, INFINITY, -INFINITY, NAN};
        for (int op = SINCOS_FOLD; op <= SINCOS_NOFOLD; ++op) {
            double hv[5][2];
            for (int i = 0; i < 5; ++i) {
                double a[NIN] = {sp[i]}, o[NOUT] = {0, 0, 0, 0};
                eval(op, mt, a, o);
                hv[i][0] = o[0];
                hv[i][1] = o[1];
            }
            long long mismatch = -1;
#if defined(__HIPCC__)
            if (hipMemcpy(din, sp, sizeof sp, hipMemcpyHostToDevice) != hipSuccess) return 3;
            hipLaunchKernelGGL(run, dim3(1), dim3(64), 0, 0, op, 1, dtab, din, dout, 5LL);
            if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) return 4;
            double dv[5 * NOUT];
            if (hipMemcpy(dv, dout, sizeof dv, hipMemcpyDeviceToHost) != hipSuccess) return 3;
            mismatch = 0;
            for (int i = 0; i < 5; ++i) mismatch += !(same_bits(dv[NOUT * i], hv[i][0]) && same_bits(dv[NOUT * i + 1], hv[i][1]));
#endif
            std::printf("{\"fn\": \"%s\", \"range\": \"special\", \"n\": 5, \"device_mismatch\": %lld, \"values\": [",
                        op == SINCOS_FOLD ? "sincos_f64<true>" : "sincos_f64<false>", mismatch);
            for (int i = 0; i < 5; ++i) std::printf("%s[\"%a\", \"%a\", \"%a\"]", i ? ", " : "", sp[i], hv[i][0], hv[i][1]);
            std::printf("]}\n");
        }
    }
#if defined(__HIPCC__)
    (void)hipFree(dtab);
    (void)hipFree(din);
    (void)hipFree(dout);
#endif
    return 0;
}
#endif // !__HIP_DEVICE_COMPILE__
