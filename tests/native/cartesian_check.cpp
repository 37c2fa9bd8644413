// computeCartesianPath through the C++ host mirror (pick_ik_amd/host/pick_ik_amd.hpp Solver::compute_cartesian_paths)
// against the C ABI call (pikamd_cartesian_paths) and the host interpolation (pikamd_interpolate_poses) applied to the
// mirror's own forward kinematics.  Needs a GPU; prints "cartesian C++ checks OK".
#include <cmath>
#include <cstdio>
#include <cstring>

#include "../../pick_ik_amd/host/pick_ik_amd.hpp"

using namespace pick_ik_amd;

static Chain panda_chain() {
    const double PI = M_PI;
    const double o[7][6] = {{0, 0, 0.333, 0, 0, 0},        {0, 0, 0, -PI / 2, 0, 0},
                            {0, -0.316, 0, PI / 2, 0, 0},  {0.0825, 0, 0, PI / 2, 0, 0},
                            {-0.0825, 0.384, 0, -PI / 2, 0, 0}, {0, 0, 0, PI / 2, 0, 0},
                            {0.088, 0, 0, PI / 2, 0, 0}};
    const double lo[7] = {-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973};
    const double hi[7] = {2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973};
    const double vm[7] = {2.175, 2.175, 2.175, 2.175, 2.61, 2.61, 2.61};
    Chain c;
    for (int j = 0; j < 7; ++j) {
        Joint J;
        J.origin_xyz = {o[j][0], o[j][1], o[j][2]};
        J.origin_rpy = {o[j][3], o[j][4], o[j][5]};
        J.min = lo[j];
        J.max = hi[j];
        J.max_velocity = vm[j];
        c.joints.push_back(J);
    }
    c.tip_xyz = {0, 0, 0.107};
    c.tip_rpy = {0, 0, -PI / 4};
    return c;
}

#define CHECK(cond)                                                      \
    do {                                                                 \
        if (!(cond)) {                                                   \
            std::printf("CHECK FAILED line %d: %s\n", __LINE__, #cond);  \
            return 1;                                                    \
        }                                                                \
    } while (0)

int main() {
    Solver pa(panda_chain());
    const int D = 7, P = 6, W = 9;
    const std::vector<double> home = {0.0, -M_PI / 4, 0.0, -3.0 * M_PI / 4, 0.0, M_PI / 2, M_PI / 4};
    // offsets of 0.05 .. 1.05 m from configurations 0.3 rad off the ready pose: the long ones need more than W steps
    // or leave the workspace
    std::vector<double> start, pose0;
    std::vector<Pose> targets;
    for (int p = 0; p < P; ++p) {
        std::vector<double> q = home;
        for (int j = 0; j < D; ++j) q[j] += 0.3 * std::sin(1.0 + p + 2.0 * j);
        start.insert(start.end(), q.begin(), q.end());
        const Pose f = pa.fk(q);
        for (double v : {f.x, f.y, f.z, f.qw, f.qx, f.qy, f.qz}) pose0.push_back(v);
        const double len = 0.05 + 0.2 * p;
        Pose t;
        t.x = len * std::cos(0.25 * p);
        t.y = len * std::sin(0.25 * p) * 0.8;
        t.z = len * std::sin(0.25 * p) * 0.6;
        targets.push_back(t);
    }
    CostSpec c;
    GradientIkParams gd;
    const std::vector<double> limit(D, 0.15);
    const pikamd_params p = Solver::to_params(c, nullptr, &gd, false);
    const pikamd_cartesian ca = {PIKAMD_CARTESIAN_OFFSET, 3, 0.1, 0.0, 1.3};
    std::vector<double> t7;
    for (const Pose& g : targets)
        for (double v : {g.x, g.y, g.z, g.qw, g.qx, g.qy, g.qz}) t7.push_back(v);
    for (int with_limit = 0; with_limit < 2; ++with_limit) {
        const CartesianResult r = pa.compute_cartesian_paths(start, targets, W, ca, c, gd, false, with_limit ? &limit : nullptr);
        CHECK(r.paths.solution.size() == (size_t)P * W * D && r.paths.status.size() == (size_t)P * W);
        CHECK(r.paths.reached.size() == (size_t)P && r.steps.size() == (size_t)P && r.fraction.size() == (size_t)P);
        CHECK(r.goals.size() == (size_t)P * W);
        // the C ABI call with the same arguments: the same bytes
        std::vector<double> sol((size_t)P * W * D), cost((size_t)P * W), fraction(P), goals((size_t)P * W * 7);
        std::vector<int32_t> st((size_t)P * W), reached(P), steps(P);
        std::vector<pikamd_stats> stats((size_t)P * W);
        CHECK(pikamd_cartesian_paths(pa.handle(), &p, &ca, P, W, start.data(), t7.data(), with_limit ? limit.data() : nullptr,
                                     sol.data(), st.data(), cost.data(), stats.data(), reached.data(), steps.data(),
                                     fraction.data(), goals.data()) == 0);
        CHECK(std::memcmp(sol.data(), r.paths.solution.data(), sizeof(double) * sol.size()) == 0);
        CHECK(std::memcmp(cost.data(), r.paths.cost.data(), sizeof(double) * cost.size()) == 0);
        CHECK(std::memcmp(fraction.data(), r.fraction.data(), sizeof(double) * fraction.size()) == 0);
        CHECK(st == r.paths.status && reached == r.paths.reached && steps == r.steps);
        CHECK(std::memcmp(stats.data(), r.paths.stats.data(), sizeof(pikamd_stats) * stats.size()) == 0);
        // the poses that were walked: the host interpolation of the mirror's forward kinematics, bit for bit
        std::vector<double> want((size_t)P * W * 7);
        std::vector<int32_t> want_steps(P);
        CHECK(pikamd_interpolate_poses(&ca, P, W, pose0.data(), t7.data(), want.data(), want_steps.data()) == 0);
        CHECK(want_steps == steps && std::memcmp(want.data(), goals.data(), sizeof(double) * want.size()) == 0);
        int walked = 0, too_long = 0, whole = 0;
        for (int i = 0; i < P; ++i) {
            const Pose& g = r.goals[(size_t)i * W];
            CHECK(g.x == goals[(size_t)i * W * 7] && g.qz == goals[(size_t)i * W * 7 + 6]);
            CHECK(r.steps[i] >= 3 && r.fraction[i] >= 0.0 && r.fraction[i] <= 1.0);
            too_long += r.steps[i] > W;
            walked += r.steps[i] <= W;
            whole += r.fraction[i] == 1.0;
            if (r.steps[i] > W) CHECK(r.paths.reached[i] == 0 && r.fraction[i] == 0.0);
        }
        std::printf("cartesian paths (step limit %s): %d walked, %d whole, %d too long\n", with_limit ? "0.15" : "none", walked,
                    whole, too_long);
        CHECK(walked >= 1 && too_long >= 1);
    }
    // argument checks of the mirror
    try {
        pa.compute_cartesian_paths(start, targets, 0, ca, c, gd);
        CHECK(false);
    } catch (const std::invalid_argument&) {
    }
    try {
        pa.compute_cartesian_paths(home, targets, W, ca, c, gd);
        CHECK(false);
    } catch (const std::invalid_argument&) {
    }
    std::puts("cartesian C++ checks OK");
    return 0;
}
