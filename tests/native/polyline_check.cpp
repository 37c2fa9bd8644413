// computeCartesianPath through waypoints by the C++ host mirror (pick_ik_amd/host/pick_ik_amd.hpp
// Solver::compute_cartesian_waypoints) against the C ABI call (pikamd_cartesian_waypoints) with the ragged lists
// written out as n_targets.  Needs a GPU; prints "polyline C++ checks OK".
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
    const int D = 7, P = 6, S = 3, W = 10;
    const std::vector<double> home = {0.0, -M_PI / 4, 0.0, -3.0 * M_PI / 4, 0.0, M_PI / 2, M_PI / 4};
    // lists of 1 .. 3 offsets of 0.05 .. 0.4 m from configurations 0.3 rad off the ready pose: the long ones do not
    // fit into W rows or leave the workspace
    std::vector<double> start;
    std::vector<std::vector<Pose>> targets;
    std::vector<double> t7((size_t)7 * P * S, 0.0);
    std::vector<int32_t> count;
    for (int p = 0; p < P; ++p) {
        std::vector<double> q = home;
        for (int j = 0; j < D; ++j) q[j] += 0.3 * std::sin(1.0 + p + 2.0 * j);
        start.insert(start.end(), q.begin(), q.end());
        std::vector<Pose> list;
        for (int i = 0; i < 1 + p % S; ++i) {
            const double len = 0.05 + 0.07 * p;
            Pose t;
            t.x = len * std::cos(0.25 * p + 1.5 * i);
            t.y = len * std::sin(0.25 * p + 1.5 * i) * 0.8;
            t.z = len * std::sin(0.25 * p + 1.5 * i) * 0.6;
            const double v[7] = {t.x, t.y, t.z, t.qw, t.qx, t.qy, t.qz};
            for (int k = 0; k < 7; ++k) t7[7 * ((size_t)p * S + i) + k] = v[k];
            list.push_back(t);
        }
        count.push_back((int32_t)list.size());
        targets.push_back(list);
    }
    CostSpec c;
    GradientIkParams gd;
    const std::vector<double> limit(D, 0.15);
    const pikamd_params p = Solver::to_params(c, nullptr, &gd, false);
    const pikamd_cartesian ca = {PIKAMD_CARTESIAN_OFFSET, 2, 0.1, 0.0, 1.3};
    for (int with_limit = 0; with_limit < 2; ++with_limit) {
        const CartesianWaypointsResult r = pa.compute_cartesian_waypoints(start, targets, W, ca, c, gd, false, with_limit ? &limit : nullptr);
        const CartesianResult& rc = r.cartesian;
        CHECK(r.max_targets == S && r.segment_steps.size() == (size_t)P * S);
        CHECK(rc.paths.solution.size() == (size_t)P * W * D && rc.paths.status.size() == (size_t)P * W);
        CHECK(rc.paths.reached.size() == (size_t)P && rc.steps.size() == (size_t)P && rc.fraction.size() == (size_t)P);
        CHECK(rc.goals.size() == (size_t)P * W);
        // the C ABI call with the same arguments: the same bytes
        std::vector<double> sol((size_t)P * W * D), cost((size_t)P * W), fraction(P), goals((size_t)P * W * 7);
        std::vector<int32_t> st((size_t)P * W), reached(P), steps(P), segs((size_t)P * S);
        std::vector<pikamd_stats> stats((size_t)P * W);
        CHECK(pikamd_cartesian_waypoints(pa.handle(), &p, &ca, P, S, W, start.data(), t7.data(), count.data(),
                                         with_limit ? limit.data() : nullptr, sol.data(), st.data(), cost.data(), stats.data(),
                                         reached.data(), steps.data(), segs.data(), fraction.data(), goals.data()) == 0);
        CHECK(std::memcmp(sol.data(), rc.paths.solution.data(), sizeof(double) * sol.size()) == 0);
        CHECK(std::memcmp(cost.data(), rc.paths.cost.data(), sizeof(double) * cost.size()) == 0);
        CHECK(std::memcmp(fraction.data(), rc.fraction.data(), sizeof(double) * fraction.size()) == 0);
        CHECK(st == rc.paths.status && reached == rc.paths.reached && steps == rc.steps && segs == r.segment_steps);
        CHECK(std::memcmp(stats.data(), rc.paths.stats.data(), sizeof(pikamd_stats) * stats.size()) == 0);
        int fitted = 0, whole = 0;
        for (int i = 0; i < P; ++i) {
            const Pose& g = rc.goals[(size_t)i * W];
            CHECK(g.x == goals[(size_t)i * W * 7] && g.qz == goals[(size_t)i * W * 7 + 6]);
            CHECK(rc.fraction[i] >= 0.0 && rc.fraction[i] <= 1.0);
            int sum = 0;
            for (int k = 0; k < S; ++k) {
                sum += segs[(size_t)i * S + k];
                if (k >= count[i]) CHECK(segs[(size_t)i * S + k] == 0); // (no segment behind the list's end)
            }
            CHECK(segs[(size_t)i * S] >= 2 && sum == rc.steps[i]); // (steps: the rows of every segment started)
            fitted += rc.steps[i] <= W;
            whole += rc.fraction[i] == 1.0;
        }
        std::printf("cartesian waypoints (step limit %s): %d fitted, %d whole\n", with_limit ? "0.15" : "none", fitted, whole);
        CHECK(fitted >= 1 && whole >= 1);
    }
    // argument checks of the mirror: fewer rows than targets, a start of the wrong size
    try {
        pa.compute_cartesian_waypoints(start, targets, S - 1, ca, c, gd);
        CHECK(false);
    } catch (const std::invalid_argument&) {
    }
    try {
        pa.compute_cartesian_waypoints(home, targets, W, ca, c, gd);
        CHECK(false);
    } catch (const std::invalid_argument&) {
    }
    std::puts("polyline C++ checks OK");
    return 0;
}
