// Cartesian waypoint paths through the C++ host mirror (pick_ik_amd/host/pick_ik_amd.hpp Solver::ik_gradient_paths)
// against the C ABI call (pikamd_solve_paths) and against the loop of ik_gradient_batch calls it is defined by.
// Needs a GPU; prints "path C++ checks OK".
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
    const int D = 7, P = 6, W = 12;
    const std::vector<double> home = {0.0, -M_PI / 4, 0.0, -3.0 * M_PI / 4, 0.0, M_PI / 2, M_PI / 4};
    // paths: from the ready pose (each path a little off it) along a straight line of 0.05 .. 1.05 m -- the long ones
    // leave the workspace and stop inside
    std::vector<double> start;
    std::vector<Pose> goals;
    for (int p = 0; p < P; ++p) {
        std::vector<double> q = home;
        for (int j = 0; j < D; ++j) q[j] += 0.05 * std::sin(1.0 + p + 2.0 * j);
        start.insert(start.end(), q.begin(), q.end());
        const Pose f = pa.fk(q);
        const double dir[3] = {std::cos(0.25 * p), std::sin(0.25 * p) * 0.8, std::sin(0.25 * p) * 0.6}, len = 0.05 + 0.2 * p;
        for (int k = 0; k < W; ++k) {
            Pose g = f;
            const double t = len * (k + 1) / W;
            g.x += t * dir[0];
            g.y += t * dir[1];
            g.z += t * dir[2];
            goals.push_back(g);
        }
    }
    CostSpec c;
    GradientIkParams gd;
    const std::vector<double> limit(D, 0.1);
    for (int with_limit = 0; with_limit < 2; ++with_limit) {
        const PathResult r = pa.ik_gradient_paths(start, goals, W, c, gd, false, with_limit ? &limit : nullptr);
        CHECK(r.solution.size() == (size_t)P * W * D && r.status.size() == (size_t)P * W && r.reached.size() == (size_t)P);
        // (1) the C ABI call with the same arguments: the same bytes
        const pikamd_params p = Solver::to_params(c, nullptr, &gd, false);
        std::vector<double> g7;
        for (const Pose& g : goals)
            for (double v : {g.x, g.y, g.z, g.qw, g.qx, g.qy, g.qz}) g7.push_back(v);
        std::vector<double> sol((size_t)P * W * D), cost((size_t)P * W);
        std::vector<int32_t> st((size_t)P * W), reached(P);
        std::vector<pikamd_stats> stats((size_t)P * W);
        CHECK(pikamd_solve_paths(pa.handle(), &p, P, W, g7.data(), start.data(), with_limit ? limit.data() : nullptr,
                                 sol.data(), st.data(), cost.data(), stats.data(), reached.data()) == 0);
        CHECK(std::memcmp(sol.data(), r.solution.data(), sizeof(double) * sol.size()) == 0);
        CHECK(std::memcmp(cost.data(), r.cost.data(), sizeof(double) * cost.size()) == 0);
        CHECK(st == r.status && reached == r.reached);
        CHECK(std::memcmp(stats.data(), r.stats.data(), sizeof(pikamd_stats) * stats.size()) == 0);
        // (2) the loop it is defined by, one ik_gradient_batch call per waypoint and held path
        int complete = 0, stopped = 0;
        for (int pth = 0; pth < P; ++pth) {
            std::vector<double> seed(start.begin() + (size_t)pth * D, start.begin() + (size_t)(pth + 1) * D);
            bool held = true;
            int n = 0;
            for (int k = 0; k < W; ++k) {
                const size_t row = (size_t)pth * W + k;
                if (!held) {
                    CHECK(r.status[row] == PIKAMD_NOT_ATTEMPTED && r.cost[row] == 0.0 && r.stats[row].cost_evals == 0);
                    CHECK(std::memcmp(&r.solution[row * D], seed.data(), sizeof(double) * D) == 0);
                    continue;
                }
                const BatchResult b = pa.ik_gradient_batch(seed, {goals[row]}, c, gd);
                bool jump = false;
                for (int j = 0; j < D && with_limit; ++j) jump = jump || std::fabs(b.solution[j] - seed[j]) > limit[j];
                jump = jump && b.status[0] > 0;
                CHECK(r.status[row] == (jump ? PIKAMD_PATH_JUMP : b.status[0]));
                CHECK(r.cost[row] == b.cost[0] && r.stats[row].cost_evals == b.stats[0].cost_evals);
                if (b.status[0] > 0 && !jump) {
                    seed = b.solution;
                    ++n;
                } else {
                    held = false;
                }
                CHECK(std::memcmp(&r.solution[row * D], seed.data(), sizeof(double) * D) == 0);
            }
            CHECK(r.reached[pth] == n);
            complete += held ? 1 : 0;
            stopped += held ? 0 : 1;
        }
        std::printf("paths (step limit %s): %d complete, %d stopped\n", with_limit ? "0.1" : "none", complete, stopped);
        CHECK(complete >= 1 && stopped >= 1);
    }
    // argument checks of the mirror and of the library behind it
    try {
        pa.ik_gradient_paths(start, goals, 5, c, gd);
        CHECK(false);
    } catch (const std::invalid_argument&) {
    }
    std::puts("path C++ checks OK");
    return 0;
}
