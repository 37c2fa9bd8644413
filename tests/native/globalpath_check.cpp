// Cartesian paths from a pose with a memetic start through the C++ host mirror (pick_ik_amd/host/pick_ik_amd.hpp
// Solver::ik_memetic_search_paths) against the C ABI call (pikamd_search_global_paths) and, with one attempt, against
// the ik_memetic_batch + ik_gradient_paths calls it is defined by.  Needs a GPU; prints "globalpath C++ checks OK".
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
    const int D = 7, P = 6, W = 5, K = 4;
    const std::vector<double> home = {0.0, -M_PI / 4, 0.0, -3.0 * M_PI / 4, 0.0, M_PI / 2, M_PI / 4};
    // paths: every search is seeded with the ready pose; the lines start at configurations 0.3 rad off it and run
    // 0.05 .. 1.05 m -- the long ones leave the workspace
    std::vector<double> seeds;
    std::vector<Pose> goals;
    for (int p = 0; p < P; ++p) {
        std::vector<double> q = home;
        for (int j = 0; j < D; ++j) q[j] += 0.3 * std::sin(1.0 + p + 2.0 * j);
        seeds.insert(seeds.end(), home.begin(), home.end());
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
    MemeticIkParams mp;
    mp.max_generations = 12;
    mp.gd_params.max_iterations = 10;
    // the waypoints behind the first: ik_gradient with the memetic call's step size, cost delta and stop rule
    GradientIkParams gd;
    gd.step_size = mp.gd_params.step_size;
    gd.min_cost_delta = mp.gd_params.min_cost_delta;
    gd.stop_optimization_on_valid_solution = mp.stop_optimization_on_valid_solution;
    const std::vector<double> limit(D, 0.15);
    pikamd_params p = Solver::to_params(c, &mp, nullptr, false);
    p.gd_max_iters = gd.max_iterations;
    std::vector<double> g7;
    for (const Pose& g : goals)
        for (double v : {g.x, g.y, g.z, g.qw, g.qx, g.qy, g.qz}) g7.push_back(v);
    for (int with_limit = 0; with_limit < 2; ++with_limit) {
        // (1) the C ABI call with the same arguments: the same bytes
        const SearchPathsResult r = pa.ik_memetic_search_paths(seeds, goals, W, c, mp, K, 1, 3, false,
                                                               with_limit ? &limit : nullptr, nullptr, gd.max_iterations);
        CHECK(r.paths.solution.size() == (size_t)P * W * D && r.paths.status.size() == (size_t)P * W);
        CHECK(r.paths.reached.size() == (size_t)P && r.attempts.size() == (size_t)P && r.totals.size() == (size_t)P);
        std::vector<double> sol((size_t)P * W * D), cost((size_t)P * W);
        std::vector<int32_t> st((size_t)P * W), reached(P), attempts(P);
        std::vector<pikamd_stats> stats((size_t)P * W), totals(P);
        CHECK(pikamd_search_global_paths(pa.handle(), &p, P, W, g7.data(), seeds.data(), nullptr,
                                         with_limit ? limit.data() : nullptr, 1, 3, K, sol.data(), st.data(), cost.data(),
                                         stats.data(), reached.data(), attempts.data(), totals.data()) == 0);
        CHECK(std::memcmp(sol.data(), r.paths.solution.data(), sizeof(double) * sol.size()) == 0);
        CHECK(std::memcmp(cost.data(), r.paths.cost.data(), sizeof(double) * cost.size()) == 0);
        CHECK(st == r.paths.status && reached == r.paths.reached && attempts == r.attempts);
        CHECK(std::memcmp(stats.data(), r.paths.stats.data(), sizeof(pikamd_stats) * stats.size()) == 0);
        CHECK(std::memcmp(totals.data(), r.totals.data(), sizeof(pikamd_stats) * totals.size()) == 0);
        int complete = 0, open = 0;
        for (int pth = 0; pth < P; ++pth) {
            CHECK(r.attempts[pth] >= 1 && r.attempts[pth] <= K && r.paths.reached[pth] >= 0 && r.paths.reached[pth] <= W);
            CHECK((r.paths.reached[pth] == W) || r.attempts[pth] == K);
            complete += r.paths.reached[pth] == W;
            open += r.paths.reached[pth] != W;
        }
        std::printf("search global paths (step limit %s): %d complete, %d never\n", with_limit ? "0.15" : "none", complete, open);
        CHECK(complete >= 1 && open >= 1);
        // (2) one attempt: one ik_memetic_batch for waypoint 0 (the path's problem offset), one ik_gradient_paths behind it
        const SearchPathsResult one = pa.ik_memetic_search_paths(seeds, goals, W, c, mp, 1, 1, 3, false,
                                                                 with_limit ? &limit : nullptr, nullptr, gd.max_iterations);
        for (int pth = 0; pth < P; ++pth) {
            const size_t row0 = (size_t)pth * W;
            const BatchResult b = pa.ik_memetic_batch(home, {goals[row0]}, c, mp, false, 1, 3 + pth);
            CHECK(one.attempts[pth] == 1);
            CHECK(one.paths.status[row0] == b.status[0] && one.paths.cost[row0] == b.cost[0]);
            CHECK(one.paths.stats[row0].cost_evals == b.stats[0].cost_evals);
            CHECK(std::memcmp(&one.paths.solution[row0 * D], b.solution.data(), sizeof(double) * D) == 0);
            int64_t evals = b.stats[0].cost_evals;
            if (b.status[0] > 0) {
                const std::vector<Pose> rest(goals.begin() + row0 + 1, goals.begin() + row0 + W);
                const PathResult pr = pa.ik_gradient_paths(b.solution, rest, W - 1, c, gd, false, with_limit ? &limit : nullptr);
                CHECK(one.paths.reached[pth] == 1 + pr.reached[0]);
                for (int k = 1; k < W; ++k) {
                    CHECK(one.paths.status[row0 + k] == pr.status[k - 1] && one.paths.cost[row0 + k] == pr.cost[k - 1]);
                    CHECK(std::memcmp(&one.paths.solution[(row0 + k) * D], &pr.solution[(size_t)(k - 1) * D], sizeof(double) * D) == 0);
                    evals += pr.stats[k - 1].cost_evals;
                }
            } else {
                CHECK(one.paths.reached[pth] == 0);
                for (int k = 1; k < W; ++k) {
                    CHECK(one.paths.status[row0 + k] == PIKAMD_NOT_ATTEMPTED && one.paths.cost[row0 + k] == 0.0);
                    CHECK(std::memcmp(&one.paths.solution[(row0 + k) * D], home.data(), sizeof(double) * D) == 0);
                }
            }
            CHECK(one.totals[pth].cost_evals == evals);
        }
    }
    // argument checks of the mirror
    try {
        pa.ik_memetic_search_paths(seeds, goals, 4, c, mp, K);
        CHECK(false);
    } catch (const std::invalid_argument&) {
    }
    try {
        pa.ik_memetic_search_paths(seeds, goals, W, c, mp, PIKAMD_MAX_ATTEMPTS + 1);
        CHECK(false);
    } catch (const std::invalid_argument&) {
    }
    std::puts("globalpath C++ checks OK");
    return 0;
}
