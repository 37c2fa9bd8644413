// Memetic IK with random restarts through the C++ host mirror (pick_ik_amd/host/pick_ik_amd.hpp
// Solver::ik_memetic_search_batch) against the C ABI call (pikamd_search_global_batch), against ik_memetic_batch for
// the first attempt, and against the loop's rule over the rows of every attempt.  Needs a GPU; prints
// "search global C++ checks OK".
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
    const int D = 7, B = 24, K = 4;
    const std::vector<double> home = {0.0, -M_PI / 4, 0.0, -3.0 * M_PI / 4, 0.0, M_PI / 2, M_PI / 4};
    // targets: the poses of configurations spread over the joint ranges, the last four moved out of reach; every search
    // from the ready pose, on a budget small enough for a first attempt to fail now and then
    const double lo[7] = {-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973};
    const double hi[7] = {2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973};
    std::vector<double> seeds;
    std::vector<Pose> goals;
    for (int b = 0; b < B; ++b) {
        std::vector<double> q(D);
        for (int j = 0; j < D; ++j) q[j] = 0.5 * (lo[j] + hi[j]) + 0.45 * (hi[j] - lo[j]) * std::sin(1.0 + 3.0 * b + 2.0 * j);
        Pose g = pa.fk(q);
        if (b >= B - 4) g.x += 5.0;
        goals.push_back(g);
        seeds.insert(seeds.end(), home.begin(), home.end());
    }
    CostSpec c;
    MemeticIkParams me;
    me.max_generations = 12;
    me.gd_params.max_iterations = 10;
    const uint64_t rng_seed = (7ull << 32) + 11ull;
    const SearchResult r = pa.ik_memetic_search_batch(seeds, goals, c, me, K, rng_seed, 100, false, true);
    CHECK(r.batch.solution.size() == (size_t)B * D && r.batch.status.size() == (size_t)B && r.attempts.size() == (size_t)B);
    CHECK(r.all_solution.size() == (size_t)B * K * D && r.all_status.size() == (size_t)B * K);
    // (1) the C ABI call with the same arguments: the same bytes
    const pikamd_params p = Solver::to_params(c, &me, nullptr, false);
    std::vector<double> g7;
    for (const Pose& g : goals)
        for (double v : {g.x, g.y, g.z, g.qw, g.qx, g.qy, g.qz}) g7.push_back(v);
    std::vector<double> sol((size_t)B * D), cost(B), all_sol((size_t)B * K * D);
    std::vector<int32_t> st(B), attempts(B), all_st((size_t)B * K);
    std::vector<pikamd_stats> stats(B);
    CHECK(pikamd_search_global_batch(pa.handle(), &p, B, g7.data(), seeds.data(), nullptr, rng_seed, 100, K, sol.data(),
                                     st.data(), cost.data(), stats.data(), attempts.data(), all_sol.data(),
                                     all_st.data()) == 0);
    CHECK(std::memcmp(sol.data(), r.batch.solution.data(), sizeof(double) * sol.size()) == 0);
    CHECK(std::memcmp(cost.data(), r.batch.cost.data(), sizeof(double) * cost.size()) == 0);
    CHECK(st == r.batch.status && attempts == r.attempts && all_st == r.all_status);
    CHECK(std::memcmp(stats.data(), r.batch.stats.data(), sizeof(pikamd_stats) * stats.size()) == 0);
    CHECK(std::memcmp(all_sol.data(), r.all_solution.data(), sizeof(double) * all_sol.size()) == 0);
    // (2) asking for every attempt changes nothing in the primary outputs
    const SearchResult q = pa.ik_memetic_search_batch(seeds, goals, c, me, K, rng_seed, 100);
    CHECK(q.all_solution.empty() && q.all_status.empty());
    CHECK(std::memcmp(q.batch.solution.data(), r.batch.solution.data(), sizeof(double) * sol.size()) == 0);
    CHECK(q.batch.status == r.batch.status && q.attempts == r.attempts);
    CHECK(std::memcmp(q.batch.stats.data(), r.batch.stats.data(), sizeof(pikamd_stats) * stats.size()) == 0);
    // (3) the first attempt is ik_memetic_batch from the seed with the caller's rng_seed; the primary outputs follow
    //     the loop's rule over the rows
    const BatchResult first = pa.ik_memetic_batch(seeds, goals, c, me, false, rng_seed, 100);
    int at_first = 0, later = 0, never = 0;
    for (int b = 0; b < B; ++b) {
        CHECK(r.all_status[(size_t)b * K] == first.status[b]);
        CHECK(std::memcmp(&r.all_solution[(size_t)b * K * D], &first.solution[(size_t)b * D], sizeof(double) * D) == 0);
        int win = K - 1;
        for (int a = K - 1; a >= 0; --a)
            if (r.all_status[(size_t)b * K + a] > 0) win = a;
        CHECK(r.attempts[b] == win + 1 && r.batch.status[b] == r.all_status[(size_t)b * K + win]);
        CHECK(std::memcmp(&r.batch.solution[(size_t)b * D], &r.all_solution[((size_t)b * K + win) * D], sizeof(double) * D) == 0);
        CHECK(r.batch.stats[b].cost_evals >= first.stats[b].cost_evals);
        if (win == 0) {
            CHECK(r.batch.cost[b] == first.cost[b] && r.batch.stats[b].cost_evals == first.stats[b].cost_evals);
            CHECK(r.batch.stats[b].generations == first.stats[b].generations);
        } else {
            CHECK(r.batch.stats[b].cost_evals > first.stats[b].cost_evals); // (summed over the attempts)
        }
        if (r.batch.status[b] > 0) (win == 0 ? at_first : later) += 1;
        else never += 1;
    }
    std::printf("search global: %d solved at the first attempt, %d later, %d never\n", at_first, later, never);
    CHECK(at_first >= 1 && never >= 4);
    // (4) one attempt is ik_memetic_batch
    const SearchResult one = pa.ik_memetic_search_batch(seeds, goals, c, me, 1, rng_seed, 100);
    CHECK(one.batch.status == first.status);
    CHECK(std::memcmp(one.batch.solution.data(), first.solution.data(), sizeof(double) * sol.size()) == 0);
    CHECK(std::memcmp(one.batch.cost.data(), first.cost.data(), sizeof(double) * cost.size()) == 0);
    // argument checks of the mirror and of the library behind it
    for (int bad : {0, PIKAMD_MAX_ATTEMPTS + 1}) {
        try {
            pa.ik_memetic_search_batch(seeds, goals, c, me, bad);
            CHECK(false);
        } catch (const std::invalid_argument&) {
        }
    }
    pikamd_params local = p;
    local.mode = 1;
    CHECK(pikamd_search_global_batch(pa.handle(), &local, B, g7.data(), seeds.data(), nullptr, 0, 0, K, sol.data(),
                                     st.data(), nullptr, nullptr, nullptr, nullptr, nullptr) == PIKAMD_EINVAL);
    CHECK(std::strstr(pikamd_last_error(), "pikamd_search_batch") != nullptr);
    std::puts("search global C++ checks OK");
    return 0;
}
