// The sphere validity model through the C++ host mirror (pick_ik_amd/host/pick_ik_amd.hpp Solver::set_validity_model,
// clear_validity_model, validity) against the C ABI (pikamd_set_validity_model, pikamd_validity_batch + the two search
// entry points), and the first attempt of a validated search against the plain one + the test by hand.  Needs a GPU;
// prints "validity C++ checks OK".
#include <algorithm>
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

static bool same_bytes(const std::vector<double>& a, const std::vector<double>& b) {
    return a.size() == b.size() && std::memcmp(a.data(), b.data(), sizeof(double) * a.size()) == 0;
}

static bool same_result(const SearchResult& a, const SearchResult& b) {
    return same_bytes(a.batch.solution, b.batch.solution) && same_bytes(a.batch.cost, b.batch.cost) &&
           a.batch.status == b.batch.status && a.attempts == b.attempts && same_bytes(a.all_solution, b.all_solution) &&
           a.all_status == b.all_status &&
           std::memcmp(a.batch.stats.data(), b.batch.stats.data(), sizeof(pikamd_stats) * a.batch.stats.size()) == 0;
}

int main() {
    Solver pa(panda_chain());
    const int D = 7, B = 24, K = 4;
    const std::vector<double> home = {0.0, -M_PI / 4, 0.0, -3.0 * M_PI / 4, 0.0, M_PI / 2, M_PI / 4};
    const double lo[7] = {-2.8973, -1.7628, -2.8973, -3.0718, -2.8973, -0.0175, -2.8973};
    const double hi[7] = {2.8973, 1.7628, 2.8973, -0.0698, 2.8973, 3.7525, 2.8973};
    std::vector<double> seeds;
    std::vector<Pose> goals;
    for (int b = 0; b < B; ++b) {
        std::vector<double> q(D);
        for (int j = 0; j < D; ++j) q[j] = 0.5 * (lo[j] + hi[j]) + 0.45 * (hi[j] - lo[j]) * std::sin(1.0 + 3.0 * b + 2.0 * j);
        goals.push_back(pa.fk(q));
        seeds.insert(seeds.end(), home.begin(), home.end());
    }
    CostSpec c;
    c.minimal_displacement_weight = 0.001;
    c.cost_threshold = 3.0e-4;
    GradientIkParams gd;
    const uint64_t rng_seed = (7ull << 32) + 11ull;
    const pikamd_params p = Solver::to_params(c, nullptr, &gd, true);
    std::vector<double> g7;
    for (const Pose& g : goals)
        for (double v : {g.x, g.y, g.z, g.qw, g.qx, g.qy, g.qz}) g7.push_back(v);
    // the hand, the flange (the last frame's origin), the forearm and two obstacles in the base frame
    const std::vector<pikamd_sphere> spheres = {{6, 0, {0.0, 0.0, 0.14}, 0.07},  {6, 0, {0.0, 0.0, 0.0}, 0.05},
                                                {4, 0, {0.0, 0.04, -0.18}, 0.08}, {-1, 0, {0.25, 0.3, 0.6}, 0.2},
                                                {-1, 0, {0.45, -0.2, 0.45}, 0.15}};
    const std::vector<int32_t> pairs = {0, 3, 0, 4, 1, 3, 1, 4, 2, 3, 2, 4};
    const int NS = (int)spheres.size();

    // (1) without a model: pikamd_validity_batch is refused, the search is the plain one
    double clearance = 0.0;
    bool threw = false;
    try {
        pa.validity(home);
    } catch (const std::runtime_error&) {
        threw = true;
    }
    CHECK(threw);
    const SearchResult plain = pa.ik_gradient_search_batch(seeds, goals, c, gd, K, rng_seed, 100, true, true);
    for (int b = 0; b < B; ++b) CHECK(plain.attempts[b] == 1 && plain.batch.status[b] > 0);
    // (2) Solver::validity on its answers is pikamd_validity_batch; the flange is where fk of the chain without a tip
    // transform puts it (pikamd_fk_batch of the cut chain: the definition)
    pa.set_validity_model(spheres, pairs);
    std::vector<int32_t> valid(B);
    std::vector<double> clear(B), centres((size_t)B * NS * 3);
    CHECK(pikamd_validity_batch(pa.handle(), B, plain.batch.solution.data(), valid.data(), clear.data(), centres.data()) == 0);
    Chain flange = panda_chain();
    flange.tip_xyz = {0, 0, 0};
    flange.tip_rpy = {0, 0, 0};
    Solver cut(flange);
    int accepted = 0, refused = 0;
    for (int b = 0; b < B; ++b) {
        const std::vector<double> q(plain.batch.solution.begin() + b * D, plain.batch.solution.begin() + (b + 1) * D);
        std::vector<double> cen;
        CHECK(pa.validity(q, &clearance, &cen) == (valid[b] != 0));
        CHECK(clearance == clear[b] && (valid[b] != 0) == !(clear[b] < 0.0));
        CHECK((int)cen.size() == 3 * NS && std::memcmp(cen.data(), &centres[(size_t)b * NS * 3], sizeof(double) * 3 * NS) == 0);
        const Pose at = cut.fk(q);
        CHECK(cen[3] == at.x && cen[4] == at.y && cen[5] == at.z);
        CHECK(cen[9] == 0.25 && cen[10] == 0.3 && cen[11] == 0.6);
        (valid[b] ? accepted : refused) += 1;
    }
    std::printf("validity: %d valid, %d refused at attempt 0\n", accepted, refused);
    CHECK(accepted >= 1 && refused >= 1);
    // (3) the validated search through the mirror is the C ABI's, and its first row is (1) + (2)
    const SearchResult r = pa.ik_gradient_search_batch(seeds, goals, c, gd, K, rng_seed, 100, true, true);
    SearchResult abi = r;
    for (auto* v : {&abi.batch.solution, &abi.batch.cost, &abi.all_solution}) std::fill(v->begin(), v->end(), -1.0);
    CHECK(pikamd_search_batch(pa.handle(), &p, B, g7.data(), seeds.data(), nullptr, rng_seed, 100, K,
                              abi.batch.solution.data(), abi.batch.status.data(), abi.batch.cost.data(),
                              abi.batch.stats.data(), abi.attempts.data(), abi.all_solution.data(),
                              abi.all_status.data()) == 0);
    CHECK(same_result(r, abi));
    int later = 0, never = 0;
    for (int b = 0; b < B; ++b) {
        const size_t row = (size_t)b * K;
        CHECK(r.all_status[row] == (valid[b] ? plain.batch.status[b] : PIKAMD_VALIDITY_REFUSED));
        CHECK(std::memcmp(&r.all_solution[row * D], valid[b] ? &plain.batch.solution[(size_t)b * D] : &seeds[(size_t)b * D],
                          sizeof(double) * D) == 0);
        CHECK((r.attempts[b] == 1) == (valid[b] != 0));
        if (!valid[b]) (r.batch.status[b] > 0 ? later : never) += 1;
        if (!(r.batch.status[b] > 0)) CHECK(r.batch.status[b] == PIKAMD_VALIDITY_REFUSED && r.attempts[b] == K);
    }
    std::printf("validated search: %d valid at once, %d later, %d never\n", accepted, later, never);
    // (4) the same for the memetic search
    MemeticIkParams m;
    m.population_size = 16;
    m.elite_size = 4;
    m.max_generations = 6;
    m.gd_params.max_iterations = 10;
    const pikamd_params pm = Solver::to_params(c, &m, nullptr, true);
    const SearchResult rg = pa.ik_memetic_search_batch(seeds, goals, c, m, K, rng_seed, 100, true, true);
    SearchResult abig = rg;
    for (auto* v : {&abig.batch.solution, &abig.batch.cost, &abig.all_solution}) std::fill(v->begin(), v->end(), -1.0);
    CHECK(pikamd_search_global_batch(pa.handle(), &pm, B, g7.data(), seeds.data(), nullptr, rng_seed, 100, K,
                                     abig.batch.solution.data(), abig.batch.status.data(), abig.batch.cost.data(),
                                     abig.batch.stats.data(), abig.attempts.data(), abig.all_solution.data(),
                                     abig.all_status.data()) == 0);
    CHECK(same_result(rg, abig));
    int refused_rows = 0;
    for (int32_t s : rg.all_status) refused_rows += s == PIKAMD_VALIDITY_REFUSED;
    CHECK(refused_rows >= 1);
    // (5) without the model again: (1)
    pa.clear_validity_model();
    CHECK(same_result(pa.ik_gradient_search_batch(seeds, goals, c, gd, K, rng_seed, 100, true, true), plain));
    // refusals of the C ABI
    CHECK(pikamd_validity_batch(pa.handle(), B, seeds.data(), valid.data(), nullptr, nullptr) == PIKAMD_EINVAL);
    pa.set_validity_model(spheres, pairs);
    CHECK(pikamd_validity_batch(pa.handle(), B, nullptr, valid.data(), nullptr, nullptr) == PIKAMD_EINVAL);
    CHECK(pikamd_validity_batch(pa.handle(), B, seeds.data(), nullptr, nullptr, nullptr) == PIKAMD_EINVAL);
    CHECK(pikamd_validity_batch(pa.handle(), 0, nullptr, nullptr, nullptr, nullptr) == 0);
    CHECK(pikamd_validity_batch(pa.handle(), B, seeds.data(), valid.data(), nullptr, nullptr) == 0);
    std::puts("validity C++ checks OK");
    return 0;
}
