// The validity model inside the path entry points through the C++ host mirror (pick_ik_amd/host/pick_ik_amd.hpp
// Solver::set_path_validity) against the C ABI (pikamd_set_path_validity): ik_gradient_paths with the switch off is
// the plain walk whatever model is set; with it on every path is the plain one cut at the first row the model refuses
// (pikamd_validity_batch by hand over the plain rows).  Needs a GPU; prints "pathvalid C++ checks OK".
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

static bool same_paths(const PathResult& a, const PathResult& b) {
    return a.solution.size() == b.solution.size() &&
           std::memcmp(a.solution.data(), b.solution.data(), sizeof(double) * a.solution.size()) == 0 &&
           a.status == b.status && std::memcmp(a.cost.data(), b.cost.data(), sizeof(double) * a.cost.size()) == 0 &&
           std::memcmp(a.stats.data(), b.stats.data(), sizeof(pikamd_stats) * a.stats.size()) == 0 && a.reached == b.reached;
}

int main() {
    // refusals need no model and no call
    CHECK(pikamd_set_path_validity(nullptr, 1) == PIKAMD_EINVAL);
    Solver pa(panda_chain());
    CHECK(pikamd_set_path_validity(pa.handle(), 2) == PIKAMD_EINVAL);
    CHECK(pikamd_set_path_validity(pa.handle(), -1) == PIKAMD_EINVAL);
    const int D = 7, P = 6, W = 9;
    const std::vector<double> home = {0.0, -M_PI / 4, 0.0, -3.0 * M_PI / 4, 0.0, M_PI / 2, M_PI / 4};
    // joint-space lines from home: reachable by construction
    std::vector<double> start;
    std::vector<Pose> goals;
    for (int p = 0; p < P; ++p) {
        start.insert(start.end(), home.begin(), home.end());
        for (int k = 0; k < W; ++k) {
            std::vector<double> q(home);
            for (int j = 0; j < D; ++j) q[j] += 0.35 * (k + 1.0) / W * std::sin(1.0 + 2.0 * p + 3.0 * j);
            goals.push_back(pa.fk(q));
        }
    }
    CostSpec c;
    GradientIkParams gd;
    const PathResult plain = pa.ik_gradient_paths(start, goals, W, c, gd);
    for (int p = 0; p < P; ++p) CHECK(plain.reached[p] == W);
    // the hand and the flange against one obstacle: where the hand of path 1 is at row 4
    std::vector<pikamd_sphere> spheres = {{6, 0, {0.0, 0.0, 0.14}, 0.07}, {6, 0, {0.0, 0.0, 0.0}, 0.05}, {-1, 0, {0.0, 0.0, 0.0}, 0.03}};
    const std::vector<int32_t> pairs = {0, 2, 1, 2};
    pa.set_validity_model(spheres, pairs);
    std::vector<double> cen;
    const std::vector<double> q14(plain.solution.begin() + (1 * W + 4) * D, plain.solution.begin() + (1 * W + 5) * D);
    pa.validity(q14, nullptr, &cen);
    for (int i = 0; i < 3; ++i) spheres[2].centre[i] = cen[i];
    pa.set_validity_model(spheres, pairs);
    // the switch is off: the model is ignored
    CHECK(same_paths(pa.ik_gradient_paths(start, goals, W, c, gd), plain));
    // on: the plain rows cut by hand
    std::vector<int32_t> valid((size_t)P * W);
    CHECK(pikamd_validity_batch(pa.handle(), (int64_t)P * W, plain.solution.data(), valid.data(), nullptr, nullptr) == 0);
    CHECK(valid[1 * W + 4] == 0);
    PathResult want = plain;
    int cut = 0;
    for (int p = 0; p < P; ++p) {
        int f = -1;
        for (int k = 0; k < W && f < 0; ++k)
            if (!valid[p * W + k]) f = k;
        if (f < 0) continue;
        ++cut;
        const double* held = f == 0 ? &start[(size_t)p * D] : &plain.solution[((size_t)p * W + f - 1) * D];
        for (int k = f; k < W; ++k) {
            std::memcpy(&want.solution[((size_t)p * W + k) * D], held, sizeof(double) * D);
            if (k > f) {
                want.status[p * W + k] = PIKAMD_NOT_ATTEMPTED;
                want.cost[p * W + k] = 0.0;
                std::memset(&want.stats[p * W + k], 0, sizeof(pikamd_stats));
            }
        }
        want.status[p * W + f] = PIKAMD_VALIDITY_REFUSED;
        want.reached[p] = f;
    }
    CHECK(cut >= 1 && cut < P);
    pa.set_path_validity(true);
    const PathResult got = pa.ik_gradient_paths(start, goals, W, c, gd);
    CHECK(same_paths(got, want));
    std::printf("path validity: %d of %d paths cut\n", cut, P);
    // the C ABI's switch is the mirror's; clearing the model leaves the switch on and changes nothing more
    CHECK(pikamd_set_path_validity(pa.handle(), 0) == 0);
    CHECK(same_paths(pa.ik_gradient_paths(start, goals, W, c, gd), plain));
    CHECK(pikamd_set_path_validity(pa.handle(), 1) == 0);
    CHECK(same_paths(pa.ik_gradient_paths(start, goals, W, c, gd), want));
    pa.clear_validity_model();
    CHECK(same_paths(pa.ik_gradient_paths(start, goals, W, c, gd), plain));
    pa.set_validity_model(spheres, pairs);
    CHECK(same_paths(pa.ik_gradient_paths(start, goals, W, c, gd), want));
    pa.set_path_validity(false);
    CHECK(same_paths(pa.ik_gradient_paths(start, goals, W, c, gd), plain));
    std::puts("pathvalid C++ checks OK");
    return 0;
}
