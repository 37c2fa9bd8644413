// pik_validity.hpp -- the sphere validity test (pikamd_validity_batch, and the step of the restart searches that
// stands where searchPositionIK calls the solution callback, src/pick_ik_plugin.cpp:269-274).
//
// The robot as spheres fixed to its links, obstacles as spheres fixed in the base frame, a list of sphere pairs that
// must not overlap (include/pick_ik_amd.h has the normative definition).  One lane per candidate walks the chain ONCE:
// the loop is fk's literal loop (pik_math.hpp, PIK_STRICT) statement for statement, without the floating and the mimic
// branches -- the first origin copied while `blank`, chain_origin, sincos_f64, chain_joint -- and behind joint v the
// centres of the spheres attached there are emitted by the translation rows of the iso_mul the tip transform gets
// (fk's `if (!tip_ident)`: an all-zero local centre is the frame's origin t as it is).  That is what makes a centre the
// position pikamd_fk_batch returns for the chain cut behind variable v with the centre as its tip, bit for bit.
//
// Compiled with the exact flavours' flags only (-ffp-contract=off for the whole translation unit; the fused flavour's
// multiply-adds are the stated ones of pik_math.hpp): the chain product of fk exists only where PIK_STRICT is defined,
// and one arithmetic serves every handle whatever kernels solve its calls.  The model and the chain's constants are a
// device buffer of their own (ValidityImage), read through the constant address space with wave-uniform addresses.
//
// A lane's centres -- at most 3 * PIKAMD_MAX_SPHERES = 96 doubles -- live in LDS, one column per lane: they are
// written in chain order and read by pair index, and a per-lane array indexed so would be scratch memory.  The kernels
// ask for 3 * n_spheres * 64 doubles of dynamic LDS (48 KiB at the cap), one wavefront per block.
#pragma once

#if !defined(PIK_STRICT)
#error "pik_validity.hpp: the exact flavours only (fk's chain product is compiled where PIK_STRICT is defined)"
#endif

#include "pik_math.hpp"
#include "pik_validity_ops.hpp"

namespace pik {

constexpr int VALIDITY_WAVE = 64;

template <int D>
struct ValidityImage {
    ChainK<D> chain;
    ValidityModelK model;
};

using VM = const PIK_CONSTANT ValidityModelK&;

// The test of one candidate q.  store[(3 * k + i) * stride]: component i of the centre of sphere k (caller's index),
// written for all n_spheres.  Returns valid; clearance: the smallest clear_m (+infinity without a pair).
template <int D>
__device__ __forceinline__ bool validity_clear(CK<D> c, VM m, const double (&q)[D], double* store, int stride,
                                               double& clearance) {
    const int n_spheres = m.n_spheres, n_pairs = m.n_pairs;
    const uint32_t zero_mask = m.zero_mask;
    int k = 0; // the next sphere in chain order (wave-uniform)
    // spheres fixed in the base frame: copied
#pragma unroll 1
    for (; k < n_spheres && m.after[k] < 0; ++k) {
        const int dst = 3 * m.index[k];
        store[(dst + 0) * stride] = m.centre[k][0];
        store[(dst + 1) * stride] = m.centre[k][1];
        store[(dst + 2) * stride] = m.centre[k][2];
    }
    // fk's literal loop (pik_math.hpp fk, PIK_STRICT), one tip frame, no floating and no mimic joint
    const uint32_t prismatic_mask = c.prismatic_mask;
    const uint32_t kinds = c.axis_kind;
    double R[9], t[3];
    R[0] = 1.0; R[1] = 0.0; R[2] = 0.0;
    R[3] = 0.0; R[4] = 1.0; R[5] = 0.0;
    R[6] = 0.0; R[7] = 0.0; R[8] = 1.0;
    t[0] = t[1] = t[2] = 0.0;
    bool blank = true;
#pragma unroll 1
    for (int j = 0; j < D; ++j) {
        const double qj = q[j];
        chain_origin<D>(c, j, R, t, blank);
        const bool pj = (prismatic_mask >> j) & 1u;
        double sn = 0.0, cs = 1.0;
        if (!pj) sincos_f64(c.mt, qj, sn, cs);
        chain_joint<D>(c, j, R, t, pj, (kinds >> (2 * j)) & 3u, qj, sn, cs);
        blank = false;
        // the spheres of the link behind joint j: the translation rows of iso_mul(R, t, (1, centre))
#pragma unroll 1
        for (; k < n_spheres && m.after[k] == j; ++k) {
            const int dst = 3 * m.index[k];
            if ((zero_mask >> k) & 1u) {
                store[(dst + 0) * stride] = t[0];
                store[(dst + 1) * stride] = t[1];
                store[(dst + 2) * stride] = t[2];
            } else {
                const double o9 = m.centre[k][0], o10 = m.centre[k][1], o11 = m.centre[k][2];
#pragma unroll
                for (int i = 0; i < 3; ++i) {
#if PIK_XF
                    store[(dst + i) * stride] =
                        fma_f64(R[i * 3 + 2], o11, fma_f64(R[i * 3 + 1], o10, fma_f64(R[i * 3 + 0], o9, t[i])));
#else
                    store[(dst + i) * stride] = R[i * 3 + 0] * o9 + R[i * 3 + 1] * o10 + R[i * 3 + 2] * o11 + t[i];
#endif
                }
            }
        }
    }
    // the pairs, ascending: every operation rounded on its own, IEEE square root
    bool valid = true;
    clearance = HUGE_VAL;
#pragma unroll 1
    for (int p = 0; p < n_pairs; ++p) {
        const int a = m.pairs[p][0], b = m.pairs[p][1];
        const double dx = store[(3 * a + 0) * stride] - store[(3 * b + 0) * stride];
        const double dy = store[(3 * a + 1) * stride] - store[(3 * b + 1) * stride];
        const double dz = store[(3 * a + 2) * stride] - store[(3 * b + 2) * stride];
        const double xx = dx * dx, yy = dy * dy, zz = dz * dz;
        const double xy = xx + yy;
        const double d2 = xy + zz;
        const double rr = m.radius[a] + m.radius[b];
        const double clear = sqrt(d2) - rr;
        if (clear < clearance) clearance = clear; // (a NaN never replaces)
        if (clear < 0.0) valid = false;           // (a NaN does not trip the test)
    }
    return valid;
}

#define PIK_VALIDITY_IMAGE(img)                                                                           \
    const PIK_CONSTANT ValidityImage<D>* const vi_ = (const PIK_CONSTANT ValidityImage<D>*)(img);         \
    CK<D> c = vi_->chain;                                                                                 \
    VM m = vi_->model

// pikamd_validity_batch_device: one lane per candidate
template <int D>
__global__ __launch_bounds__(VALIDITY_WAVE) void validity_kernel(const ValidityImage<D>* __restrict__ img, long long n,
                                                                 const double* __restrict__ q, int* __restrict__ valid,
                                                                 double* __restrict__ clearance,
                                                                 double* __restrict__ centres) {
    extern __shared__ double validity_lds[];
    PIK_VALIDITY_IMAGE(img);
    const long long i = (long long)blockIdx.x * VALIDITY_WAVE + threadIdx.x;
    if (i >= n) return; // (no barrier below: a lane only touches its own LDS column)
    double qq[D];
#pragma unroll
    for (int j = 0; j < D; ++j) qq[j] = q[i * D + j];
    double* col = validity_lds + threadIdx.x;
    double clear;
    const bool ok = validity_clear<D>(c, m, qq, col, VALIDITY_WAVE, clear);
    valid[i] = ok ? 1 : 0;
    if (clearance) clearance[i] = clear;
    if (centres) {
        const int n3 = 3 * m.n_spheres;
        double* o = centres + i * n3;
#pragma unroll 1
        for (int e = 0; e < n3; ++e) o[e] = col[e * VALIDITY_WAVE];
    }
}

// The step of pikamd_search_global_batch*, between the gate and the fold of an attempt, one lane per problem: the rows
// restart_gate_kernel visits (the attempt ran for the problem, its status is > 0) are tested, and a refused row is
// rewritten as that kernel rewrites one -- PIKAMD_VALIDITY_REFUSED and the seed; its cost and counters stay.
template <int D>
__global__ __launch_bounds__(VALIDITY_WAVE) void validity_rows_kernel(const ValidityImage<D>* __restrict__ img,
                                                                      ValidityRows r) {
    extern __shared__ double validity_lds[];
    PIK_VALIDITY_IMAGE(img);
    const long long b = (long long)blockIdx.x * VALIDITY_WAVE + threadIdx.x;
    if (b >= r.B) return;
    const bool ran = r.every != 0 || r.open[b] != 0;
    if (!ran || !(r.row_status[b] > 0)) return;
    double qq[D];
#pragma unroll
    for (int j = 0; j < D; ++j) qq[j] = r.row_solution[b * D + j];
    double clear;
    if (validity_clear<D>(c, m, qq, validity_lds + threadIdx.x, VALIDITY_WAVE, clear)) return;
    r.row_status[b] = PIKAMD_VALIDITY_REFUSED_K;
#pragma unroll
    for (int j = 0; j < D; ++j) r.row_solution[b * D + j] = r.seed[b * D + j];
}

template <int D>
void validity_pack(const pikamd_solver* s, const ValidityModelK& m, void* image) {
    ValidityImage<D>& img = *static_cast<ValidityImage<D>*>(image);
    std::memset(&img, 0, sizeof img);
    img.chain = make_chain_k<D>(s->chain);
    img.model = m;
}

inline size_t validity_lds_bytes(int n_spheres) { return sizeof(double) * 3 * (size_t)n_spheres * VALIDITY_WAVE; }

template <int D>
int launch_validity(const void* d_image, int n_spheres, long long n, const double* d_q, int* d_valid, double* d_clear,
                    double* d_centres, hipStream_t st) {
    if (n == 0) return 0;
    const long long grid = (n + VALIDITY_WAVE - 1) / VALIDITY_WAVE;
    if (grid > 0x7fffffffLL) return fail(PIKAMD_EINVAL, "pikamd_validity_batch: n = %lld is more than one launch holds", n);
    hipLaunchKernelGGL(validity_kernel<D>, dim3((unsigned)grid), dim3(VALIDITY_WAVE), validity_lds_bytes(n_spheres), st,
                       static_cast<const ValidityImage<D>*>(d_image), n, d_q, d_valid, d_clear, d_centres);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
int launch_validity_rows(const void* d_image, int n_spheres, const ValidityRows& r, hipStream_t st) {
    if (r.B == 0) return 0;
    const long long grid = (r.B + VALIDITY_WAVE - 1) / VALIDITY_WAVE;
    hipLaunchKernelGGL(validity_rows_kernel<D>, dim3((unsigned)grid), dim3(VALIDITY_WAVE), validity_lds_bytes(n_spheres),
                       st, static_cast<const ValidityImage<D>*>(d_image), r);
    HIP_TRY(hipGetLastError());
    return 0;
}

template <int D>
const ValidityOps* make_validity_ops() {
    static const ValidityOps ops = {sizeof(ValidityImage<D>), &validity_pack<D>, &launch_validity<D>,
                                    &launch_validity_rows<D>};
    return &ops;
}

} // namespace pik
