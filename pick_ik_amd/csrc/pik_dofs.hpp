// pik_dofs.hpp -- the chain lengths the library is built for, written out ONCE, and what is generated from the list:
// the per-length ops functions a kernel family's translation units export (declarations, lookup, definition) and the
// memetic kernel variants the routed and the restart launcher name.  Host-side macros only, no device code; not read
// by pik_inst.hip (whose launch_ops_d<N> / launch_ops() in pik_solver.hpp stay written out by hand: pik_solver.hpp is
// part of the text pick_ik_amd/build.py flavour_sha hashes, and the pinned hashes say that text is untouched).
#pragma once

// X(N, ...) for N = 1..16
#define PIK_FOR_EACH_DOF(X, ...)                                                                                       \
    X(1, __VA_ARGS__) X(2, __VA_ARGS__) X(3, __VA_ARGS__) X(4, __VA_ARGS__) X(5, __VA_ARGS__) X(6, __VA_ARGS__)          \
    X(7, __VA_ARGS__) X(8, __VA_ARGS__) X(9, __VA_ARGS__) X(10, __VA_ARGS__) X(11, __VA_ARGS__) X(12, __VA_ARGS__)       \
    X(13, __VA_ARGS__) X(14, __VA_ARGS__) X(15, __VA_ARGS__) X(16, __VA_ARGS__)

#define PIK_CAT2(a, b) a##b
#define PIK_CAT(a, b) PIK_CAT2(a, b)

// A kernel family's ops tables: `const TYPE* <stem>_ops_d<N>()` for every length -- defined by the family's
// instantiation file, one translation unit per length -- and the lookup `<stem>_ops(dof)` (null: no such length).
#define PIK_DECLARE_OPS_D(N, TYPE, STEM) const TYPE* STEM##_ops_d##N();
#define PIK_OPS_CASE_D(N, TYPE, STEM) case N: return STEM##_ops_d##N();
#define PIK_DECLARE_OPS_FAMILY(TYPE, STEM)                                                                             \
    PIK_FOR_EACH_DOF(PIK_DECLARE_OPS_D, TYPE, STEM)                                                                    \
    inline const TYPE* STEM##_ops(int dof) {                                                                           \
        switch (dof) {                                                                                                 \
            PIK_FOR_EACH_DOF(PIK_OPS_CASE_D, TYPE, STEM)                                                               \
            default: return nullptr;                                                                                   \
        }                                                                                                              \
    }

#if defined(PIK_INST_D)
// ... and, in an instantiation file (-DPIK_INST_D=<dof>), the definition for its length: make_<stem>_ops<dof>(), or
// null with -DPIK_INST_STUB (experiment builds: nothing for this length)
#if defined(PIK_INST_STUB)
#define PIK_DEFINE_OPS(TYPE, STEM) const TYPE* PIK_CAT(STEM##_ops_d, PIK_INST_D)() { return nullptr; }
#else
#define PIK_DEFINE_OPS(TYPE, STEM) const TYPE* PIK_CAT(STEM##_ops_d, PIK_INST_D)() { return make_##STEM##_ops<PIK_INST_D>(); }
#endif

// The memetic kernel variants (lanes per elite, several tip frames?, wavefronts per SIMD) a launcher outside
// pik_inst.hip names.  They are NOT compiled there: each is declared as an explicit instantiation that lives in the
// flavour's pik_inst object of this length.  Both launchers go through the shared switch from a variant id to its
// kernel (pik_launch.hpp with_variant_kernel), which names all of them -- the routed launcher enqueues the forms for
// one tip frame only.  The two-per-SIMD build exists up to nine joints; the 16 / 8-lane forms for several tips are
// the product flavours' cooperative descent.
#if PIK_INST_D <= 9
#define PIK_MEMETIC_TWO_PER_SIMD(X) X(1, false, 2)
#else
#define PIK_MEMETIC_TWO_PER_SIMD(X)
#endif
#if !defined(PIK_STRICT)
#define PIK_MEMETIC_WIDE_MULTI(X) X(16, true, 1) X(8, true, 1)
#else
#define PIK_MEMETIC_WIDE_MULTI(X)
#endif
#define PIK_MEMETIC_ONE_TIP(X) X(16, false, 1) X(8, false, 1) X(4, false, 1) X(2, false, 1) X(1, false, 1) PIK_MEMETIC_TWO_PER_SIMD(X)
#define PIK_MEMETIC_ALL(X) PIK_MEMETIC_ONE_TIP(X) PIK_MEMETIC_WIDE_MULTI(X) X(2, true, 1) X(1, true, 1)
#define PIK_EXTERN_MEMETIC(LPE, MULTI, OCC)                                                                            \
    extern template __global__ void memetic_kernel<PIK_INST_D, LPE, MULTI, OCC>(const ConstsK<PIK_INST_D>* __restrict__, \
                                                                                 SolveArgs);
#endif
