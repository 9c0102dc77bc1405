// One unit of head kernel instantiations (host.hpp OCT_HEAD_UNITS): the including translation unit names a family, a
// direction and a class range,
//     OCT_HEAD_FAMILY  0 register | 1 channel-streaming | 2 class-streaming   (HeadRoute)
//     OCT_HEAD_BWD     0 forward | 1 backward
//     OCT_HEAD_C0, OCT_HEAD_C1   first and last class count
// and gets head_unit_<family>_<direction>_<first C>, which launches the kernel of that family for C classes (and, register
// family, for cin input channels) on the grid it is handed.  The checks, the profiler name and the choice of the unit are
// tu_head.hip's.
#pragma once
#include <hip/hip_runtime.h>

#include "host.hpp"
#include "kernels_head_cls.hpp"

namespace octh {
using namespace oct;

#define OCT_HEAD_UNIT_IS(fam, dir, c0, c1) || (fam == OCT_HEAD_FAMILY && dir == OCT_HEAD_BWD && c0 == OCT_HEAD_C0 && c1 == OCT_HEAD_C1)
static_assert(false OCT_HEAD_UNITS(OCT_HEAD_UNIT_IS), "this unit's family / direction / class range is not a row of OCT_HEAD_UNITS (host.hpp)");
#undef OCT_HEAD_UNIT_IS

#define OCT_HEAD_CAT2(a, b, c, d) a##b##_##c##_##d
#define OCT_HEAD_CAT(a, b, c, d) OCT_HEAD_CAT2(a, b, c, d)
#define OCT_HEAD_FN OCT_HEAD_CAT(head_unit_, OCT_HEAD_FAMILY, OCT_HEAD_BWD, OCT_HEAD_C0)
#if OCT_HEAD_BWD
#define OCT_HEAD_ARGS HeadBwdArgs
#define OCT_HEAD_K(family) head_bwd_##family
#else
#define OCT_HEAD_ARGS HeadFwdArgs
#define OCT_HEAD_K(family) head_fwd_##family
#endif

namespace {
template <int C>
int head_unit_launch(const OCT_HEAD_ARGS& a, int cin, dim3 grid, hipStream_t s) {
#if OCT_HEAD_FAMILY == 0
    switch (cin) {      // one instantiation per start_neurons up to 32
#define OCT_HEAD_CIN(N) case N: AT_DISPATCH(a.act_bf16, OCT_HEAD_K(k)<C, N, AT><<<grid, dim3(kBlock), 0, s>>>(a)); break;
        OCT_HEAD_CIN(4) OCT_HEAD_CIN(8) OCT_HEAD_CIN(12) OCT_HEAD_CIN(16) OCT_HEAD_CIN(20) OCT_HEAD_CIN(24) OCT_HEAD_CIN(28) OCT_HEAD_CIN(32)
#undef OCT_HEAD_CIN
        default: return fail(-3, "head: unsupported start_neurons");
    }
#elif OCT_HEAD_FAMILY == 1
    AT_DISPATCH(a.act_bf16, OCT_HEAD_K(wide_k)<C, AT><<<grid, dim3(kBlock), 0, s>>>(a, cin));
#else
    AT_DISPATCH(a.act_bf16, OCT_HEAD_K(cls_k)<C, AT><<<grid, dim3(kBlock), 0, s>>>(a, cin));
#endif
    HIP_OK(hipGetLastError());
    return 0;
}
// the unit's class counts, one after the other
template <int C>
int head_unit_pick(const OCT_HEAD_ARGS& a, int n_cls, int cin, dim3 grid, hipStream_t s) {
    if constexpr (C > OCT_HEAD_C1) return fail(-3, "bad n_cls");
    else return n_cls == C ? head_unit_launch<C>(a, cin, grid, s) : head_unit_pick<C + 1>(a, n_cls, cin, grid, s);
}
}  // namespace

int OCT_HEAD_FN(const OCT_HEAD_ARGS& a, int C, int cin, dim3 grid, hipStream_t s) { return head_unit_pick<OCT_HEAD_C0>(a, C, cin, grid, s); }

}  // namespace octh
