// One quarter of the class-streaming head kernels (kernels_head_cls.hpp): the including translation unit names a direction
// and four class counts, OCT_HEAD_CLS_BWD (0 forward, 1 backward) and OCT_HEAD_CLS_C0 (9 or 13: C0 .. C0 + 3), and gets the
// launch function tu_head_cls.hip routes those to.  Four units, so that build.sh compiles the 32 kernels side by side.
#pragma once
#include <hip/hip_runtime.h>

#include "host.hpp"
#include "kernels_head_cls.hpp"

namespace octh {
using namespace oct;

#if OCT_HEAD_CLS_BWD
#define OCT_HEAD_CLS_KERNEL head_bwd_cls_k
#define OCT_HEAD_CLS_ARGS HeadBwdArgs
#else
#define OCT_HEAD_CLS_KERNEL head_fwd_cls_k
#define OCT_HEAD_CLS_ARGS HeadFwdArgs
#endif
#define OCT_HEAD_CLS_CAT2(a, b, c) a##b##_##c
#define OCT_HEAD_CLS_CAT(a, b, c) OCT_HEAD_CLS_CAT2(a, b, c)
// head_cls_launch_<direction>_<C0>, declared in host.hpp
#define OCT_HEAD_CLS_FN OCT_HEAD_CLS_CAT(head_cls_launch_, OCT_HEAD_CLS_BWD, OCT_HEAD_CLS_C0)

int OCT_HEAD_CLS_FN(const OCT_HEAD_CLS_ARGS& a, int C, int cin, dim3 grid, hipStream_t s) {
    constexpr int C0 = OCT_HEAD_CLS_C0;
    switch (C) {
        case C0 + 0: AT_DISPATCH(a.act_bf16, OCT_HEAD_CLS_KERNEL<C0 + 0, AT><<<grid, dim3(kBlock), 0, s>>>(a, cin)); break;
        case C0 + 1: AT_DISPATCH(a.act_bf16, OCT_HEAD_CLS_KERNEL<C0 + 1, AT><<<grid, dim3(kBlock), 0, s>>>(a, cin)); break;
        case C0 + 2: AT_DISPATCH(a.act_bf16, OCT_HEAD_CLS_KERNEL<C0 + 2, AT><<<grid, dim3(kBlock), 0, s>>>(a, cin)); break;
        case C0 + 3: AT_DISPATCH(a.act_bf16, OCT_HEAD_CLS_KERNEL<C0 + 3, AT><<<grid, dim3(kBlock), 0, s>>>(a, cin)); break;
        default: return fail(-3, "bad n_cls");
    }
    HIP_OK(hipGetLastError());
    return 0;
}

}  // namespace octh
