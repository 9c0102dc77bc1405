// One translation unit of liboct_unet_hip.so (see host.hpp): the channel-streaming head kernels (kernels_head_wide.hpp),
// head_fwd_wide_k<C, AT> / head_bwd_wide_k<C, AT> for C = 2..8 classes and both activation storage types, behind the two
// launchers oct_unet.hip routes start_neurons > 32 (or every width, option "head_wide") to.  Neither allocates or waits.
// More than 8 classes never come here: at every width they take the class-streaming kernels (tu_head_cls.hip).
#include <hip/hip_runtime.h>

#include <cstdio>

#include "host.hpp"
#include "kernels_head_wide.hpp"

using namespace oct;

namespace octh {

namespace {
template <int C>
int fwd_c(const HeadFwdArgs& a, int cin, dim3 grid, hipStream_t s) {
    AT_DISPATCH(a.act_bf16, head_fwd_wide_k<C, AT><<<grid, dim3(kBlock), 0, s>>>(a, cin));
    HIP_OK(hipGetLastError());
    return 0;
}
template <int C>
int bwd_c(const HeadBwdArgs& a, int cin, dim3 grid, hipStream_t s) {
    AT_DISPATCH(a.act_bf16, head_bwd_wide_k<C, AT><<<grid, dim3(kBlock), 0, s>>>(a, cin));
    HIP_OK(hipGetLastError());
    return 0;
}
int cin_ok(int cin) {
    if (cin < 4 || cin > kHeadWideMaxCin || cin % 4) return fail(-3, "wide head: channel count must be a multiple of 4 in 4..64");
    return 0;
}
}  // namespace

#define HEAD_WIDE_C(fn, ...)                            \
    switch (C) {                                        \
        case 2: return fn<2>(__VA_ARGS__);              \
        case 3: return fn<3>(__VA_ARGS__);              \
        case 4: return fn<4>(__VA_ARGS__);              \
        case 5: return fn<5>(__VA_ARGS__);              \
        case 6: return fn<6>(__VA_ARGS__);              \
        case 7: return fn<7>(__VA_ARGS__);              \
        case 8: return fn<8>(__VA_ARGS__);              \
        default: return fail(-3, "bad n_cls");          \
    }

int launch_head_fwd_wide(const HeadFwdArgs& a, int C, int cin, int B, hipStream_t s) {
    if (int rc = cin_ok(cin)) return rc;
    const dim3 grid(a.nblk, B);
    const double px = (double)B * a.HW;
    char nm[64]; snprintf(nm, sizeof nm, "head_fwd_wide_k<%d,%d,%s>", C, cin, AT_NAME(a.act_bf16));
    ProfScope ps(s, nm, "head", 2.0 * cin * C * px, px * (cin * 4 + (a.probs ? C * 4 : 0) + (a.argmax ? 1 : 0) + (a.labels ? 1 : 0)));
    HEAD_WIDE_C(fwd_c, a, cin, grid, s)
}

int launch_head_bwd_wide(const HeadBwdArgs& a, int C, int cin, int B, hipStream_t s) {
    if (int rc = cin_ok(cin)) return rc;
    if (a.fin.counter) return fail(-3, "wide head: the statistics are finalized by a launch of their own");
    const dim3 grid(a.nblk, B);
    const double px = (double)B * a.HW;
    char nm[64]; snprintf(nm, sizeof nm, "head_bwd_wide_k<%d,%d,%s>", C, cin, AT_NAME(a.act_bf16));
    ProfScope ps(s, nm, "head", 6.0 * cin * C * px, px * (cin * 4 * 2 + 1));
    HEAD_WIDE_C(bwd_c, a, cin, grid, s)
}

}  // namespace octh
