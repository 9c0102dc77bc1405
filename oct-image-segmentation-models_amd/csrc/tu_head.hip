// One translation unit of liboct_unet_hip.so (see host.hpp): the two launchers of the head, for all three kernel families
// (kernels_head.hpp, kernels_head_wide.hpp, kernels_head_cls.hpp).  The kernels themselves are instantiated in tu_head_<family>_<direction>_<first C>.hip (launch_head.hpp);
// this unit checks the shape, names the launch for the profiler and picks the unit.  Neither launcher allocates or waits.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <type_traits>

#include "host.hpp"

using namespace oct;

namespace octh {

namespace {
const char* const kFamily[3] = {"", "wide_", "cls_"};      // head_<fwd|bwd>_<family>k: the kernel names, as the profiler reports them

int shape_ok(HeadRoute r, int C, int cin) {
    if (r == HEAD_CLS ? (C < kHeadClsMin || C > kHeadClsMax) : (C < 2 || C >= kHeadClsMin)) return fail(-3, "head: bad n_cls for the kernel family");
    if (cin < 4 || cin % 4 || cin > (r == HEAD_REG ? 32 : 64)) return fail(-3, "head: unsupported start_neurons (a multiple of 4 in 4..64; register kernels: up to 32)");
    return 0;
}

// the unit of OCT_HEAD_UNITS that holds (family, direction, C)
template <typename Args>
int launch_unit(const Args& a, HeadRoute r, int C, int cin, dim3 grid, hipStream_t s) {
#define OCT_HEAD_UNIT_CALL(fam, dir, c0, c1)                                                                     \
    if constexpr (std::is_same<Args, OCT_HEAD_UNIT_ARGS_##dir>::value)                                           \
        if (r == fam && C >= c0 && C <= c1) return head_unit_##fam##_##dir##_##c0(a, C, cin, grid, s);
    OCT_HEAD_UNITS(OCT_HEAD_UNIT_CALL)
#undef OCT_HEAD_UNIT_CALL
    return fail(-3, "bad n_cls");
}
}  // namespace

int launch_head_fwd(const HeadFwdArgs& a, HeadRoute r, int C, int cin, int B, hipStream_t s) {
    if (int rc = shape_ok(r, C, cin)) return rc;
    const double px = (double)B * a.HW;
    char nm[64]; snprintf(nm, sizeof nm, "head_fwd_%sk<%d,%d,%s>", kFamily[r], C, cin, AT_NAME(a.act_bf16));
    ProfScope ps(s, nm, "head", 2.0 * cin * C * px, px * (cin * 4 + (a.probs ? C * 4 : 0) + (a.argmax ? 1 : 0) + (a.labels ? 1 : 0)));
    return launch_unit(a, r, C, cin, dim3(a.nblk, B), s);
}

int launch_head_bwd(const HeadBwdArgs& a, HeadRoute r, int C, int cin, int B, hipStream_t s) {
    if (int rc = shape_ok(r, C, cin)) return rc;
    if (a.fin.counter && r != HEAD_REG) return fail(-3, "streaming head: the statistics are finalized by a launch of their own");
    const double px = (double)B * a.HW;
    char nm[64]; snprintf(nm, sizeof nm, "head_bwd_%sk<%d,%d,%s>", kFamily[r], C, cin, AT_NAME(a.act_bf16));
    ProfScope ps(s, nm, "head", 6.0 * cin * C * px, px * (cin * 4 * 2 + 1));
    return launch_unit(a, r, C, cin, dim3(a.nblk, B), s);
}

}  // namespace octh
