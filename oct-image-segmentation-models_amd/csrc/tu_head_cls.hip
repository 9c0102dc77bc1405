// One translation unit of liboct_unet_hip.so (see host.hpp): the two launchers of the class-streaming head kernels
// (kernels_head_cls.hpp), which oct_unet.hip routes every n_cls in 9..16 to.  The kernels themselves are instantiated in
// tu_head_cls_{fwd,bwd}_{9,13}.hip, four class counts each; this unit checks, names the launch for the profiler and picks
// the quarter.  Neither launcher allocates or waits.
#include <hip/hip_runtime.h>

#include <cstdio>

#include "host.hpp"
#include "kernels_fwd.hpp"

using namespace oct;

namespace octh {

namespace {
int shape_ok(int C, int cin) {
    if (C < 9 || C > 16) return fail(-3, "class-streaming head: n_cls must be in 9..16");
    if (cin < 4 || cin > 64 || cin % 4) return fail(-3, "class-streaming head: channel count must be a multiple of 4 in 4..64");
    return 0;
}
}  // namespace

int launch_head_fwd_cls(const HeadFwdArgs& a, int C, int cin, int B, hipStream_t s) {
    if (int rc = shape_ok(C, cin)) return rc;
    const dim3 grid(a.nblk, B);
    const double px = (double)B * a.HW;
    char nm[64]; snprintf(nm, sizeof nm, "head_fwd_cls_k<%d,%d,%s>", C, cin, AT_NAME(a.act_bf16));
    ProfScope ps(s, nm, "head", 2.0 * cin * C * px, px * (cin * 4 + (a.probs ? C * 4 : 0) + (a.argmax ? 1 : 0) + (a.labels ? 1 : 0)));
    return C < 13 ? head_cls_launch_0_9(a, C, cin, grid, s) : head_cls_launch_0_13(a, C, cin, grid, s);
}

int launch_head_bwd_cls(const HeadBwdArgs& a, int C, int cin, int B, hipStream_t s) {
    if (int rc = shape_ok(C, cin)) return rc;
    if (a.fin.counter) return fail(-3, "class-streaming head: the statistics are finalized by a launch of their own");
    const dim3 grid(a.nblk, B);
    const double px = (double)B * a.HW;
    char nm[64]; snprintf(nm, sizeof nm, "head_bwd_cls_k<%d,%d,%s>", C, cin, AT_NAME(a.act_bf16));
    ProfScope ps(s, nm, "head", 6.0 * cin * C * px, px * (cin * 4 * 2 + 1));
    return C < 13 ? head_cls_launch_1_9(a, C, cin, grid, s) : head_cls_launch_1_13(a, C, cin, grid, s);
}

}  // namespace octh
