// One translation unit of liboct_unet_hip.so (see host.hpp): the class-streaming head kernels head_fwd_cls_k<C, AT>, C = 13..16.
// (family, direction, first C, last C): a row of OCT_HEAD_UNITS in host.hpp
#define OCT_HEAD_FAMILY 2
#define OCT_HEAD_BWD 0
#define OCT_HEAD_C0 13
#define OCT_HEAD_C1 16
#include "launch_head.hpp"
