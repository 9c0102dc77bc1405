// One translation unit of liboct_unet_hip.so (see host.hpp): the channel-streaming head kernels head_fwd_wide_k<C, AT>, C = 2..8.
// (family, direction, first C, last C): a row of OCT_HEAD_UNITS in host.hpp
#define OCT_HEAD_FAMILY 1
#define OCT_HEAD_BWD 0
#define OCT_HEAD_C0 2
#define OCT_HEAD_C1 8
#include "launch_head.hpp"
