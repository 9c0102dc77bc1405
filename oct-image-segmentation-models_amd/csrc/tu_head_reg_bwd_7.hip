// One translation unit of liboct_unet_hip.so (see host.hpp): the register head kernels head_bwd_k<C, CIN, AT>, C = 7.
// (family, direction, first C, last C): a row of OCT_HEAD_UNITS in host.hpp
#define OCT_HEAD_FAMILY 0
#define OCT_HEAD_BWD 1
#define OCT_HEAD_C0 7
#define OCT_HEAD_C1 7
#include "launch_head.hpp"
