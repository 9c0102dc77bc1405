// One translation unit of liboct_unet_hip.so (see host.hpp): the register head kernels head_fwd_k<C, CIN, AT>, C = 2..5.
// (family, direction, first C, last C): a row of OCT_HEAD_UNITS in host.hpp
#define OCT_HEAD_FAMILY 0
#define OCT_HEAD_BWD 0
#define OCT_HEAD_C0 2
#define OCT_HEAD_C1 5
#include "launch_head.hpp"
