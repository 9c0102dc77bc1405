// One translation unit of liboct_unet_hip.so (see host.hpp): the class-streaming head kernels head_bwd_cls_k<C, AT>, C = 9..12.
#define OCT_HEAD_CLS_BWD 1
#define OCT_HEAD_CLS_C0 9
#include "launch_head_cls.hpp"
