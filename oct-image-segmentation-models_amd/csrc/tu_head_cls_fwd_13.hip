// One translation unit of liboct_unet_hip.so (see host.hpp): the class-streaming head kernels head_fwd_cls_k<C, AT>, C = 13..16.
#define OCT_HEAD_CLS_BWD 0
#define OCT_HEAD_CLS_C0 13
#include "launch_head_cls.hpp"
