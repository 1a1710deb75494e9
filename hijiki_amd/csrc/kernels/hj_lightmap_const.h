// What the light-map kernels (hj_lightmap.h) and the light-map filter's (hj_lightmap_filter.h) have in common.
#pragma once
#include "../../../include/hijiki_hip.h"
#include "hj_num.h"

namespace hj {

constexpr uint32_t kLmThreads = 256u;          // threads of a k_lm_* workgroup = texels of a scan tile (4 waves)
constexpr uint32_t kLmNone = 0xFFFFFFFFu;      // owner word of a texel nobody owns

}  // namespace hj
