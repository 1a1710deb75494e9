// What the path kernels of the queries share beside the text of their round loop (api/query_round_loop.h): k_pq_paths
// (api/path_query.hip) and k_gq_paths (api/gather_query.hip).  Included behind kernels/hj_stages.h.
#pragma once

namespace hj {

constexpr uint32_t kQueryTail = 128u;   // rays of a round at which the workgroup shrinks to one wave (the path kernel's HJ_TAIL1)
#define HJ_QUERY_WAVES 7                // the path kernel's register budget (HJ_PATH_WAVES): the called stages are compiled for it

// 64-sample groups of workgroup g: group k of its sequence is global group g + k * num_wg (the path kernel's round-robin deal)
HJ_DEV uint32_t query_num_groups(uint32_t num_samples, uint32_t num_wg, uint32_t g) {
  const uint32_t groups = (num_samples + 63u) / 64u;
  return groups > g ? (groups - g + num_wg - 1u) / num_wg : 0u;
}

}  // namespace hj
