// hj_optimize_bvh_device restated on the host, for tests/test_reinsert_host.py: the per-node steps of api/tree_reinsert.h called from
// plain loops in the order the kernels of api/tree_reinsert.hip run them - search, lock, check, win, apply, boxes, cost, the second
// attempt by the whole-path rule - with a tree check after every pass.  No device is touched.
//   reinsert_restatement IN OUT PASSES    IN, OUT: files of 32-byte skip-link records; prints one line per pass, then "result ..."
#include "../hijiki_amd/csrc/api/tree_reinsert.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace hj::reinsert;

struct Rec { float lo[3]; uint32_t shape; float hi[3]; uint32_t exit; };

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::fseek(f, 0, SEEK_END);
  const uint32_t N = (uint32_t)(std::ftell(f) / 32);
  std::fseek(f, 0, SEEK_SET);
  std::vector<Rec> rec(N);
  if (std::fread(rec.data(), 32, N, f) != N) return 2;
  std::fclose(f);
  const int passes = std::atoi(argv[3]);
  std::vector<uint32_t> parent(N, kNone), c0(N, kNone), c1(N, kNone), target(N), moving(N), win(N), pivot(N), arrived(N), size(N), info(kInfoWords);
  std::vector<float4> lo(N), hi(N);
  std::vector<float> gain(N);
  std::vector<unsigned long long> lock(N, 0);
  for (uint32_t i = 0; i < N; i++) {                                       // k_ri_init
    lo[i] = make_float4(rec[i].lo[0], rec[i].lo[1], rec[i].lo[2], __builtin_bit_cast(float, rec[i].shape));
    hi[i] = make_float4(rec[i].hi[0], rec[i].hi[1], rec[i].hi[2], 0.f);
    if (rec[i].shape != 0xFFFFFFFFu) continue;
    c0[i] = i + 1; c1[i] = rec[i + 1].exit;
    if (c1[i] >= N) return 3;
    parent[c0[i]] = i; parent[c1[i]] = i;
  }
  Tree t{N, parent.data(), c0.data(), c1.data(), lo.data(), hi.data(), target.data(), moving.data(), win.data(), pivot.data(), gain.data(),
         lock.data(), arrived.data(), size.data(), info.data()};
  std::vector<uint32_t> order;
  auto boxes = [&]() -> bool {                                             // k_ri_climb<false>, and: the links are a tree's
    order.clear();
    std::vector<uint32_t> st{0};
    while (!st.empty()) {
      const uint32_t i = st.back(); st.pop_back();
      order.push_back(i);
      if (order.size() > N) return false;
      if (c0[i] != kNone) { st.push_back(c1[i]); st.push_back(c0[i]); }
    }
    if (order.size() != N) return false;
    for (size_t k = N; k-- > 0;) {
      const uint32_t i = order[k];
      if (c0[i] == kNone) continue;
      if (parent[c0[i]] != i || parent[c1[i]] != i) return false;
      const Box b = ri_join(ri_box(t, c0[i]), ri_box(t, c1[i]));
      lo[i].x = b.lo[0]; lo[i].y = b.lo[1]; lo[i].z = b.lo[2]; hi[i].x = b.hi[0]; hi[i].y = b.hi[1]; hi[i].z = b.hi[2];
    }
    return true;
  };
  auto area_sum = [&]() {                                                  // k_ri_cost: 256 nodes a partial sum (LDS tree), added in index order
    double total = 0.0;
    for (uint32_t b = 0; b < N; b += 256) {
      double s[256];
      for (uint32_t k = 0; k < 256; k++) s[k] = (b + k < N && c0[b + k] != kNone) ? ri_area(ri_box(t, b + k)) : 0.0;
      for (uint32_t w = 128; w > 0; w >>= 1) for (uint32_t k = 0; k < w; k++) s[k] += s[k + w];
      total += s[0];
    }
    return total;
  };
  auto resolve = [&](auto rule, uint32_t& moved, uint32_t& holders) -> bool {
    constexpr bool WP = decltype(rule)::value;
    std::fill(lock.begin(), lock.end(), 0ull);
    for (uint32_t n = 0; n < N; n++) if (target[n] != kNone) {
      const unsigned long long key = ri_key(gain[n], n);
      if (!ri_walk_path<WP>(t, n, target[n], pivot[n], [&](uint32_t a) { lock[a] = std::max(lock[a], key); return true; })) return false;
    }
    holders = 0;
    for (uint32_t n = 0; n < N; n++) {
      const unsigned long long key = ri_key(gain[n], n);
      moving[n] = target[n] != kNone && ri_walk_path<WP>(t, n, target[n], pivot[n], [&](uint32_t a) { return lock[a] == key; });
      holders += moving[n];
    }
    for (uint32_t n = 0; n < N; n++) win[n] = moving[n] && (WP || ri_target_stays(t, moving.data(), n, target[n]));
    moved = 0;
    for (uint32_t n = 0; n < N; n++) if (win[n]) { ri_apply(t, n, target[n]); moved++; }
    return boxes();
  };
  if (!boxes()) return 3;
  double sum = area_sum();
  const double sum0 = sum;
  uint32_t moves = 0;
  int done = 0;
  for (int pass = 0; pass < passes; pass++, done++) {
    for (uint32_t n = 0; n < N; n++) {                                     // k_ri_search
      Found fd;
      if (!ri_search(t, n, fd)) return 4;
      target[n] = fd.x; pivot[n] = fd.pivot; gain[n] = (float)fd.gain;
    }
    const std::vector<uint32_t> sp = parent, s0 = c0, s1 = c1;
    uint32_t moved = 0, holders = 0;
    if (!resolve(std::false_type{}, moved, holders)) return 5;
    double now = area_sum();
    const bool again = moved != 0 ? !(now < sum) : holders != 0;
    if (again) {
      parent = sp; c0 = s0; c1 = s1;
      if (!resolve(std::true_type{}, moved, holders)) return 5;
      now = area_sum();
      if (moved != 0 && !(now < sum)) return 6;                            // the whole-path rule's gains are independent
    }
    std::printf("pass %d: %u moves%s, area sum %.17g\n", pass, moved, again ? " (whole-path rule)" : "", now);
    moves += moved;
    if (moved == 0) break;
    sum = now;
  }
  const double root = ri_area(ri_box(t, 0));
  std::printf("result passes %d moves %u cost_before %.17g cost_after %.17g\n", done, moves, sum0 / root, sum / root);
  // flatten: pre-order, left child first (k_ri_climb<true>, k_ri_flatten)
  std::vector<uint32_t> pos(N), sz(N, 1);
  for (uint32_t k = 0; k < N; k++) pos[order[k]] = k;
  for (size_t k = N; k-- > 0;) if (c0[order[k]] != kNone) sz[order[k]] = 1 + sz[c0[order[k]]] + sz[c1[order[k]]];
  const uint32_t root_exit = N > 1000000u ? N : 1000000u;
  std::vector<Rec> out(N);
  for (uint32_t i = 0; i < N; i++) {
    Rec& r = out[pos[i]];
    r.lo[0] = lo[i].x; r.lo[1] = lo[i].y; r.lo[2] = lo[i].z; r.hi[0] = hi[i].x; r.hi[1] = hi[i].y; r.hi[2] = hi[i].z;
    r.shape = __builtin_bit_cast(uint32_t, lo[i].w);
    r.exit = pos[i] + sz[i] < N ? pos[i] + sz[i] : root_exit;
  }
  f = std::fopen(argv[2], "wb");
  if (!f || std::fwrite(out.data(), 32, N, f) != N) return 2;
  std::fclose(f);
  return 0;
}
