// csrc/weight_pack.h on the CPU (tests/pwl_ref.py builds this, plain: the packer runs under ASan + UBSan in tests/test_weight_pack_cpu.py):
// packs one blob and writes block 1's piecewise-linear table as the kernel of pwl.hip receives it.
//   pwl_table_dump <desc: raw chiron_model_desc> <blob: float32> <segment_len> <dtype> <switches: one of "wWFpRS" each, or -> <out>
// out: int32 {pwl_nbp, k, c, stride, left, floats of pwl_bp, of pwl_ref, of pwl_tab, of pwl_shift}, then the four buffers as float32.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>

#include "../../chiron_amd/csrc/weight_pack.h"

namespace chiron {
chiron_status set_error(chiron_status st, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  fprintf(stderr, "refused %d ", (int)st);
  vfprintf(stderr, fmt, ap);
  fprintf(stderr, "\n");
  va_end(ap);
  return st;
}
}  // namespace chiron
using namespace chiron;

template <class Tp>
static std::vector<Tp> read_file(const char* path) {
  std::vector<Tp> v;
  FILE* f = fopen(path, "rb");
  if (!f) return v;
  fseek(f, 0, SEEK_END);
  v.resize((size_t)ftell(f) / sizeof(Tp));
  fseek(f, 0, SEEK_SET);
  if (fread(v.data(), sizeof(Tp), v.size(), f) != v.size()) v.clear();
  fclose(f);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 7) return 2;
  const std::vector<chiron_model_desc> desc = read_file<chiron_model_desc>(argv[1]);
  const std::vector<float> blob = read_file<float>(argv[2]);
  auto on = [&](char c) { return strchr(argv[5], c) != nullptr; };
  PackSwitches sw;
  sw.no_winograd = on('w'), sw.wino_f2 = on('W'), sw.wino_f4 = on('F'), sw.no_pwl = on('p'), sw.split_rec32 = on('R'), sw.split_row_scale = !on('S');
  BlobMap map;
  if (desc.size() != 1 || blob_map(&desc[0], &map) || map.total != blob.size()) return 3;
  NetPlans plans;
  std::vector<Upload> ups;
  if (pack_weights(desc[0], map, blob.data(), atoi(argv[3]), atoi(argv[4]), sw, &plans, &ups)) return 4;
  if (plans.blocks.empty()) return 5;
  // the packer left the plan pointers null and recorded their addresses: find block 1's four uploads by address
  std::map<void**, const Upload*> by_dst;
  for (const Upload& u : ups) by_dst[u.dst] = &u;
  BlockPlan& b = plans.blocks[0];
  void** const want[4] = {reinterpret_cast<void**>(&b.pwl_bp), reinterpret_cast<void**>(&b.pwl_ref), reinterpret_cast<void**>(&b.pwl_tab),
                          reinterpret_cast<void**>(&b.pwl_shift)};
  const Upload* got[4];
  for (int i = 0; i < 4; ++i) {
    auto it = by_dst.find(want[i]);
    if (it == by_dst.end()) return 6;   // no table: not the lifted block, batch BN, or the switch p
    got[i] = it->second;
  }
  FILE* f = fopen(argv[6], "wb");
  if (!f) return 7;
  const int32_t head[9] = {b.pwl_nbp, b.k, b.c, b.stride, b.left, (int32_t)(got[0]->bytes / 4), (int32_t)(got[1]->bytes / 4),
                           (int32_t)(got[2]->bytes / 4), (int32_t)(got[3]->bytes / 4)};
  bool ok = fwrite(head, sizeof(head), 1, f) == 1;
  for (int i = 0; i < 4; ++i) ok = ok && (got[i]->bytes == 0 || fwrite(got[i]->data, got[i]->bytes, 1, f) == 1);
  ok = fclose(f) == 0 && ok;
  return ok ? 0 : 8;
}
