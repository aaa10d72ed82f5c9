// csrc/weight_pack.h on the CPU (tests/test_weight_pack_cpu.py builds this under ASan + UBSan): packs one blob and prints the scalar
// geometry and, per device buffer, "<plan pointer> <byte length> <FNV-1a-64 of the bytes>"; for the shift of an f16 GEMM the same for
// the dW and shift0 that calibration keeps.
//   weight_pack_digest <desc: raw chiron_model_desc> <blob: float32> <segment_len> <dtype> <switches: one of "wWFpRS" each, or ->
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "../../chiron_amd/csrc/weight_pack.h"

namespace chiron {
chiron_status set_error(chiron_status st, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  printf("refused %d ", (int)st);
  vprintf(fmt, ap);
  printf("\n");
  va_end(ap);
  return st;
}
}  // namespace chiron
using namespace chiron;

struct Digest {
  size_t bytes;
  unsigned long long fnv;
};
static Digest digest(const void* p, size_t n) {
  unsigned long long h = 1469598103934665603ull;
  for (size_t i = 0; i < n; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  return {n, h};
}

// every device pointer of the plans, by name
template <class Plans, class F>
static void each_plan_pointer(const Plans& e, F f) {
  auto gemm = [&](const std::string& n, const ConvGemmPlan& g) { f(n + ".Wt", g.Wt), f(n + ".shift", g.shift), f(n + ".descale", g.descale); };
  f("stem_w", e.stem_w), f("stem_shift", e.stem_shift), f("stem_scale", e.stem_scale), f("stem_offset", e.stem_offset);
  for (size_t i = 0; i < e.blocks.size(); ++i) {
    const BlockPlan& b = e.blocks[i];
    const std::string n = "block" + std::to_string(i) + ".";
    f(n + "lift_a", b.lift_a), f(n + "lift_b", b.lift_b), f(n + "res_a", b.res_a), f(n + "res_b", b.res_b);
    f(n + "pwl_bp", b.pwl_bp), f(n + "pwl_ref", b.pwl_ref), f(n + "pwl_tab", b.pwl_tab), f(n + "pwl_shift", b.pwl_shift), f(n + "wino_u", b.wino_u);
    gemm(n + "ga", b.ga), gemm(n + "gb", b.gb), gemm(n + "gc", b.gc), gemm(n + "g1", b.g1);
    for (int j = 0; j < 4; ++j) f(n + "bn_scale" + std::to_string(j), b.bn_scale[j]), f(n + "bn_offset" + std::to_string(j), b.bn_offset[j]);
  }
  for (size_t i = 0; i < e.lstm.size(); ++i) {
    const LstmPlan& l = e.lstm[i];
    const std::string n = "lstm" + std::to_string(i) + ".";
    gemm(n + "proj0", l.proj[0]), gemm(n + "proj1", l.proj[1]);
    f(n + "wfrag", l.wfrag), f(n + "wwide", l.wwide), f(n + "whfused", l.whfused), f(n + "wxwide", l.wxwide), f(n + "wsplit", l.wsplit);
    f(n + "wwide32", l.wwide32), f(n + "wlight", l.wlight);
  }
  f("fc_w", e.fc_w), f("fc_b", e.fc_b), f("fc_wc", e.fc_wc), f("fc_bc", e.fc_bc);
}

template <class Plans>
static void print_geometry(const Plans& e) {
  printf("geometry T %d C %d stem k %d stride %d left %d t %d c %d\n", e.T, e.C, e.stem_k, e.stem_stride, e.stem_left, e.stem_t, e.stem_c);
  auto gemm = [](const ConvGemmPlan& g) { printf(" [%d %d %d]", g.N, g.Npad, g.K); };
  for (const BlockPlan& b : e.blocks) {
    printf("geometry block lift %d c_in %d c %d k %d stride %d left %d t_in %d t_out %d pwl_nbp %d wino_f4 %d i_bn %d gemms", (int)b.lift, b.c_in, b.c,
           b.k, b.stride, b.left, b.t_in, b.t_out, b.pwl_nbp, b.wino_f4, (int)b.i_bn);
    gemm(b.ga), gemm(b.gb), gemm(b.gc), gemm(b.g1);
    printf("\n");
  }
  for (const LstmPlan& l : e.lstm) {
    printf("geometry lstm in_w %d nproj %d wx_ksteps %d gemms", l.in_w, l.nproj, l.wx_ksteps);
    gemm(l.proj[0]), gemm(l.proj[1]);
    printf("\n");
  }
}

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
  if (argc != 6) return 2;
  const std::vector<chiron_model_desc> desc = read_file<chiron_model_desc>(argv[1]);
  const std::vector<float> blob = read_file<float>(argv[2]);
  auto on = [&](char c) { return strchr(argv[5], c) != nullptr; };
  PackSwitches sw;
  sw.no_winograd = on('w'), sw.wino_f2 = on('W'), sw.wino_f4 = on('F'), sw.no_pwl = on('p'), sw.split_rec32 = on('R'), sw.split_row_scale = !on('S');
  BlobMap map;
  if (desc.size() != 1 || blob_map(&desc[0], &map) || map.total != blob.size()) return 3;
  NetPlans plans;
  std::vector<Upload> ups;
  if (pack_weights(desc[0], map, blob.data(), atoi(argv[3]), atoi(argv[4]), sw, &plans, &ups)) return 0;   // the refusal is the output
  // what the engine's uploader does, with host memory: the pointers are stored through the addresses the packer recorded
  std::map<const void*, const Upload*> by_ptr;
  std::vector<std::vector<unsigned char>> mem(ups.size());
  for (size_t i = 0; i < ups.size(); ++i) {
    const unsigned char* b = (const unsigned char*)ups[i].data;
    mem[i].assign(b, b + ups[i].bytes);
    mem[i].push_back(0);   // an address of its own for an empty buffer too
    *ups[i].dst = mem[i].data();
    by_ptr[mem[i].data()] = &ups[i];
  }
  print_geometry(plans);
  size_t named = 0;
  each_plan_pointer(plans, [&](const std::string& name, const void* p) {
    if (!p) return;
    const Upload* u = by_ptr.at(p);
    ++named;
    const Digest d = digest(u->data, u->bytes);
    printf("%s %zu %016llx\n", name.c_str(), d.bytes, d.fnv);
    if (u->host.Npad > 0) {
      const Digest dw = digest(u->host.dW.data(), u->host.dW.size() * 4), s0 = digest(u->host.shift0.data(), u->host.shift0.size() * 4);
      printf("%s.host [%d %d %d] dW %zu %016llx shift0 %zu %016llx\n", name.c_str(), u->host.N, u->host.Npad, u->host.K, dw.bytes, dw.fnv, s0.bytes, s0.fnv);
    }
  });
  printf("uploads %zu named %zu\n", ups.size(), named);
  return 0;
}
