// Runs the bf16 x 3 plane builder of csrc/weight_pack.h (split_bf16x3, bf16x3_planes) on planted and random weights and checks, on the
// CPU: hi + mid + lo == w in double, every part is a bf16 (the fp32 it stands for has zero low 16 bits by construction: the planes hold
// its upper 16), the stage images read back through the kernel's DMA / fragment geometry restated here, and zero padding past cin.
// Built by tests/test_proj_bf16x3_cpu.py with the ROCm host compiler under AddressSanitizer + UndefinedBehaviorSanitizer.
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../chiron_amd/csrc/weight_pack.h"

using namespace chiron;

static int failures = 0;
#define CHECK(cond, ...)            \
  do {                              \
    if (!(cond)) {                  \
      if (++failures <= 20) {       \
        printf("FAIL %s: ", #cond); \
        printf(__VA_ARGS__);        \
        printf("\n");               \
      }                             \
    }                               \
  } while (0)

// exponent of the lowest set significand bit of a non-zero finite float
static int lowest_bit_exponent(float w) {
  const uint32_t u = f32_bits(w), e = (u >> 23) & 0xffu;
  const uint32_t m = (u & 0x7fffffu) | (e ? 0x800000u : 0u);
  return (int)(e ? e : 1) - 127 - 23 + __builtin_ctz(m);
}

static double part(uint16_t h) { return (double)bits_f32((uint32_t)h << 16); }

// What gemm_proj_bf16x3_kernel reads, said independently of bf16x3_index: the image of (tile, stage c) is 15 DMA pieces of 1 KB copied
// as they lie; a lane (li, kh) of the wave that owns column block ni reads, for plane pl, the 16 bytes at 16 * ((2 pl + kh) * 160 + 32 ni + li):
// element e of them multiplies the activation of channel 16 c + 8 (e >> 2) + 4 kh + (e & 3).
static uint16_t kernel_view(const std::vector<uint16_t>& planes, int stages, int pl, int n, int k) {
  const int tile = n / 160, ni = (n % 160) / 32, li = n % 32, c = k / 16;
  for (int kh = 0; kh < 2; ++kh)
    for (int e = 0; e < 8; ++e)
      if (16 * c + 8 * (e >> 2) + 4 * kh + (e & 3) == k) {
        const size_t byte = (size_t)(tile * stages + c) * 15360 + 16 * (size_t)((2 * pl + kh) * 160 + 32 * ni + li) + 2 * (size_t)e;
        return planes.at(byte / 2);
      }
  abort();
}

static void run(int N, int ld, int cin, unsigned seed) {
  std::vector<float> Wt((size_t)N * ld, 0.f);
  std::mt19937 rng(seed);
  std::normal_distribution<float> nd(0.f, 0.1f);
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < ld; ++k) Wt[(size_t)n * ld + k] = k < cin ? nd(rng) : 123.0f;   // the builder must not look past cin
  const float all24 = bits_f32(0x3fffffffu);   // 1.99999988: all 24 significand bits set
  const float plant[] = {0.0f, -0.0f, 1e-6f, 7e4f, 1e30f, 1e-30f, FLT_MAX, -FLT_MAX, FLT_MIN, -FLT_MIN, all24, -all24, bits_f32(0x00000001u),
                         bits_f32(0x007fffffu), bits_f32(0x00ffffffu)};
  const int nplant = (int)(sizeof(plant) / sizeof(plant[0]));
  for (int i = 0; i < nplant; ++i) {
    Wt[(size_t)(i * 53 % N) * ld + (i * 17) % cin] = plant[i];
    Wt[(size_t)(N - 1 - i) * ld + (cin - 1 - i)] = plant[i];
  }
  const std::vector<uint16_t> planes = bf16x3_planes(Wt.data(), N, ld, cin);
  const int stages = bf16x3_stages(cin);
  CHECK(planes.size() == (size_t)(N / 160) * stages * 7680, "size %zu", planes.size());
  size_t nonzero_seen = 0;
  for (int n = 0; n < N; ++n)
    for (int k = 0; k < stages * 16; ++k) {
      const uint16_t h = kernel_view(planes, stages, 0, n, k), m = kernel_view(planes, stages, 1, n, k), l = kernel_view(planes, stages, 2, n, k);
      if (k >= cin) {
        CHECK(h == 0 && m == 0 && l == 0, "padding n %d k %d: %04x %04x %04x", n, k, h, m, l);
        continue;
      }
      const float w = Wt[(size_t)n * ld + k];
      const double sum = part(h) + part(m) + part(l);
      // exact for every weight whose lowest set bit is worth 2^-133 or more; below that the third part has no bit to stand on
      if (w == 0.f || lowest_bit_exponent(w) >= -133)
        CHECK(sum == (double)w, "n %d k %d: w %a parts %a %a %a", n, k, w, part(h), part(m), part(l));
      else
        CHECK(fabs(sum - (double)w) <= ldexp(1.0, -133), "n %d k %d: w %a parts %a %a %a", n, k, w, part(h), part(m), part(l));
      CHECK(std::isfinite(part(h)) && std::isfinite(part(m)) && std::isfinite(part(l)), "n %d k %d: w %a has a non-finite part", n, k, w);
      CHECK(fabs(part(m)) <= fabs(part(h)) * ldexp(1.0, -7) || part(h) == 0, "n %d k %d: mid %a against hi %a", n, k, part(m), part(h));
      nonzero_seen += (h | m | l) != 0;
      const Bf16x3 s = split_bf16x3(w);
      CHECK(s.hi == h && s.mid == m && s.lo == l, "n %d k %d: the image does not hold split_bf16x3(w)", n, k);
    }
  CHECK(nonzero_seen > (size_t)N * cin * 9 / 10, "only %zu non-zero weights seen", nonzero_seen);
  // every element of the image is reached by exactly one (plane, n, k): no two weights share a place
  std::vector<unsigned char> hit(planes.size(), 0);
  for (int pl = 0; pl < 3; ++pl)
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < stages * 16; ++k) {
        const size_t at = bf16x3_index(pl, n, k, stages);
        CHECK(at < hit.size() && !hit[at], "index (%d, %d, %d) = %zu taken twice or out of range", pl, n, k, at);
        if (at < hit.size()) hit[at] = 1;
      }
  for (size_t i = 0; i < hit.size(); ++i) CHECK(hit[i], "element %zu of the image belongs to no weight", i);
}

int main() {
  run(800, 256, 256, 1);   // layer 0: K = 256, sixteen stages
  run(800, 224, 200, 2);   // K = 200 in rows of 224: thirteen stages, the last holds 8 channels
  run(160, 224, 200, 3);
  if (failures) {
    printf("%d checks failed\n", failures);
    return 1;
  }
  printf("bf16x3 planes OK\n");
  return 0;
}
