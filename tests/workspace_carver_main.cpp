// Stand-alone check of csrc/workspace.hpp's carver (no HIP call): null-base behaviour, alignment, and typed take()
// against a layout computed by hand.  Built and run by tests/test_workspace_layout_cpu.py with the host sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../bnv_fusion_amd/csrc/workspace.hpp"

using bnv::Carver;
using bnv::align256;

static int failures = 0;
#define CHECK(cond)                                             \
  do {                                                          \
    if (!(cond)) {                                              \
      printf("FAILED line %d: %s\n", __LINE__, #cond);          \
      ++failures;                                               \
    }                                                           \
  } while (0)

struct Odd {   // 20 bytes: no power of two
  int32_t a[5];
};

int main() {
  // align256: the five spellings the layouts used are one number
  for (size_t b = 0; b <= 1025; ++b) {
    const size_t want = b == 0 ? 0 : ((b - 1) / 256 + 1) * 256;
    CHECK(align256(b) == want);
    CHECK(align256(b) == (b + 255) / 256 * 256);
    CHECK(align256(b) == ((b + 255) & ~(size_t)255));
  }
  static_assert(align256(0) == 0 && align256(1) == 256 && align256(256) == 256 && align256(257) == 512, "constexpr");

  // hand-computed layout: uint8[300] | double[33] | Odd[13] | int32[0] | uint64[32] | float[1]
  //   bytes            300 -> 512 | 264 -> 512  | 260 -> 512 | 0      | 256       | 4 -> 256
  const size_t want_off[6] = {0, 512, 1024, 1536, 1536, 1792};
  const size_t want_total = 2048;

  // null base: null pieces, the same byte count
  {
    Carver c(nullptr);
    CHECK(c.bytes() == 0);
    CHECK(c.take<uint8_t>(300) == nullptr);
    CHECK(c.take<double>(33) == nullptr);
    CHECK(c.take<Odd>(13) == nullptr);
    CHECK(c.take<int32_t>(0) == nullptr);
    CHECK(c.take<uint64_t>(32) == nullptr);
    CHECK(c.take<float>(1) == nullptr);
    CHECK(c.bytes() == want_total);
  }

  // real base: the pieces sit at the hand-computed offsets, are 256-byte aligned, and every byte of every piece can be
  // written without leaving the buffer (the sanitizer watches) or touching a neighbour
  {
    void* raw = nullptr;
    if (posix_memalign(&raw, 256, want_total) != 0) return 2;
    char* base = (char*)raw;
    for (size_t i = 0; i < want_total; ++i) base[i] = 0;
    Carver c(base);
    uint8_t* p0 = c.take<uint8_t>(300);
    double* p1 = c.take<double>(33);
    Odd* p2 = c.take<Odd>(13);
    int32_t* p3 = c.take<int32_t>(0);
    uint64_t* p4 = c.take<uint64_t>(32);
    float* p5 = c.take<float>(1);
    const void* got[6] = {p0, p1, p2, p3, p4, p5};
    for (int k = 0; k < 6; ++k) {
      CHECK((const char*)got[k] == base + want_off[k]);
      CHECK(((uintptr_t)got[k] & 255) == 0);
    }
    CHECK(c.bytes() == want_total);
    for (int i = 0; i < 300; ++i) p0[i] = 1;
    for (int i = 0; i < 33; ++i) p1[i] = 2.0;
    for (int i = 0; i < 13; ++i)
      for (int j = 0; j < 5; ++j) p2[i].a[j] = 3;
    for (int i = 0; i < 32; ++i) p4[i] = 4;
    p5[0] = 5.0f;
    CHECK(p0[299] == 1 && p1[0] == 2.0 && p1[32] == 2.0 && p2[0].a[0] == 3 && p2[12].a[4] == 3 && p4[31] == 4);
    CHECK(base[300] == 0 && base[512 + 264] == 0 && base[1024 + 260] == 0 && base[1792 + 4] == 0);   // the padding
    free(raw);
  }

  // an offset is derived by laying out at a small non-null base (lattice.hip: ws_offset)
  {
    Carver c((void*)256);
    c.take<int32_t>(65);
    float* t = c.take<float>(3);
    CHECK((size_t)((char*)t - (char*)256) == 512);
  }

  // sizes that are a whole number of pieces are not padded; size queries agree for a run of counts
  for (size_t n = 0; n < 200; ++n) {
    Carver a(nullptr);
    a.take<int32_t>(n);
    a.take<double>(3 * n);
    CHECK(a.bytes() == align256(4 * n) + align256(24 * n));
  }

  if (failures) return 1;
  printf("carver ok\n");
  return 0;
}
