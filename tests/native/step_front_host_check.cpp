// Stand-alone check of the front table's HOST side (tacorl_amd/csrc/step_front_table.h): validation and assembly over the
// eligible case and the refused ones.  No GPU, no HIP: built with the host sanitizers and run on the CPU, e.g.
//   hipcc -Xarch_host -fsanitize=address,undefined -std=c++17 tests/native/step_front_host_check.cpp -o step_front_host_check
// (tests/test_step_front_cpu.py does that).  Addresses are made up and never dereferenced.  Exit status 0: all checks held.
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../tacorl_amd/csrc/step_front_table.h"

static int failures = 0;
#define CHECK(x)                                              \
  do {                                                        \
    if (!(x)) {                                               \
      printf("FAILED line %d: %s\n", __LINE__, #x);           \
      failures++;                                             \
    }                                                         \
  } while (0)

struct Case {
  const float* src_base[2 * TACORL_SF_MAXCAM + 1];
  long src_pitch[2 * TACORL_SF_MAXCAM + 1];
  const float* pack_src[TACORL_SF_MAXJOBS + 1];
  long pack_pitch[TACORL_SF_MAXJOBS + 1];
  void* pack_dst[TACORL_SF_MAXJOBS + 1];
  int pack_n[TACORL_SF_MAXJOBS + 1];
  int nsrc, njobs, disp_dtype, B, H, W;
  const void* disp;
  float *reward, *done, *acts_dst;
  const float* acts_src;
  long n_acts;
};
static const float* fp(uintptr_t a) { return reinterpret_cast<const float*>(a); }
static float* fpw(uintptr_t a) { return reinterpret_cast<float*>(a); }

// TACORL's step at B = 3, T = 2, 84 x 84, one camera: window / next sources, [obs; goal] pack jobs, an action window
static Case eligible() {
  Case c{};
  const long img = 3 * 84 * 84, T = 2;
  const uintptr_t states = 0x10000000, goal = 0x20000000, x3 = 0x30000000;
  c.H = c.W = 84; c.B = 3; c.nsrc = 2; c.njobs = 2;
  c.src_base[0] = fp(states); c.src_pitch[0] = img;
  c.src_base[1] = fp(states + 4 * (T - 1) * img); c.src_pitch[1] = T * img;
  c.pack_src[0] = fp(states); c.pack_pitch[0] = T * img; c.pack_dst[0] = reinterpret_cast<void*>(x3); c.pack_n[0] = c.B;
  c.pack_src[1] = fp(goal); c.pack_pitch[1] = img; c.pack_dst[1] = reinterpret_cast<void*>(x3 + 2 * c.B * img); c.pack_n[1] = c.B;
  c.disp = reinterpret_cast<const void*>(0x40000000); c.disp_dtype = 1;
  c.reward = fpw(0x40001000); c.done = fpw(0x40002000);
  c.acts_src = fp(0x40003000); c.acts_dst = fpw(0x40004000); c.n_acts = c.B * T * 7;
  return c;
}
static bool ok(const Case& c) {
  return sf_supported(c.nsrc, c.src_base, c.src_pitch, c.njobs, c.pack_src, c.pack_pitch, c.pack_dst, c.pack_n, c.disp, c.disp_dtype,
                      c.reward, c.B, c.acts_src, c.acts_dst, c.n_acts, c.H, c.W);
}
static void assemble(const Case& c, SFTable* t) {
  sf_assemble(t, c.nsrc, c.src_base, c.src_pitch, c.njobs, c.pack_src, c.pack_pitch, c.pack_dst, c.pack_n, c.disp, c.disp_dtype, c.reward,
              c.done, c.B, c.acts_src, c.acts_dst, c.n_acts, c.H, c.W);
}

int main() {
  // the layout the python side and the kernel rely on
  CHECK(sizeof(SFSrc) == 32 && sizeof(SFTable) == 544);
  CHECK(offsetof(SFTable, src) == 0 && offsetof(SFTable, pack_src) == 256 && offsetof(SFTable, pack_dst) == 320);
  CHECK(offsetof(SFTable, pack_pitch) == 384 && offsetof(SFTable, pack_n) == 448 && offsetof(SFTable, disp) == 480);
  CHECK(offsetof(SFTable, n_acts) == 520 && offsetof(SFTable, disp_dtype) == 528 && offsetof(SFTable, HW) == 540);

  const Case good = eligible();
  CHECK(ok(good));
  for (int dt = 0; dt <= 3; dt++) { Case c = good; c.disp_dtype = dt; CHECK(ok(c)); }
  { Case c = good; c.n_acts = 0; c.acts_src = nullptr; c.acts_dst = nullptr; CHECK(ok(c)); }                  // no action window
  { Case c = good; c.done = nullptr; CHECK(ok(c)); }                                                            // done is optional
  { Case c = good; c.src_base[0] = fp(0x10000004); CHECK(!ok(c)); }                                             // misaligned source
  { Case c = good; c.pack_src[1] = fp(0x20000004); CHECK(!ok(c)); }                                             // misaligned pack source
  { Case c = good; c.pack_dst[0] = reinterpret_cast<void*>(0x30000008); CHECK(!ok(c)); }                       // misaligned destination
  { Case c = good; c.src_pitch[1] += 2; CHECK(!ok(c)); }                                                        // pitch % 4
  { Case c = good; c.pack_pitch[0] += 2; CHECK(!ok(c)); }
  { Case c = good; c.pack_pitch[0] = -4; CHECK(!ok(c)); }
  { Case c = good; c.disp_dtype = 4; CHECK(!ok(c)); }                                                           // bad dtype codes
  { Case c = good; c.disp_dtype = -1; CHECK(!ok(c)); }
  { Case c = good; c.B = 0; CHECK(!ok(c)); }                                                                    // counts
  { Case c = good; c.pack_n[1] = 0; CHECK(!ok(c)); }
  { Case c = good; c.njobs = TACORL_SF_MAXJOBS + 1; CHECK(!ok(c)); }
  { Case c = good; c.nsrc = 2 * TACORL_SF_MAXCAM + 1; CHECK(!ok(c)); }
  { Case c = good; c.nsrc = -1; CHECK(!ok(c)); }
  { Case c = good; c.n_acts = -1; CHECK(!ok(c)); }
  { Case c = good; c.acts_dst = nullptr; CHECK(!ok(c)); }                                                       // half an action window
  { Case c = good; c.disp = nullptr; CHECK(!ok(c)); }
  { Case c = good; c.reward = nullptr; CHECK(!ok(c)); }
  { Case c = good; c.H = 85; c.W = 85; CHECK(!ok(c)); }                                                         // H*W % 4
  {                                                                                                             // every slot in use
    Case c = good;
    c.nsrc = 2 * TACORL_SF_MAXCAM; c.njobs = TACORL_SF_MAXJOBS;
    for (int i = 0; i < c.nsrc; i++) { c.src_base[i] = fp(0x10000000 + 0x100000 * i); c.src_pitch[i] = 3 * 84 * 84; }
    for (int j = 0; j < c.njobs; j++) {
      c.pack_src[j] = fp(0x20000000 + 0x100000 * j); c.pack_dst[j] = reinterpret_cast<void*>(0x30000000 + 0x100000 * j);
      c.pack_pitch[j] = 3 * 84 * 84; c.pack_n[j] = 1 + j;
    }
    CHECK(ok(c));
    SFTable* t = static_cast<SFTable*>(malloc(sizeof(SFTable)));  // (heap: an overrun is the sanitizer's to see)
    assemble(c, t);
    CHECK(t->src[2 * TACORL_SF_MAXCAM - 1].base == c.src_base[c.nsrc - 1] && t->pack_n[TACORL_SF_MAXJOBS - 1] == TACORL_SF_MAXJOBS);
    CHECK(sf_table_sane(*t));
    free(t);
  }

  // assembly: the fields, zero everywhere else, equal entries -> equal bytes whatever the buffer held before
  SFTable* a = static_cast<SFTable*>(malloc(sizeof(SFTable)));
  SFTable* b = static_cast<SFTable*>(malloc(sizeof(SFTable)));
  memset(a, 0xAB, sizeof(SFTable));
  memset(b, 0x11, sizeof(SFTable));
  assemble(good, a);
  assemble(good, b);
  CHECK(memcmp(a, b, sizeof(SFTable)) == 0 && sf_table_sane(*a));
  CHECK(a->src[0].base == good.src_base[0] && a->src[0].img_pitch == 3 * 84 * 84 && a->src[0].plane_pitch == 84 * 84 && a->src[0].row_pitch == 84);
  CHECK(a->src[1].base == good.src_base[1] && a->src[1].img_pitch == 2 * 3 * 84 * 84);
  CHECK(a->src[2].base == nullptr && a->pack_src[2] == nullptr && a->pack_n[2] == 0);
  CHECK(a->pack_src[1] == good.pack_src[1] && a->pack_dst[1] == good.pack_dst[1] && a->pack_pitch[0] == 2 * 3 * 84 * 84 && a->pack_n[1] == 3);
  CHECK(a->disp == good.disp && a->disp_dtype == 1 && a->reward == good.reward && a->done == good.done && a->B == 3);
  CHECK(a->acts_src == good.acts_src && a->acts_dst == good.acts_dst && a->n_acts == 42 && a->njobs == 2 && a->HW == 84 * 84);
  { Case c = good; c.src_base[0] = fp(0x10000010); assemble(c, b); CHECK(memcmp(a, b, sizeof(SFTable)) != 0); }  // an address moved
  { Case c = good; c.n_acts = 0; assemble(c, b); CHECK(b->acts_src == nullptr && b->acts_dst == nullptr && b->n_acts == 0); }
  { SFTable z; memset(&z, 0, sizeof z); CHECK(!sf_table_sane(z)); }  // a table never assembled is not filled
  free(a);
  free(b);
  if (failures) {
    printf("step_front_host_check: %d FAILED\n", failures);
    return 1;
  }
  printf("step_front_host_check: ok\n");
  return 0;
}
