// The device-resident front table of TACORL's fp32-source step (rl_ops.hip: step_front_kernel) and its HOST side: what the
// table takes (sf_supported) and its bytes for a step's entries (sf_assemble).  Plain C++ with no HIP in it, so that the
// host side also builds into a stand-alone program (tests/native/step_front_host_check.cpp, run under the host sanitizers).
#pragma once
#include <stdint.h>
#include <string.h>

#include "../../include/tacorl_hip.h"

// A source entry as the fused encoder reads it (encoder_fused.h EFSrc; rl_ops.hip asserts the two layouts equal): n fp32 CHW
// images, image i at base + i * img_pitch floats, planes plane_pitch and rows row_pitch apart.
struct SFSrc {
  const float* base;
  long img_pitch, plane_pitch, row_pitch;
};
struct SFTable {
  SFSrc src[2 * TACORL_SF_MAXCAM];           // camera i: entry 2 i = the window's frames, 2 i + 1 = the next observations
  const float* pack_src[TACORL_SF_MAXJOBS];  // pack job j: pack_n[j] fp32 CHW images, image i at pack_src + i * pack_pitch
  void* pack_dst[TACORL_SF_MAXJOBS];         //   -> bf16 NHWC at pack_dst (a slot of the engine's image buffer)
  long pack_pitch[TACORL_SF_MAXJOBS];
  int pack_n[TACORL_SF_MAXJOBS];
  const void* disp;                          // transition: reward = done = float(disp == 1), acts_dst = acts_src
  float* reward;
  float* done;
  const float* acts_src;
  float* acts_dst;
  long n_acts;
  int disp_dtype, B;
  int njobs, HW;
};

// Sources: 16-byte aligned, contiguous images, image pitch a non-negative multiple of four floats (the geometry itself is
// the encoder's to accept: tacorl_step_front_supported asks tacorl_encoder_src_supported as well).  Pack jobs as
// tacorl_pack_images_batch: both ends 16-byte aligned, pitch % 4 == 0, H*W % 4 == 0, n >= 1.  A known disp dtype code,
// B >= 1, an action window with both ends or none.
inline bool sf_supported(int nsrc, const float* const* src_base, const long* src_pitch, int njobs, const float* const* pack_src,
                         const long* pack_pitch, void* const* pack_dst, const int* pack_n, const void* disp, int disp_dtype,
                         const float* reward, int B, const float* acts_src, const float* acts_dst, long n_acts, int H, int W) {
  if (nsrc < 0 || nsrc > 2 * TACORL_SF_MAXCAM || njobs < 0 || njobs > TACORL_SF_MAXJOBS || H < 1 || W < 1 || ((long)H * W) % 4)
    return false;
  if ((nsrc > 0 && (!src_base || !src_pitch)) || (njobs > 0 && (!pack_src || !pack_pitch || !pack_dst || !pack_n))) return false;
  for (int i = 0; i < nsrc; i++)
    if (!src_base[i] || ((uintptr_t)src_base[i] & 15) || src_pitch[i] % 4 || src_pitch[i] < 0) return false;
  for (int j = 0; j < njobs; j++)
    if (!pack_src[j] || !pack_dst[j] || ((uintptr_t)pack_src[j] & 15) || ((uintptr_t)pack_dst[j] & 15) || pack_pitch[j] % 4 ||
        pack_pitch[j] < 0 || pack_n[j] < 1)
      return false;
  if (!disp || !reward || B < 1 || disp_dtype < 0 || disp_dtype > 3) return false;
  return n_acts == 0 || (n_acts > 0 && acts_src && acts_dst);
}

// The table's bytes for entries sf_supported accepted: every unused entry and all padding zero, so equal entries give equal
// bytes - what the caller's skip of the fill compares.
inline void sf_assemble(SFTable* t, int nsrc, const float* const* src_base, const long* src_pitch, int njobs,
                        const float* const* pack_src, const long* pack_pitch, void* const* pack_dst, const int* pack_n,
                        const void* disp, int disp_dtype, float* reward, float* done, int B, const float* acts_src,
                        float* acts_dst, long n_acts, int H, int W) {
  memset(t, 0, sizeof(SFTable));
  for (int i = 0; i < nsrc; i++) {
    t->src[i].base = src_base[i]; t->src[i].img_pitch = src_pitch[i];
    t->src[i].plane_pitch = (long)H * W; t->src[i].row_pitch = W;
  }
  for (int j = 0; j < njobs; j++) {
    t->pack_src[j] = pack_src[j]; t->pack_dst[j] = pack_dst[j]; t->pack_pitch[j] = pack_pitch[j]; t->pack_n[j] = pack_n[j];
  }
  t->disp = disp; t->reward = reward; t->done = done;
  t->acts_src = n_acts > 0 ? acts_src : nullptr; t->acts_dst = n_acts > 0 ? acts_dst : nullptr; t->n_acts = n_acts;
  t->disp_dtype = disp_dtype; t->B = B; t->njobs = njobs; t->HW = H * W;
}

// What a fill accepts of assembled bytes before it launches.
inline bool sf_table_sane(const SFTable& f) {
  return f.njobs >= 0 && f.njobs <= TACORL_SF_MAXJOBS && f.B >= 1 && f.HW >= 4 && f.HW % 4 == 0 && f.disp_dtype >= 0 && f.disp_dtype <= 3;
}
