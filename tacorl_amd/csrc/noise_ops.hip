// The noise of a training step from a counter-based generator: every element is a pure function of
// (seed, step, draw id, GLOBAL sample index, position inside the sample), so a step's noise does not depend on how
// many ranks share the batch, and (seed, step) is all a checkpoint has to keep (tacorl_amd/noise.py states the same
// function in NumPy; DESIGN.md "Device noise").  One launch fills every noise buffer of a step.
//
// Philox4x32-10 (Salmon et al., SC'11): key (seed lo, seed hi), counter (q, sample0 + b, draw_id << 16 | k, step) with
// q = j >> 2 the group of four inside the sample's `inner` elements; element j takes word j & 3.
#include <limits.h>

#include "../../include/tacorl_hip.h"
#include "common.h"

#define LAUNCH_OK() (hipGetLastError() == hipSuccess ? TACORL_OK : TACORL_ELAUNCH)

namespace {

constexpr int NOISE_WG = 256;  // threads (= groups of four) per workgroup

struct NoiseTbl {
  int n_seg, n_groups;
  tacorl_noise_seg s[TACORL_NOISE_MAX_SEGS];
};

__device__ __forceinline__ void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

__device__ __forceinline__ float word_uniform(uint32_t w) { return (float)(w >> 8) * 0x1p-24f; }  // [0, 1), exact

// Box-Muller on a word pair: u1 = ((a >> 8) + 1) 2^-24 in (0, 1], angle 2 pi u2 with u2 = (b >> 8) 2^-24.  sincospif
// takes the exact argument 2 u2 (a 24-bit integer times 2^-23), so no fp32 range reduction of 2 pi u2 is involved.
__device__ __forceinline__ void word_pair_normal(uint32_t a, uint32_t b, float& z0, float& z1) {
  const float u1 = (float)((a >> 8) + 1u) * 0x1p-24f;
  const float r = sqrtf(-2.0f * logf(u1));
  float s, c;
  sincospif((float)(b >> 8) * 0x1p-23f, &s, &c);
  z0 = r * c;
  z1 = r * s;
}

// One thread per group of four elements; groups of all segments are numbered densely (s.group0 = groups in front of
// the segment), so every workgroup but the last has 256 groups of work whatever the segments' sizes.
__global__ __launch_bounds__(NOISE_WG) void noise_fill_kernel(NoiseTbl t, float* __restrict__ base_f32,
                                                              unsigned char* __restrict__ base_u8, uint32_t key0,
                                                              uint32_t key1, uint32_t step, uint32_t sample0) {
  const int g = blockIdx.x * NOISE_WG + threadIdx.x;
  if (g >= t.n_groups) return;
  int lo = 0, hi = t.n_seg - 1;  // last segment whose group0 <= g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.s[mid].group0 <= g) lo = mid; else hi = mid - 1;
  }
  const tacorl_noise_seg sg = t.s[lo];
  const int qn = (sg.inner + 3) >> 2;
  const int gl = g - sg.group0;
  const int q = gl % qn, row = gl / qn;  // row: (b, k) in the segment's own order
  int b, k;
  if (sg.outer_major) { k = row / sg.B_local; b = row - k * sg.B_local; }
  else { b = row / sg.n_outer; k = row - b * sg.n_outer; }
  uint32_t w[4] = {(uint32_t)q, sample0 + (uint32_t)b, ((uint32_t)sg.draw_id << 16) | (uint32_t)k, step};
  philox4x32_10(w, key0, key1);
  const int j0 = q << 2;
  const int nj = min(4, sg.inner - j0);
  const long at = (long)sg.offset + (long)row * sg.inner + j0;
  if (sg.kind == TACORL_NOISE_KEEP) {
    unsigned char* d = base_u8 + at;
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (i < nj) d[i] = word_uniform(w[i]) < sg.keep_p ? 1 : 0;
    return;
  }
  float v[4];
  if (sg.kind == TACORL_NOISE_NORMAL) {
    word_pair_normal(w[0], w[1], v[0], v[1]);
    word_pair_normal(w[2], w[3], v[2], v[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = word_uniform(w[i]);
  }
  float* d = base_f32 + at;
  if (nj == 4 && (at & 3) == 0) {  // (base_f32 is 16-byte aligned: checked by the entry point)
    *reinterpret_cast<f32x4*>(d) = f32x4{v[0], v[1], v[2], v[3]};
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; i++)
    if (i < nj) d[i] = v[i];
}

}  // namespace

extern "C" int tacorl_noise_fill(const void* segs, int n_seg, void* base_f32, void* base_u8, unsigned long long seed,
                                 unsigned int step, int sample0, tacorl_stream_t stream) {
  if (segs == nullptr || n_seg < 1 || n_seg > TACORL_NOISE_MAX_SEGS || sample0 < 0) return TACORL_EINVAL;
  const tacorl_noise_table* tab = static_cast<const tacorl_noise_table*>(segs);
  if (tab->n_f32 < 0 || tab->n_u8 < 0 || tab->reserved != 0) return TACORL_EINVAL;
  if (((uintptr_t)base_f32 & 15) != 0) return TACORL_EINVAL;
  NoiseTbl t{};
  t.n_seg = n_seg;
  long groups = 0;
  for (int i = 0; i < n_seg; i++) {
    const tacorl_noise_seg& s = tab->seg[i];
    if (s.kind != TACORL_NOISE_NORMAL && s.kind != TACORL_NOISE_UNIFORM && s.kind != TACORL_NOISE_KEEP) return TACORL_EINVAL;
    if (s.draw_id < 0 || s.draw_id > 65535 || s.n_outer < 1 || s.n_outer > 65535 || s.B_local < 1 || s.inner < 1) return TACORL_EINVAL;
    if (s.outer_major != 0 && s.outer_major != 1) return TACORL_EINVAL;
    if (s.offset < 0 || s.reserved != 0) return TACORL_EINVAL;
    if ((long)sample0 + s.B_local > (long)INT_MAX) return TACORL_EINVAL;
    const long rows = (long)s.n_outer * s.B_local;  // < 2^47
    if (s.inner > INT_MAX / 4 || rows > (long)INT_MAX) return TACORL_EINVAL;
    const long elems = rows * s.inner;  // < 2^62
    const bool u8 = s.kind == TACORL_NOISE_KEEP;
    if (u8 ? base_u8 == nullptr : base_f32 == nullptr) return TACORL_EINVAL;
    if (u8 && !(s.keep_p >= 0.0f && s.keep_p <= 1.0f)) return TACORL_EINVAL;
    if (s.offset + elems > (long)(u8 ? tab->n_u8 : tab->n_f32)) return TACORL_EINVAL;
    if (s.group0 != groups) return TACORL_EINVAL;
    groups += rows * ((s.inner + 3) / 4);
    if (groups > (long)INT_MAX - NOISE_WG) return TACORL_EINVAL;
    t.s[i] = s;
  }
  if (groups != tab->n_groups) return TACORL_EINVAL;
  t.n_groups = (int)groups;
  hipLaunchKernelGGL(noise_fill_kernel, dim3(cdiv(groups, NOISE_WG)), dim3(NOISE_WG), 0, (hipStream_t)stream, t, (float*)base_f32,
                     (unsigned char*)base_u8, (uint32_t)(seed & 0xffffffffull), (uint32_t)(seed >> 32), (uint32_t)step,
                     (uint32_t)sample0);
  return LAUNCH_OK();
}
